"""The two device inflaters (kv_inflate.hip: one wavefront per BGZF member; kv_gunzip.hip: the speculative parallel decoder
of an ordinary gzip stream) on the hand-assembled DEFLATE streams of tests/deflate_common.py, against zlib's inflate byte for
byte: every length and distance symbol, the deepest codes, every run of the code-length alphabet, empty blocks, stored blocks
on every bit phase, copies on either side of the LDS ring, tails of nothing but markers, false block starts, 300 members, and
the part of zlib's own space gzip.compress() does not write.  What zlib refuses both inflaters must refuse; what it accepts
they must inflate -- a decline ("no DEFLATE block start", "too many stretches needed decoding again") is a failure here:
every input is far below the 4 MB search margin.  tests/test_deflate_streams.py holds the same catalogue to zlib on the host.

KV_GUNZIP_CHUNK_KB (the block search's chunk; 16 by default) is set to 1 so that a stream of a few KB is cut into as many
stretches, false starts, marker chains and repairs as a real file of gigabytes, and to 64 for the false starts of group 13."""
import contextlib
import os

import pytest

import deflate_common as dc
from test_gpu_ingest import device_gunzip, device_inflate

pytestmark = pytest.mark.gpu

DECLINES = ('no DEFLATE block start', 'too many stretches needed decoding again')


@contextlib.contextmanager
def chunk_kb(value):
    old = os.environ.pop('KV_GUNZIP_CHUNK_KB', None)
    if value:
        os.environ['KV_GUNZIP_CHUNK_KB'] = str(value)
    try:
        yield
    finally:
        os.environ.pop('KV_GUNZIP_CHUNK_KB', None)
        if old is not None:
            os.environ['KV_GUNZIP_CHUNK_KB'] = old


def errors():
    from kevlar_amd import _lib
    return (ValueError, OSError, _lib.KvError)


def gunzip_all(cases, chunks, segments):
    """every (name, gzip image, text) through kv_gunzip_host at every chunk size and segment size: the failures"""
    failed = []
    for name, image, text in cases:
        for chunk in chunks:
            for segment in segments:
                with chunk_kb(chunk):
                    try:
                        got, stats = device_gunzip(image, segment, cap=len(text) + 64)
                    except errors() as exc:
                        declined = any(d in str(exc) for d in DECLINES)
                        failed.append((name, chunk, segment, 'DECLINED' if declined else 'refused', str(exc)[:120]))
                        continue
                if got != text:
                    at = next((i for i in range(min(len(got), len(text))) if got[i] != text[i]), min(len(got), len(text)))
                    failed.append((name, chunk, segment, 'text differs', 'lengths {} {}, first at {}'.format(len(got), len(text), at)))
    return failed


def refused_all(cases, chunks, segments):
    """every (name, gzip image) that must be an error: the ones that delivered text"""
    delivered = []
    for name, image, cap in cases:
        for chunk in chunks:
            for segment in segments:
                with chunk_kb(chunk):
                    try:
                        got, _ = device_gunzip(image, segment, cap=cap)
                    except errors():
                        continue
                delivered.append((name, chunk, segment, len(got)))
    return delivered


@pytest.mark.parametrize('name', dc.GROUPS)
def test_gunzip_inflates_what_zlib_accepts(hk, name):
    wide = name == 'false'                             # group 13 also at the largest chunk and a third segment size
    cases = [(case, dc.gzip_member(raw, text), text) for case, raw, text in dc.group(name)]
    failed = gunzip_all(cases, (None, 1, 64) if wide else (None, 1), (0, 20000, 100000) if wide else (0, 20000))
    assert not failed, failed


def test_gunzip_cuts_the_small_streams_into_many_stretches(hk):
    """the chunk size does what the tests above rely on: 1 KB chunks turn the 60 KB of group 12 into hundreds of stretches"""
    case, raw, text = dc.group('chains')[0]
    image = dc.gzip_member(raw, text)
    with chunk_kb(1):
        got, small = device_gunzip(image, 0, cap=len(text) + 64)
    got_default, default = device_gunzip(image, 0, cap=len(text) + 64)
    assert got == text and got_default == text
    assert small[1] >= 128 and small[1] > 2 * default[1], (small, default)


@pytest.mark.parametrize('name', [g for g in dc.GROUPS if any(dc.fits_bgzf(raw, text) for _, raw, text in dc.group(g))])
def test_bgzf_inflates_what_zlib_accepts(hk, name):
    fitting = [(case, raw, text) for case, raw, text in dc.group(name) if dc.fits_bgzf(raw, text)]
    image = b''.join(dc.bgzf_member(raw, text) for _, raw, text in fitting) + dc.BGZF_EOF
    got, members, _ = device_inflate(image)
    assert members == len(fitting) + 1
    at = 0
    for case, _, text in fitting:
        assert got[at:at + len(text)] == text, case
        at += len(text)
    assert at == len(got)


def test_gunzip_refuses_what_zlib_refuses(hk):
    cases = [(case, dc.gzip_member(raw, dc.LENIENT[case]), len(dc.LENIENT[case]) + 4096) for case, raw, _ in dc.group('rejected')]
    delivered = refused_all(cases, (None, 1), (0, 20000))
    assert not delivered, delivered


def test_bgzf_refuses_what_zlib_refuses(hk):
    good = dc.bgzf_member(*dc.group('copies')[0][1:])
    delivered = []
    for case, raw, _ in dc.group('rejected'):
        image = good + dc.bgzf_member(raw, dc.LENIENT[case]) + good + dc.BGZF_EOF
        try:
            got, _, _ = device_inflate(image)
        except errors():
            continue
        delivered.append((case, len(got)))
    assert not delivered, delivered
    assert device_inflate(good + good + dc.BGZF_EOF)[0] == dc.group('copies')[0][2] * 2


def test_gunzip_whole_files(hk):
    """300 members of 100 bytes (the CRC-32 of the members may go unchecked, the sizes may not), one of them with another ISIZE,
    a header with every optional field in the middle of the file, a member behind the stream of false starts"""
    accepted = [(case, image, text) for case, image, text in dc.IMAGES if text is not None]
    failed = gunzip_all(accepted, (None, 1, 64), (0, 20000, 100000))
    assert not failed, failed
    refused = [(case, image, 1 << 20) for case, image, text in dc.IMAGES if text is None]
    assert refused
    delivered = refused_all(refused, (None, 1), (0, 20000))
    assert not delivered, delivered


@pytest.mark.parametrize('kind', ['fastq', 'runs', 'periodic'])
@pytest.mark.parametrize('strategy', sorted(dc.STRATEGIES))
def test_gunzip_inflates_what_zlib_writes_beyond_gzip_compress(hk, strategy, kind):
    cases = [(case, dc.gzip_member(raw, text), text) for case, raw, text in dc.zlib_space(strategy) if ' {} '.format(kind) in case]
    assert len(cases) == 6
    failed = gunzip_all(cases, (None, 1, 64), (0, 20000, 100000))
    assert not failed, failed
