"""Every way into a read batch builds the same batch (kv_host.hip build_reads over the plan of kv_reads_layout.h): from ASCII, from
packed words, from a FASTQ file parsed on the device, parsed on the host, and streamed from the packed-read cache.  For the length
vectors of tests/reads_layout_common.py -- the boundaries of the tile rule -- each route's packed words, flags and k-mer numbers are
what the sequences say, and its count tables and scan hits are the oracle's."""
import functools
import os

import numpy as np
import pytest

import reads_layout_common as rl

pytestmark = pytest.mark.gpu

C = rl.constants()
CASES = {name: lens for name, lens in rl.cases(C).items() if lens}
K = 21
CODE = np.zeros(256, dtype=np.uint32)
for _i, _c in enumerate('ACGT'):
    CODE[ord(_c)] = _i


@functools.lru_cache(maxsize=None)
def sequences(name):
    """seeded sequences of the case's lengths; two of the reads carry an N (a batch of one read: that one)"""
    lens = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    letters = np.array(list('ACGT'))
    seqs = [''.join(letters[rng.integers(0, 4, size=n)]) for n in lens]
    with_bases = [i for i, n in enumerate(lens) if n > 0]
    for i in rng.permutation(with_bases)[:2]:
        at = int(rng.integers(0, lens[i]))
        seqs[i] = seqs[i][:at] + 'N' + seqs[i][at + 1:]
    return tuple(seqs)


def packed(seqs):
    """the batch's words: every read starts on a word, base j in bits 2 (j % 16), A for what is not ACGT, zeros behind the end"""
    out = []
    for s in seqs:
        codes = np.zeros((len(s) + 15) // 16 * 16, dtype=np.uint32)
        codes[:len(s)] = CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
        out.append((codes.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def reference(seqs):
    """the oracle's count tables of the reads and the hits of a scan for every k-mer the (empty) control lacks"""
    from oracle import okhmer as ok
    case, ctrl = ok.Counttable(K, 5e4, 4), ok.Counttable(K, 5e4, 4)
    bases, offs = ok.concat_reads(list(seqs))
    n_kmers = ok.consume_reads(case, bases, offs, len(seqs))
    hits, _ = ok.novel_scan([case], [ctrl], bases, offs, len(seqs), K, 1, 0)
    return n_kmers, [case.table_bytes(t) for t in range(4)], hits


def write_fastq(path, seqs):
    with open(path, 'w') as fh:
        for i, s in enumerate(seqs):
            fh.write('@read{}\n{}\n+\n{}\n'.format(i, s, 'I' * len(s)))


def parsed(hk, path, env, want_type, want_cache=False):
    """the file's one batch through ReadParser, by the route the environment asks for -- and by no other"""
    os.environ.update(env)
    try:
        parser = hk.ReadParser(path)
        assert parser.from_cache == want_cache
        tb = parser.text_batch(1000)
        assert type(tb).__name__ == want_type
        assert parser.text_batch(1000) is None            # (a complete pass: with KEVLAR_PACK_CACHE=1 this writes the cache)
        return tb.batch
    finally:
        for key in env:
            os.environ.pop(key, None)


def build(hk, route, seqs, tmp_path):
    if route == 'ascii':
        return hk.ReadBatch(list(seqs))
    if route == 'packed':
        return hk.ReadBatch.from_packed(packed(seqs).reshape(len(seqs), -1), len(seqs[0]))
    path = str(tmp_path / 'reads.fq')
    write_fastq(path, seqs)
    if route == 'fastq_device':
        return parsed(hk, path, {}, 'DeviceTextBatch')
    if route == 'fastq_host':
        return parsed(hk, path, {'KV_INGEST': 'host'}, 'TextBatch')
    parsed(hk, path, {'KEVLAR_PACK_CACHE': '1'}, 'TextBatch').close()
    assert os.path.exists(path + '.kvpack')
    return parsed(hk, path, {'KEVLAR_PACK_CACHE': '1'}, 'TextBatch', want_cache=True)


def routes(name):
    lens = CASES[name]
    out = ['ascii']
    if rl.plan(C, lens)['uni_len']:
        out.append('packed')
    if 0 not in lens:                                       # (a FASTQ record without bases is not what the file routes are about)
        out += ['fastq_device', 'fastq_host', 'fastq_cache']
    return out


def check(hk, route, seqs, tmp_path):
    batch = build(hk, route, seqs, tmp_path)
    words = packed(seqs)
    assert batch.n_reads == len(seqs)
    assert np.array_equal(batch.packed_words(0, len(words)), words)
    with pytest.raises(Exception):
        batch.packed_words(0, len(words) + 1)               # and not a word more
    assert list(batch.flagged_reads()) == [i for i, s in enumerate(seqs) if 'N' in s]
    for k in (21, 31):
        assert batch.num_kmers(k) == sum(max(0, len(s) - k + 1) for s in seqs)
    n_kmers, tables, hits = reference(seqs)
    case, ctrl = hk.Counttable(K, 5e4, 4), hk.Counttable(K, 5e4, 4)
    assert case.consume_batch(batch) == n_kmers
    for t in range(4):
        assert case.table_bytes(t) == tables[t]
    r, o, a, _ = hk.novel_scan([case], [ctrl], batch, 1, 0)
    assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == hits
    batch.close()


@pytest.mark.parametrize('name,route', [(name, route) for name in sorted(CASES) for route in routes(name)])
def test_every_route_builds_the_same_batch(hk, tmp_path, name, route):
    seqs = sequences(name)
    clean = tuple(s.replace('N', 'A') for s in seqs)
    if route != 'packed':                                   # (packed words cannot say N: the stand-in base, and no flag)
        check(hk, route, seqs, tmp_path)
    # the scan skips a read with an N: where that leaves it nothing to find -- a batch of one read -- the read without its N as well
    if route == 'packed' or (clean != seqs and not any('N' not in s for s in seqs)):
        (tmp_path / 'clean').mkdir()
        check(hk, route, clean, tmp_path / 'clean')
