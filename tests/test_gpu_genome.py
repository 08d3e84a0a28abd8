"""The reference genome parsed and kept on the device (kevlar_amd/csrc/kv_genome.hip; kevlar_amd.localize.DeviceGenome) against
today's host path -- seqio.parse_seq_dict + localize.Genome, which tests/test_genome_reference.py holds to the byte-level rule and
to the reference's fixtures -- never against itself: ids, starts, lengths and the whole text of every file of
tests/genome_common.py, in all three containers; the files whose edges sit where a pass over the text ends; the declines; the scan
of the resident text against the scan of the uploaded one; the gather of slices; and `kevlar localize` / `kevlar alac` with the
reference as .fa, .fa.gz and BGZF against the same run handed an open stream."""
import ctypes
import gzip
import io
import os
import random

import numpy as np
import pytest

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd.localize import DeviceGenome, Genome, GenomeDeclined, SeedSet, load_genome, localize
from kevlar_amd.sequence import Record
import kevlar_amd.localize as localize_module

import genome_common as gc
import localize_common as lc

pytestmark = pytest.mark.gpu

HAND = gc.hand_built()
_COMP = str.maketrans('ACGT', 'TGCA')


def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(data)
    return path


def same_as_host(path, text, segment_text=0, container=None):
    """the device genome of the file at `path` (whose text is `text`) equals the host's; returns the passes it took"""
    host = gc.host_genome(text)
    with DeviceGenome(path, segment_text=segment_text) as genome:
        assert genome.on_device and (container is None or genome.container == container)
        assert genome.ids == host.ids
        assert genome.starts.tolist() == host.starts.tolist()
        assert genome.lengths.tolist() == [len(s) for s in host.seqs]
        assert genome.n_text == len(host.text)
        assert genome.fetch_text(0, genome.n_text) == host.text.tobytes()
        return genome.n_segments


# ---- hand-built files
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_built(hk, tmp_path, name):
    same_as_host(put(tmp_path, 'g.fa', HAND[name]), HAND[name], container='plain')


def test_abi_handle(hk, tmp_path):
    lib = _lib.load()
    data = b'>a x\nACGT\nGG\n>b\n\n>c\nTT\n'
    path = put(tmp_path, 'g.fa', data)
    handle = ctypes.c_void_p()
    assert lib.kv_genome_open(path.encode(), 0, ctypes.byref(handle)) == 0
    nseq, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
    stats = (ctypes.c_uint64 * 4)()
    assert lib.kv_genome_info(handle, ctypes.byref(nseq), ctypes.byref(nbytes), stats, None, None, None, None) == 0
    assert (nseq.value, nbytes.value) == (3, len(b'ACGTGG>>TT')) and list(stats)[:3] == [0, 1, len(data)] and stats[3] >= len(data)
    starts, lens = (ctypes.c_uint64 * 4)(0, 7, 8, 5), (ctypes.c_uint64 * 4)(6, 0, 99, 1)
    out, offs = ctypes.create_string_buffer(128), (ctypes.c_uint64 * 5)()
    assert lib.kv_genome_fetch(handle, starts, lens, 4, out, offs) == 0
    assert list(offs) == [0, 6, 6, 8, 9] and out.raw[:9] == b'ACGTGG' + b'TT' + b'G'
    assert lib.kv_genome_close(handle) == 0 and lib.kv_genome_close(None) == 0
    assert lib.kv_genome_open(str(tmp_path / 'missing.fa').encode(), 0, ctypes.byref(handle)) == _lib.KV_ERR_IO
    assert lib.kv_genome_open(None, 0, ctypes.byref(handle)) == _lib.KV_ERR_ARG


def test_duplicate_ids_raise_the_host_s_assertion(hk, tmp_path):
    data = b'>dup a\nAC\n>other\nGG\n>dup b\nTT\n'
    with pytest.raises(AssertionError, match='^dup$'):
        gc.host_genome(data)
    with pytest.raises(AssertionError, match='^dup$'):
        DeviceGenome(put(tmp_path, 'g.fa', data))


# ---- segment edges
@pytest.mark.parametrize('S', [1024, 4096])
def test_segment_edges(hk, tmp_path, S):
    for name, data in gc.segment_cases(S).items():
        passes = same_as_host(put(tmp_path, name + '.fa', data), data, segment_text=S)
        assert passes == -(-len(data) // S), name
    # an interior run of blanks longer than the bound: taken where one pass holds the line, declined where passes end inside it
    path = put(tmp_path, 'over.fa', gc.over_bound(S))
    same_as_host(path, gc.over_bound(S))
    with pytest.raises(GenomeDeclined, match='blanks'):
        DeviceGenome(path, segment_text=S)


def test_hand_built_in_small_segments(hk, tmp_path):
    for name in ('records_3000', 'width_61', 'one_line_100000', 'crlf_mixed', 'defline_runs', 'blank_lines', 'text_in_front'):
        same_as_host(put(tmp_path, name + '.fa', HAND[name]), HAND[name], segment_text=1024)


# ---- seeded files and containers
def test_seeded_plain(hk, tmp_path):
    path = str(tmp_path / 'g.fa')
    for seed in range(gc.N_SEEDED):
        data = gc.seeded(seed)
        with open(path, 'wb') as fh:
            fh.write(data)
        same_as_host(path, data, container='plain')
        if seed % 5 == 0:
            same_as_host(path, data, segment_text=1024)


def test_seeded_containers(hk, tmp_path):
    for seed in range(0, gc.N_SEEDED, 10):
        data = gc.seeded(seed)
        same_as_host(put(tmp_path, 'g.fa.gz', gc.gzip_of(data)), data, container='gzip')
        same_as_host(gc.bgzf_of(data, str(tmp_path / 'b.fa.gz')), data, container='bgzf')
    big = HAND['records_3000'] + HAND['one_line_100000'] + HAND['width_61']
    for S in (0, 4096):
        same_as_host(put(tmp_path, 'big.fa.gz', gc.gzip_of(big)), big, segment_text=S, container='gzip')
        passes = same_as_host(gc.bgzf_of(big, str(tmp_path / 'bigb.fa.gz')), big, segment_text=S, container='bgzf')
        assert passes == (1 if S == 0 else -(-len(big) // 65280))      # (a BGZF pass is one member at least)


# ---- declines
DECLINE_BASE = b'>s1 first\n' + gc.wrap(gc.bases(random.Random(3), 400), 60) + b'>s2\n' + gc.wrap(gc.bases(random.Random(4), 300), 60)
DECLINING_FILES = {
    'high_byte': DECLINE_BASE + b'>s3 caf\xc3\xa9\nACGT\n',
    'sep_1f': DECLINE_BASE.replace(b'\n', b'\x1f\n', 3),
    'nul': DECLINE_BASE + b'>s3 a\x00b\nACGT\n',
    'lone_cr': DECLINE_BASE[:100] + b'\r' + DECLINE_BASE[100:],
}


@pytest.mark.parametrize('name', sorted(gc.declines()))
def test_the_abi_declines(hk, tmp_path, name):
    handle = ctypes.c_void_p()
    path = put(tmp_path, 'g.fa', gc.declines()[name])
    assert _lib.load().kv_genome_open(path.encode(), 0, ctypes.byref(handle)) == _lib.KV_ERR_TYPE
    assert not handle.value and 'host' in _lib.last_error()
    with pytest.raises(GenomeDeclined):
        DeviceGenome(path)


@pytest.mark.parametrize('name', sorted(DECLINING_FILES))
def test_localize_falls_back_to_the_host(hk, tmp_path, name, kevlar_log):
    data = DECLINING_FILES[name]
    assert not gc.device_eligible(data)
    path = put(tmp_path, 'g.fa', data)
    host = gc.host_genome(data)
    parts = [('1', [Record(name='c1', sequence=host.seqs[0][120:260])]), ('2', [Record(name='c2', sequence=host.seqs[1][10:150].translate(_COMP)[::-1])])]
    want = [(p, g.defline, g.sequence) for p, g in localize(parts, io.TextIOWrapper(io.BytesIO(data)), seedsize=31, delta=20)]
    assert localize_module.last_load == {'on_device': False, 'declined': None}
    got = [(p, g.defline, g.sequence) for p, g in localize(parts, path, seedsize=31, delta=20)]
    assert got == want and [d for p, d, s in got] == ['s1_100-280', 's2_0-170']
    assert localize_module.last_load['on_device'] is False and 'host' in localize_module.last_load['declined']
    genome = load_genome(path)
    assert isinstance(genome, Genome) and genome.on_device is False


def test_name_and_content_must_agree_about_gzip(hk, tmp_path):
    data = b'>s1\nACGT\n'
    assert load_genome(put(tmp_path, 'g.fa', data)).on_device is True
    assert load_genome(put(tmp_path, 'h.fa.gz', gc.gzip_of(data))).on_device is True
    with pytest.raises(gzip.BadGzipFile):                     # the host goes by the name, and so does the answer
        load_genome(put(tmp_path, 'plain_named.gz', data))
    assert localize_module.last_load == {'on_device': False, 'declined': None}
    assert load_genome(io.StringIO(data.decode())).on_device is False


# ---- the scan of the resident text
def scan_case(z, seed):
    """(file bytes, contigs): sequences with empty records beside them; seeds from the first and the last window of a sequence on
    either strand, from the middle, beside the empty records, twice in the genome, and one across a junction (never matches)"""
    rng = random.Random(seed)
    dna = lambda n: gc.bases(rng, n).decode()                         # noqa: E731
    rc = lambda s: s.translate(_COMP)[::-1]                           # noqa: E731
    s1, s2, s3 = dna(3 * z + 40), dna(z), dna(2 * z + 5)
    repeat = dna(z + 3)
    s4 = dna(10) + repeat + dna(25) + rc(repeat) + dna(7)
    data = ('>e0\n>s1\n' + s1 + '\n>e1\n>e2\n\n>s2\n' + s2 + '\n>s3\n' + gc.wrap(s3.encode(), 60).decode() + '>e3\n>s4\n' + s4 + '\n>short\n' + dna(z - 1) + '\n>e4\n').encode()
    contigs = [s1[:z], rc(s1[-z:]), s1[z:2 * z + 9], s2, rc(s3[:z + 4]), s3[-z:], repeat, s1[-(z // 2):] + s2[:z - z // 2], s2[-(z // 2):] + '>' + s3[:z],
               dna(z + 5), s4[-z:].lower()]
    return data, contigs


def sorted_pairs(seedset, ids, pos):
    """the matches as sorted (seed, position) pairs and the occurrences per seed: by the seed's sequence, because which of a
    seed's windows lends it its id is settled anew in every seed set"""
    pairs = sorted((seedset.sequence(i), int(p)) for i, p in zip(ids.tolist(), pos.tolist()))
    return pairs, {seedset.sequence(i): int(c) for i, c in enumerate(seedset.counts()) if c}


@pytest.mark.parametrize('z', [13, 51, 128])
def test_scan_genome_equals_the_scan_of_the_uploaded_text(hk, tmp_path, z):
    data, contigs = scan_case(z, z)
    host = gc.host_genome(data)
    with SeedSet(contigs, z) as seedset:
        want, want_counts = sorted_pairs(seedset, *seedset.scan(host.text))
    positions = {p for seed, p in want}
    for i, seq in enumerate(host.seqs):                               # what was planted is found: first and last windows, both strands
        if host.ids[i] in ('s1', 's2', 's3', 's4'):
            assert int(host.starts[i]) in positions or host.ids[i] == 's4'
            assert int(host.starts[i]) + len(seq) - z in positions
    assert len(want) >= 12 + 2 and max(want_counts.values()) == 2 and len(set(want)) == len(want)
    with DeviceGenome(put(tmp_path, 'g.fa', data)) as genome:
        for chunk in (0, z, z + 1, 4096, 64 + z - 1):
            with SeedSet(contigs, z) as seedset:
                got, counts = sorted_pairs(seedset, *seedset.scan_genome(genome, chunk_bytes=chunk))
                assert got == want, chunk
                assert counts == want_counts, chunk
                if chunk == 0:                                        # the same seed set once more: the counters go on counting
                    again, counts = sorted_pairs(seedset, *seedset.scan_genome(genome))
                    assert again == want and counts == {seed: 2 * c for seed, c in want_counts.items()}
        with SeedSet(contigs, z) as seedset:                          # room for one match: the call is repeated, nothing counted twice
            got, counts = sorted_pairs(seedset, *seedset.scan_genome(genome, chunk_bytes=z + 1, capacity=1))
            assert got == want and counts == want_counts
            assert seedset.stats()[2] == len(want)


def test_scan_genome_of_nothing(hk, tmp_path):
    with DeviceGenome(put(tmp_path, 'g.fa', b'')) as genome, SeedSet(['ACGTACGTACGTACGT'], 13) as seedset:
        ids, pos = seedset.scan_genome(genome)
        assert len(ids) == 0 and len(pos) == 0
    with DeviceGenome(put(tmp_path, 'h.fa', b'>s\nACGTACGTACGT\n')) as genome, SeedSet(['ACGTACGTACGTACGT'], 13) as seedset:
        assert len(seedset.scan_genome(genome)[0]) == 0             # twelve bases: no window


# ---- slices
def test_fetch_many(hk, tmp_path):
    data = HAND['empty_records_beside'] + HAND['records_3000'][:20000].rsplit(b'>', 1)[0] + b'>long\n' + gc.bases(random.Random(8), 5000) + b'\n>last_empty\n'
    host = gc.host_genome(data)
    rng = random.Random(9)
    with DeviceGenome(put(tmp_path, 'g.fa', data)) as genome:
        n = len(genome.ids)
        empty = [i for i in range(n) if genome.lengths[i] == 0]
        long_one = genome.ids.index('long')
        requests = [(long_one, 0, 0), (long_one, 0, 10), (long_one, 4990, 5000), (long_one, 4990, 9999), (long_one, 0, 5000), (long_one, 6000, 7000),
                    (long_one, -5, 3), (empty[0], 0, 0), (empty[0], 0, 50), (empty[-1], 3, 9), (0, 0, 1)]
        while len(requests) < 2000:
            i = rng.randrange(n)
            length = int(genome.lengths[i])
            a = rng.randint(-3, length + 3)
            requests.append((i, a, a + rng.choice((0, 1, 15, 16, 17, 100, length))))
        got = genome.fetch_many(requests)
        assert len(got) == 2000
        for (i, a, b), piece in zip(requests, got):
            assert piece == host.seqs[i][max(a, 0):max(b, 0)], (i, a, b)
        assert genome.fetch_many([]) == []
        # the lazy sequences of seqdict(): len() and slices as a str has them
        seqs = genome.seqdict()
        assert list(seqs) == host.ids
        for seqid in ('long', 'last_empty', 's1', 'e2'):
            lazy, real = seqs[seqid], host.seqdict()[seqid]
            assert len(lazy) == len(real) and str(lazy) == real
            for key in (slice(0, 10), slice(None, None), slice(-7, None), slice(5, 2), slice(4990, 10 ** 9), slice(-10 ** 9, 3), slice(0, 40, 3)):
                assert lazy[key] == real[key], (seqid, key)
            if real:
                assert lazy[0] == real[0] and lazy[-1] == real[-1]
        # a collector notes the slices; one resolve fetches them all
        noted = []
        seqs = genome.seqdict(noted)
        pieces = [seqs['long'][100:200], seqs['s1'][2:9], seqs['e2'][0:5]]
        assert [len(p) for p in pieces] == [100, 7, 0] and all(p.value is None for p in pieces)
        genome.resolve(noted)
        assert [p.value for p in pieces] == [host.seqdict()['long'][100:200], host.seqdict()['s1'][2:9], '']


# ---- end to end
def containers_of(path, tmp_path, stem):
    """the reference FASTA at `path` as .fa, as one gzip stream and re-blocked as BGZF"""
    text = gc.file_text(path)
    assert gc.device_eligible(text)
    return {'plain': put(tmp_path, stem + '.fa', text), 'gzip': put(tmp_path, stem + '.fa.gz', gc.gzip_of(text)),
            'bgzf': gc.bgzf_of(text, str(tmp_path / (stem + '.bgzf.fa.gz')))}


@pytest.mark.parametrize('refr,contigs,flags', [('fiveparts-refr.fa.gz', 'fiveparts.contigs.augfasta.gz', []),
                                                ('localize-refr.fa', 'localize-contig.fa', ['--seed-size', '23', '--delta', '50']),
                                                ('maxdiff-refr.fa.gz', 'maxdiff-contig.augfasta', ['--seed-size', '51', '--max-diff', '5000'])])
def test_localize_command_line(hk, tmp_path, capsys, kevlar_log, refr, contigs, flags):
    paths = containers_of(lc.fixture(refr), tmp_path, 'refr')
    args = kevlar_amd.cli.parser().parse_args(['localize'] + flags + [paths['plain'], lc.fixture(contigs)])
    args.refr = io.TextIOWrapper(io.BytesIO(gc.file_text(lc.fixture(refr))))         # an open stream: the host path
    kevlar_amd.localize.main(args)
    want = capsys.readouterr().out
    assert localize_module.last_load['on_device'] is False and want.count('>') >= 1
    for container, path in paths.items():
        kevlar_amd.cli.run(['localize'] + flags + [path, lc.fixture(contigs)])
        assert capsys.readouterr().out == want, container
        assert localize_module.last_load == {'on_device': True, 'declined': None, 'container': container}
    kevlar_amd.cli.run(['localize'] + flags + [lc.fixture(refr), lc.fixture(contigs)])       # the fixture as it is
    assert capsys.readouterr().out == want and localize_module.last_load['on_device'] is True


def test_alac_command_line(hk, tmp_path, capsys, kevlar_log):
    import assemble_common as ac
    from kevlar_amd.alac import alac
    reads, refr = ac.fixture_path('fiveparts.augfastq.gz'), ac.fixture_path('fiveparts-refr.fa.gz')
    stream = kevlar_amd.parse_partitioned_reads(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(reads, 'r')))
    want = [call.vcf for call in alac(stream, io.TextIOWrapper(io.BytesIO(gc.file_text(refr))), seedsize=31)]
    assert localize_module.last_load['on_device'] is False and len(want) >= 5
    outputs = {}
    for container, path in containers_of(refr, tmp_path, 'refr').items():
        out = str(tmp_path / (container + '.vcf'))
        kevlar_amd.cli.run(['alac', '--seed-size', '31', '-o', out, reads, path])
        assert localize_module.last_load == {'on_device': True, 'declined': None, 'container': container}
        text = open(out).read()
        assert [line for line in text.split('\n') if line and not line.startswith('#')] == want, container
        outputs[container] = text.replace(path, 'REFR')
    assert outputs['plain'] == outputs['gzip'] == outputs['bgzf']
