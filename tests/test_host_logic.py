"""CPU-side checks: the C-ABI library loads and exports every declared symbol, the product
fails loudly without a GPU, and the host logic (augfastx codec, seqio, CLI, unband, timers)
matches the reference's own expectations.  No kernel is launched here."""
import io
import os
import re

import numpy as np
import pytest

from conftest import ROOT, data_file, expected_file


def test_cabi_library_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    from kevlar_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'kvsketch.h')).read()
    declared = set(re.findall(r'\b(kv_[a-z0-9_]+)\s*\(', header))
    assert declared, 'no declarations found'
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert b'gfx950' in lib.kv_version()


def test_host_helpers_need_no_gpu(ok):
    """prime picking, single k-mer hashing and band bounds are host code in the library."""
    import ctypes
    from kevlar_amd import _lib, khmer
    lib = _lib.load()
    assert khmer.primes_below(2500, 4) == [2477, 2473, 2467, 2459]
    assert khmer.primes_below(2e5, 4) == ok.primes_below(2e5, 4)
    for target in (3, 4, 10, 97 / 4, 1e6 / 4, 12345.9):
        assert khmer.primes_below(target, 4) == ok.primes_below(target, 4)
    out = ctypes.c_uint64()
    for kmer in ('GATTACAGATTACAGATTACA', 'A' * 31, ('ACGTTGCA' * 7)[:51]):
        assert lib.kv_hash_kmer(0, kmer.encode(), len(kmer), ctypes.byref(out)) == 0
        assert out.value == ok.Counttable(len(kmer), 100, 1).hash(kmer)
    assert lib.kv_hash_kmer(3, b'GATTACAGATTACAGATTACA', 21, ctypes.byref(out)) == 0
    assert out.value == ok.Countgraph(21, 100, 1).hash('GATTACAGATTACAGATTACA')
    assert lib.kv_hash_kmer(0, b'GATTACANATTACAGATTACA', 21, ctypes.byref(out)) == 0   # murmur takes any byte
    assert lib.kv_hash_kmer(3, b'GATTACANATTACAGATTACA', 21, ctypes.byref(out)) == _lib.KV_ERR_ARG
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.kv_band_bounds(8, 0, ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert (lo.value, hi.value) == ok.band_bounds(8, 0)
    assert lib.kv_band_bounds(8, 8, ctypes.byref(lo), ctypes.byref(hi)) == _lib.KV_ERR_ARG


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    from kevlar_amd import khmer, _lib
    with pytest.raises(_lib.KvError, match='no HIP device'):
        khmer.Counttable(31, 1e6, 4)
    with pytest.raises(_lib.KvError, match='no HIP device'):
        khmer.ReadBatch(['ACGT'])


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under kevlar_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'kevlar_amd')):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, fn)).read()
                assert 'okhmer' not in text and 'kvoracle' not in text and 'from oracle' not in text, fn


def test_memory_setting_and_cli_defaults():
    import kevlar_amd
    ms = kevlar_amd.khmer.khmer_args.memory_setting
    assert ms('10K') == 1e4 and ms('500M') == 5e8 and ms('1e7') == 1e7 and ms('2g') == 2e9
    with pytest.raises(ValueError):
        ms('12Q')
    args = kevlar_amd.cli.parser().parse_args(['novel', '--case', 'case1.fq', '--control', 'cntl1.fq',
                                               '--control', 'cntl2.fq', '-k', '17'])
    assert (args.ksize, args.case_min, args.ctrl_max, args.num_bands, args.band) == (17, 6, 1, None, None)
    args = kevlar_amd.cli.parser().parse_args(['novel', '--num-bands', '8', '--band', '1', '--case', 'case1.fq',
                                               '--control', 'cntl1.fq', '--control', 'cntl2.fq'])
    assert (args.ksize, args.num_bands, args.band) == (31, 8, 1)
    args = kevlar_amd.cli.parser().parse_args(['count', 'out.ct', 'in.fq'])
    assert (args.ksize, args.counter_size, args.memory, args.max_fpr, args.threads) == (31, 8, 1e6, 0.2, 1)
    args = kevlar_amd.cli.parser().parse_args(['filter', 'in.augfastq'])
    assert (args.memory, args.max_fpr, args.ctrl_max, args.case_min) == (1e6, 0.01, 1, 6)
    args = kevlar_amd.cli.parser().parse_args(['partition', 'in.augfastq'])
    assert (args.min_abund, args.max_abund, args.dedup, args.strict) == (2, 200, True, False)
    args = kevlar_amd.cli.parser().parse_args(['unband', 'a', 'b'])
    assert args.n_batches == 16 and args.infile == ['a', 'b']
    args = kevlar_amd.cli.parser().parse_args(['dist', 'mask.nt', 'a.fq', 'b.fq'])
    assert (args.ksize, args.memory, args.threads, args.plot_xlim, args.infiles) == (31, 1e6, 1, (0, 100), ['a.fq', 'b.fq'])
    assert set(kevlar_amd.cli.mains) == {'count', 'novel', 'filter', 'partition', 'unband', 'dist', 'split', 'augment', 'gentrio'}
    assert kevlar_amd.sketch.get_extension() == ('.nt', '.nodetable')
    assert kevlar_amd.sketch.get_extension(count=True) == ('.ct', '.counttable')
    assert kevlar_amd.sketch.get_extension(count=True, smallcount=True) == ('.sct', '.smallcounttable')


def test_augfastx_reader():
    """kevlar/tests/test_seqio.py:46-132."""
    import kevlar_amd
    n = -1
    for n, record in enumerate(kevlar_amd.parse_augmented_fastx(open(data_file('collect.beta.1.txt')))):
        assert record.name.startswith('good')
        assert record.sequence == 'TTAACTCTAGATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCT'
        assert len(record.annotations) == 2
        assert all(k.abund == (8, 0, 0) for k in record.annotations)
    assert n == 7
    record = next(kevlar_amd.parse_augmented_fastx(open(data_file('example1.augfastq'))))
    assert record.name == 'e1' and len(record.annotations) == 2
    ik = record.annotations[0]
    assert (record.ikmerseq(ik), ik.ksize, ik.offset, ik.abund) == ('AGGGGCGTGACTTAATAAG', 19, 13, (12, 15, 1, 1))
    ik = record.annotations[1]
    assert (record.ikmerseq(ik), ik.offset, ik.abund) == ('GGGCGTGACTTAATAAGGT', 15, (20, 28, 0, 1))
    record = next(kevlar_amd.parse_augmented_fastx(open(data_file('example2.augfastq'))))
    assert record.name == 'ERR894724.125497791/1'
    assert [(k.ksize, k.offset, k.abund) for k in record.annotations] == [(31, 74, (23, 0, 0)), (31, 83, (23, 0, 0))]
    reader = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(data_file('seqs-mates.augfastq'), 'r'))
    shape = [(len(r.annotations), len(r.mates)) for r in reader]
    assert shape == [(5, 1), (4, 1), (21, 0), (2, 1)]


def test_augfastx_writer_golden_text():
    """kevlar/tests/test_seqio.py:135-182: the literal expected output."""
    import kevlar_amd
    from kevlar_amd.sequence import KmerOfInterest, Record
    output = io.StringIO()
    kevlar_amd.print_augmented_fastx(Record(
        name='BasiliscusVulgarisRead84467/1', sequence='TTAACTCTAGATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCT',
        quality='B' * 50, annotations=[KmerOfInterest(19, 13, (12, 1, 1)), KmerOfInterest(19, 15, (20, 0, 1))]), output)
    kevlar_amd.print_augmented_fastx(Record(
        name='BasiliscusVulgarisRead90577/2', sequence='CTGTAATCCCAGCACTTTGGGAGGCCGAGGCAAGCAGATGATGCGGTCAG',
        quality='B' * 50, annotations=[KmerOfInterest(19, 1, (5, 7, 9)), KmerOfInterest(19, 2, (7, 10, 9))],
        mates=['CAGATGTGTCTTGTGGGCAGTGCAGCGGAGAGGTGCAAATATGGGTTTGG']), output)
    kevlar_amd.print_augmented_fastx(Record(
        name='BasiliscusVulgarisRead99037/1', sequence='AGCACTTTGGGAGGCCGAGGCAAGCAGATGATGCGGTCAGGATTACAGAT',
        quality='B' * 50), output)
    assert output.getvalue() == (
        '@BasiliscusVulgarisRead84467/1\nTTAACTCTAGATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCT\n+\n' + 'B' * 50 + '\n'
        '             AGGGGCGTGACTTAATAAG          12 1 1#\n'
        '               GGGCGTGACTTAATAAGGT          20 0 1#\n'
        '@BasiliscusVulgarisRead90577/2\nCTGTAATCCCAGCACTTTGGGAGGCCGAGGCAAGCAGATGATGCGGTCAG\n+\n' + 'B' * 50 + '\n'
        ' TGTAATCCCAGCACTTTGG          5 7 9#\n'
        '  GTAATCCCAGCACTTTGGG          7 10 9#\n'
        '#mateseq=CAGATGTGTCTTGTGGGCAGTGCAGCGGAGAGGTGCAAATATGGGTTTGG#\n'
        '@BasiliscusVulgarisRead99037/1\nAGCACTTTGGGAGGCCGAGGCAAGCAGATGATGCGGTCAGGATTACAGAT\n+\n' + 'B' * 50 + '\n')


@pytest.mark.parametrize('name', ['novel-trio-li.augfastq', 'filter-trio1-masked.augfastq', 'novel-screen.augfasta',
                                  'unband-helium.sorted.augfastq'])
def test_augfastx_roundtrip_is_byte_exact(name):
    """parse -> print reproduces files written by the reference's own (Cython) codec."""
    import kevlar_amd
    text = open(expected_file(name)).read()
    buf = io.StringIO()
    for rec in kevlar_amd.parse_augmented_fastx(io.StringIO(text)):
        kevlar_amd.print_augmented_fastx(rec, buf)
    assert buf.getvalue() == text


def test_kmer_rep_in_read_and_revcom():
    import kevlar_amd
    read = 'AGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGATGAGGAT'
    record = kevlar_amd.sequence.Record(name='reqseq', sequence=read)
    record.annotate('GATGAGGATGAGGATGAGGATGAGG', 2, (11, 1, 0))
    record.annotate('GATGAGGATGAGGATGAGGATGAGG', 8, (11, 1, 0))
    assert read in kevlar_amd.sequence.format_augmented_fastx(record)
    assert kevlar_amd.revcom('AACGTN') == 'NACGTT'
    assert kevlar_amd.revcommin('TTTT') == 'AAAA' and kevlar_amd.revcommin('ACGG') == 'ACGG'
    with pytest.raises(AssertionError):
        record.annotate('CCCC', 0, (1,))


def test_seqio_partition_readers():
    import kevlar_amd
    lines = '>seq1\nACGT\n>seq2 yo\nGATTACA\nGATTACA\n>seq3\tdescrip\nATGATGTGA'.split('\n')
    assert dict(kevlar_amd.seqio.parse_fasta(lines)) == {'>seq1': 'ACGT', '>seq2 yo': 'GATTACAGATTACA',
                                                         '>seq3\tdescrip': 'ATGATGTGA'}
    assert kevlar_amd.seqio.parse_seq_dict(lines) == {'seq1': 'ACGT', 'seq2': 'GATTACAGATTACA', 'seq3': 'ATGATGTGA'}
    stream = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(data_file('part-reads-simple.fa'), 'r'))
    parts = [p for _, p in kevlar_amd.parse_partitioned_reads(stream)]
    assert [len(p) for p in parts] == [4, 2]
    stream = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(data_file('part-reads-mixed.fa'), 'r'))
    with pytest.raises(kevlar_amd.seqio.KevlarPartitionLabelError, match='with and without partition labels'):
        list(kevlar_amd.parse_partitioned_reads(stream))


def test_unband_golden():
    """kevlar/tests/test_unband.py:15-45 (host-side merge; the golden file is name-sorted)."""
    import kevlar_amd
    infiles = [data_file('helium-unband/novel.band{}.augfastq.gz'.format(i)) for i in (1, 2, 3, 4)]
    reads = sorted(kevlar_amd.unband.unband(kevlar_amd.seqio.afxstream(infiles), numbatches=16), key=lambda r: r.name)
    assert len(reads) == 135
    some = [r for r in reads if r.name == 'seq1_haplo1_285110_285519_1:0:0_0:0:0_2dbcd/1'][0]
    assert len(some.annotations) == 75
    buf = io.StringIO()
    for rec in reads:
        kevlar_amd.print_augmented_fastx(rec, buf)
    assert buf.getvalue() == open(expected_file('unband-helium.sorted.augfastq')).read()
    beta = [data_file('collect.beta.{}.txt'.format(i)) for i in (1, 2)]
    merged = sorted(kevlar_amd.unband.unband(kevlar_amd.seqio.afxstream(beta), numbatches=2), key=lambda r: r.name)
    assert len(merged) == 8 and len(merged[0].annotations) == 4


def test_timer_progress_and_logging(capsys):
    import kevlar_amd
    timer = kevlar_amd.Timer()
    timer.start()
    timer.start('x')
    with pytest.raises(ValueError, match='Timer already started'):
        timer.start('x')
    with pytest.raises(ValueError, match='No timer started'):
        timer.stop('y')
    assert timer.probe('x') >= 0 and timer.stop('x') >= 0 and timer.stop() >= 0
    buf = io.StringIO()
    old = kevlar_amd.logstream
    kevlar_amd.logstream = buf
    try:
        pi = kevlar_amd.ProgressIndicator('processed {counter}', interval=10, breaks=[100, 1000])
        for _ in range(1500):
            pi.update()
    finally:
        kevlar_amd.logstream = old
    lines = buf.getvalue().strip().split('\n')
    assert lines[0] == 'processed 10' and 'processed 100' in lines and lines[-1] == 'processed 1000'
    assert len(lines) == 10 + 9
    with pytest.raises(ValueError, match='invalid mode'):
        kevlar_amd.open('x', 'a')


def test_synthetic_trio_generator_properties():
    from kevlar_amd import synth
    trio = synth.make_trio(200000, 42)
    again = synth.make_trio(200000, 42)
    assert all(np.array_equal(a, b) for n in trio for a, b in zip(trio[n], again[n]))
    words = synth.sample_reads_packed(trio['proband'], 2000, 100, 0.0, 7)
    assert np.array_equal(words, synth.sample_reads_packed(trio['proband'], 2000, 100, 0.0, 7))
    haps = [''.join('ACGT'[c] for c in h) for h in trio['proband']]
    rc = lambda s: s[::-1].translate(str.maketrans('ACGT', 'TGCA'))  # noqa: E731
    for read in synth.unpack_reads(words[:100], 100):
        assert len(read) == 100 and any(read in h or rc(read) in h for h in haps)
    noisy = synth.unpack_reads(synth.sample_reads_packed(trio['proband'], 2000, 100, 0.005, 7), 100)
    clean = synth.unpack_reads(words, 100)
    diff = sum(a != b for x, y in zip(noisy, clean) for a, b in zip(x, y))
    assert 600 < diff < 1400            # ~0.5 % of 200k bases


def test_readgraph_strict_mode_edges_and_cli(tmp_path):
    """kevlar/tests/test_readgraph.py:20-31 strict edge counts (the reference asserts 11 and 12 +-1;
    its own drivers give 11 and 11, tests/golden/expected/manifest.json) -- strict mode is host-side."""
    import json
    import kevlar_amd
    want = json.load(open(expected_file('manifest.json')))['readgraph_edges']
    for infile, approx in [('connectivity-1311.augfastq', 11), ('connectivity-1541.augfastq', 12)]:
        with open(data_file(infile)) as fh:
            reads = list(kevlar_amd.parse_augmented_fastx(fh))
        rg = kevlar_amd.ReadGraph()
        rg.load(reads)
        rg.populate_edges(strict=True)
        # the reference's count depends on Python set order (which read of a tied pair receives the
        # self-loop); its own test allows +-100 %.  Components are order-free and compared below.
        assert abs(rg.number_of_edges() - want[infile]['strict']) <= 2
        assert abs(rg.number_of_edges() - approx) <= 2
    import io
    for name, infile, extra in [('partition-conn1311-strict', 'connectivity-1311.augfastq', ['--strict']),
                                ('partition-conn1541-strict-nodedup', 'connectivity-1541.augfastq', ['--strict', '--no-dedup']),
                                ('partition-pico-strict', 'pico-filtered.fq.gz', ['--strict'])]:
        gold = json.load(open(expected_file(name + '.json')))
        args = kevlar_amd.cli.parser().parse_args(['partition'] + extra + ['-o', str(tmp_path / 'out.augfastq'), data_file(infile)])
        log = io.StringIO()
        old, kevlar_amd.logstream = kevlar_amd.logstream, log
        try:
            kevlar_amd.partition.main(args)
        finally:
            kevlar_amd.logstream = old
        got = {}
        for rec in kevlar_amd.parse_augmented_fastx(open(str(tmp_path / 'out.augfastq'))):
            pid = kevlar_amd.seqio.partition_id(rec.name)
            got.setdefault(pid, []).append(kevlar_amd.revcommin(rec.sequence))
        assert sorted(got) == sorted(gold['partitions'])
        for pid in got:
            assert sorted(set(got[pid])) == sorted(set(seq for _, seq in gold['partitions'][pid]))
        assert gold['log'][0].split('] ')[-1] in log.getvalue()
    # readpair known answers in the spirit of kevlar/tests/test_readpair.py: a perfect overlap merges,
    # a mismatch inside the overlap does not
    from kevlar_amd.readpair import merged_sequence
    from kevlar_amd.sequence import KmerOfInterest, Record
    k = 'GGGCGTGACTTAATAAGGT'
    a = Record('a', 'TTAACTCTAGATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCT', annotations=[KmerOfInterest(19, 15, (20, 0, 0))])
    b = Record('b', 'GATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCTAACGTTTAC', annotations=[KmerOfInterest(19, 6, (20, 0, 0))])
    assert kevlar_amd.revcommin(merged_sequence(a, b, k)) == kevlar_amd.revcommin(
        'TTAACTCTAGATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGTCTAACGTTTAC')
    brc = Record('brc', kevlar_amd.revcom(b.sequence), annotations=[KmerOfInterest(19, 50 - 6 - 19, (20, 0, 0))])
    assert merged_sequence(a, brc, k) is not None
    c = Record('c', 'GATTAGGGGCGTGACTTAATAAGGTGTGGGCCTAAGCGACTAACGTTTAC', annotations=[KmerOfInterest(19, 6, (20, 0, 0))])
    assert merged_sequence(a, c, k) is None


def test_native_fastx_reader_matches_record_parser(ok, tmp_path):
    """kv_fastx_* (zlib + C++ record splitter) vs the oracle's plain Python reader on the reference's
    own FASTA/FASTQ fixtures, plus CRLF / no-trailing-newline / blank-line handling."""
    from kevlar_amd import khmer
    files = ['trio1/case1.fq.gz', 'bogus-genome/refr.fa', 'simple-genome-case-reads.fa.gz', 'ambig.fasta',
             'screen-case.fa', 'microtrios/trio-li-proband.fq.gz', 'bogus-genome/mask-chr1.fa']
    for rel in files:
        got = [(r.name, r.sequence, r.quality) for r in khmer.ReadParser(data_file(rel))]
        want = [(r.name, r.sequence, r.quality) for r in ok.ReadParser(data_file(rel))]
        assert got == want and len(got) > 0, rel
        parser = khmer.ReadParser(data_file(rel))
        total = sum(tb.n for tb in parser.text_batches(1000, upload=False))
        assert total == len(want) == parser.num_reads
    odd = tmp_path / 'odd.fx'
    odd.write_bytes(b'@q1\r\nGATTACA\r\n+\r\n@@@IIII\r\n\r\n>s1 desc\r\nACGT\r\nAC GT \r\n\r\n>s2\nTT\nGG')
    got = [(r.name, r.sequence, r.quality) for r in khmer.ReadParser(str(odd))]
    assert got == [('q1', 'GATTACA', '@@@IIII'), ('s1 desc', 'ACGTAC GT', None), ('s2', 'TTGG', None)]
    assert got == [(r.name, r.sequence, r.quality) for r in ok.ReadParser(str(odd))]
    tb = khmer.ReadParser(data_file('trio1/case1.fq.gz')).text_batch(5000, upload=False)
    assert tb.find_name('bogus-genome-chr1_115_449_0:0:0_0:0:0_1f4/1') == 1000
    assert tb.find_name('bogus-genome-chr1_115_449') == -1 and tb.record(1000).name.endswith('1f4/1')
    with pytest.raises(OSError):
        khmer.ReadParser(str(tmp_path / 'missing.fq'))
    bad = tmp_path / 'bad.fq'
    bad.write_text('ACGT\n')
    with pytest.raises(OSError):
        list(khmer.ReadParser(str(bad)))


# ---- kevlar dist host arithmetic (kevlar/tests/test_dist.py)
def test_dist_mu_sigma_and_table():
    import pytest
    from kevlar_amd.dist import calc_mu_sigma, compute_dist, KevlarZeroAbundanceDistError
    abund = {10: 6, 11: 10, 12: 12, 13: 18, 14: 16, 15: 11, 16: 9, 17: 9, 18: 11, 19: 8, 20: 9, 21: 7, 22: 3}
    mu, sigma = calc_mu_sigma(abund)
    assert mu == pytest.approx(15.32558, abs=1e-5) and sigma == pytest.approx(3.280581, abs=1e-6)
    with pytest.raises(KevlarZeroAbundanceDistError):
        calc_mu_sigma(dict())
    data = compute_dist(abund)
    assert list(data['Count'][:5]) == [6.0, 10.0, 12.0, 18.0, 16.0]
    assert list(data['CumulativeCount'][:5]) == [6.0, 16.0, 28.0, 46.0, 62.0]
    assert data['CumulativeFraction'].iloc[-1] == 1.0


# ---- kevlar split / augment (kevlar/tests/test_split.py, test_augment.py): host text plumbing
def test_split_round_robin_and_cli(tmp_path):
    from io import StringIO
    import kevlar_amd
    from conftest import data_file

    def partitions_of(path):
        stream = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(path, 'r'))
        return [part for _, part in kevlar_amd.parse_partitioned_reads(stream)]
    infile = data_file('fiveparts.augfastq.gz')
    partstream = kevlar_amd.parse_partitioned_reads(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(infile, 'r')))
    outstreams = [StringIO(), StringIO(), StringIO()]
    kevlar_amd.split.split(partstream, outstreams)
    for part, stream in ((1, 0), (2, 1), (3, 2), (4, 0), (5, 1)):
        assert 'kvcc={}'.format(part) in outstreams[stream].getvalue()
    args = kevlar_amd.cli.parser().parse_args(['split', infile, '3', str(tmp_path / 'out')])
    kevlar_amd.split.main(args)
    sizes = [[len(p) for p in partitions_of(str(tmp_path / 'out.{}.augfastx.gz'.format(i)))] for i in range(3)]
    assert sizes == [[67, 12], [23, 11], [15]]


def test_augment_contigs_reads_and_cli(capsys):
    import kevlar_amd
    from kevlar_amd.augment import augment
    from conftest import data_file

    def stream(name):
        return kevlar_amd.parse_augmented_fastx(kevlar_amd.open(data_file(name), 'r'))
    augseqs = list(augment(stream('snorkel.augfastq'), stream('snorkel-contig.fasta')))
    assert len(augseqs) == 1 and [k.offset for k in augseqs[0].annotations] == [17, 20, 22]
    contigs = list(augment(stream('deadbeef.augfastq.gz'), stream('deadbeef.contig.fa')))
    assert len(contigs) == 1 and len(contigs[0].annotations) == 74
    augreads = list(stream('deadbeef.augfastq.gz'))
    newreads = list(augment(augreads, stream('deadbeef.fq.gz'), upint=5))
    for oldread, newread in zip(augreads, newreads):
        assert oldread.sequence == newread.sequence and oldread.annotations == newread.annotations
    args = kevlar_amd.cli.parser().parse_args(['augment', data_file('reaugment.augfastq'), data_file('reaugment.fq')])
    kevlar_amd.augment.main(args)
    out, _ = capsys.readouterr()
    assert out == open(data_file('reaugment.out')).read()
    args = kevlar_amd.cli.parser().parse_args(['augment', data_file('snorkel.augfastq'), data_file('snorkel-contig.fasta')])
    kevlar_amd.augment.main(args)
    out, _ = capsys.readouterr()
    assert out.strip() == """>contig1
AGGTCTTCGATGCTAGCATTTTTACGACAGACAAAAACAAGATTACATTCCAAAATACATACCGCGCC
                 ATTTTTACGAC          8 0 0#
                    TTTACGACAGA          11 0 0#
                      TACGACAGACA          9 0 0#"""


def test_oracle_threaded_consume_equals_single_thread(ok):
    """bench.py's all-cores CPU baseline (khmer-style: threads share one sketch, atomic saturating adds,
    kevlar/count.py:41-76) must build the same tables as the scalar loop it is compared with"""
    import numpy as np
    rng = np.random.default_rng(3)
    letters = np.array(list('ACGT'))
    genome = ''.join(letters[rng.integers(0, 4, size=5000)])
    reads = [genome[s:s + 80] for s in rng.integers(0, 4920, size=3000)] + ['A' * 80] * 300 + ['ACG', '']
    bases, offs = ok.concat_reads(reads)
    for kind in ('Counttable', 'SmallCounttable', 'Nodetable'):
        one, many = getattr(ok, kind)(21, 3e4, 4), getattr(ok, kind)(21, 3e4, 4)
        n1 = ok.consume_reads(one, bases, offs, len(reads))
        n4 = ok.consume_reads_mt(many, bases, offs, len(reads), 4)
        assert n1 == n4 > 0
        for t in range(4):
            assert one.table_bytes(t) == many.table_bytes(t)
        assert one.n_occupied() == many.n_occupied()
    kid, mom = ok.Counttable(21, 3e4, 4), ok.Counttable(21, 3e4, 4)
    ok.consume_reads(kid, bases, offs, len(reads))
    hits, _ = ok.novel_scan([kid], [mom], bases, offs, len(reads), 21, 5, 0)
    assert ok.novel_scan_count_mt([kid], [mom], bases, offs, len(reads), 21, 5, 0, 3) == len(hits) > 0
    # the threaded scan that keeps its hits (whole-sample comparisons of tests/test_gpu_fullsize.py): the scalar loop's hits, in order,
    # also when a range of reads outgrows its share of the output buffers (cap 8)
    for cap in (1 << 16, 8):
        r, o, a = ok.novel_scan_mt([kid], [mom], bases, offs, len(reads), 21, 5, 0, 3, cap=cap)
        assert [(int(x), int(y), tuple(int(v) for v in z)) for x, y, z in zip(r, o, a)] == hits


def test_oracle_threaded_banded_consume_and_scan_equal_single_thread(ok):
    """the band legs of the cfg4-shaped GPU test: kvo_consume_reads_mt_banded against kvo_consume_reads with the same band, and the
    threaded scan against the scalar one under the hash-range band rule"""
    import numpy as np
    rng = np.random.default_rng(5)
    letters = np.array(list('ACGT'))
    genome = ''.join(letters[rng.integers(0, 4, size=8000)])
    child = genome[:4000] + ('A' if genome[4000] != 'A' else 'C') + genome[4001:]
    reads = {name: [g[s:s + 90] for s in rng.integers(0, 7910, size=3000)] for name, g in (('kid', child), ('mom', genome))}
    for nbands, band in ((2, 1), (8, 0), (8, 7)):
        one, many = {}, {}
        for name, seqs in reads.items():
            bases, offs = ok.concat_reads(seqs)
            one[name], many[name] = ok.Counttable(25, 2e4, 4), ok.Counttable(25, 2e4, 4)
            n1 = ok.consume_reads(one[name], bases, offs, len(seqs), nbands, band)
            n5 = ok.consume_reads_mt_banded(many[name], bases, offs, len(seqs), 5, nbands, band)
            assert n1 == n5 > 0
            for t in range(4):
                assert one[name].table_bytes(t) == many[name].table_bytes(t)
            assert one[name].n_occupied() == many[name].n_occupied()
        bases, offs = ok.concat_reads(reads['kid'])
        hits, _ = ok.novel_scan([one['kid']], [one['mom']], bases, offs, 3000, 25, 5, 1, band_mode=1, nbands=nbands, band=band)
        r, o, a = ok.novel_scan_mt([many['kid']], [many['mom']], bases, offs, 3000, 25, 5, 1, 4, band_mode=1, nbands=nbands, band=band)
        assert [(int(x), int(y), tuple(int(v) for v in z)) for x, y, z in zip(r, o, a)] == hits
    assert len(hits) > 0


def test_oracle_all_bands_in_one_pass_equal_the_band_by_band_legs(ok):
    """config 3's checker (tests/test_gpu_config3.py): kvo_consume_reads_mt_allbands / kvo_novel_scan_mt_allbands hash every k-mer once
    and send it to its band's sketches; per band they must give what the scalar banded count and scan (kvo_consume_reads with a
    band, kvo_novel_scan band_mode 1: kevlar/count.py:62-66 run once per band) give, and the union in (read, offset) order"""
    import numpy as np
    rng = np.random.default_rng(11)
    letters = np.array(list('ACGT'))
    genome = ''.join(letters[rng.integers(0, 4, size=9000)])
    child = genome[:3000] + ('A' if genome[3000] != 'A' else 'C') + genome[3001:6000] + ('G' if genome[6000] != 'G' else 'T') + genome[6001:]
    reads = {name: [g[s:s + 90] for s in rng.integers(0, 8910, size=3500)] for name, g in (('kid', child), ('mom', genome), ('dad', genome))}
    reads['kid'][17] = reads['kid'][17][:40] + 'N' + reads['kid'][17][41:]          # skipped by the scan, cleaned by the count
    for nbands in (1, 3, 8):
        scalar = {name: [ok.Counttable(25, 2e4, 4) for _ in range(nbands)] for name in reads}
        once = {name: [ok.Counttable(25, 2e4, 4) for _ in range(nbands)] for name in reads}
        for name, seqs in reads.items():
            bases, offs = ok.concat_reads(seqs)
            total = sum(ok.consume_reads(scalar[name][b], bases, offs, len(seqs), nbands, b) for b in range(nbands))
            assert ok.consume_reads_mt_allbands(once[name], bases, offs, len(seqs), 5) == total == len(seqs) * 66
            for b in range(nbands):
                for t in range(4):
                    assert scalar[name][b].table_bytes(t) == once[name][b].table_bytes(t)
                assert scalar[name][b].n_occupied() == once[name][b].n_occupied()
        bases, offs = ok.concat_reads(reads['kid'])
        r, o, a, hb = ok.novel_scan_mt_allbands([[once['kid'][b]] for b in range(nbands)], [[once['mom'][b], once['dad'][b]] for b in range(nbands)],
                                                bases, offs, 3500, 25, 5, 1, 4)
        merged = []
        for b in range(nbands):
            hits, _ = ok.novel_scan([scalar['kid'][b]], [scalar['mom'][b], scalar['dad'][b]], bases, offs, 3500, 25, 5, 1, band_mode=1,
                                    nbands=nbands, band=b)
            sel = hb == b
            assert [(int(x), int(y), tuple(int(v) for v in z)) for x, y, z in zip(r[sel], o[sel], a[sel])] == hits
            merged += hits
        assert [(int(x), int(y)) for x, y in zip(r, o)] == sorted((x, y) for x, y, _ in merged) and len(merged) > 0
        # (a buffer too small for a range's share of the hits: the call says how much room it wants)
        r2, o2, a2, hb2 = ok.novel_scan_mt_allbands([[once['kid'][b]] for b in range(nbands)], [[once['mom'][b], once['dad'][b]] for b in range(nbands)],
                                                    bases, offs, 3500, 25, 5, 1, 3, cap=8)
        assert np.array_equal(r, r2) and np.array_equal(o, o2) and np.array_equal(a, a2) and np.array_equal(hb, hb2)


def test_progress_indicator_jumps_match_item_by_item_counting(kevlar_log):
    """update(n) must log exactly where n single updates would (the reference ticks once per item,
    kevlar/progress.py:30-42: widen the interval at a break point, log when the count reaches the due point)"""
    import random
    import kevlar_amd

    def literal(interval, breaks, steps):
        out, counter, nxt = [], 0, interval
        for n in steps:
            for _ in range(n):
                if counter in breaks:
                    interval = counter
                if counter >= nxt:
                    nxt += interval
                    out.append(counter)
                counter += 1
        return out
    rng = random.Random(1)
    for trial in range(200):
        interval = rng.choice([1, 3, 10, 100])
        breaks = sorted(rng.sample(range(1, 5000), rng.randint(0, 4))) if trial % 2 else [100, 1000, 10000]
        steps = [rng.choice([1, 1, 7, 64, 999, 2500]) for _ in range(rng.randint(1, 30))]
        kevlar_log.seek(0); kevlar_log.truncate()
        p = kevlar_amd.ProgressIndicator('n={counter}', interval=interval, breaks=breaks)
        for n in steps:
            p.update(n)
        got = [int(line.rsplit('=', 1)[1]) for line in kevlar_log.getvalue().split('\n') if '=' in line]
        assert got == literal(interval, breaks, steps)


def test_progress_lines_match_the_reference_log(kevlar_log):
    """kevlar/tests/test_progress.py:18-28: 12000 single updates, interval 1, breaks 10/100/1000, against the
    reference's own expected log; and the same count in uneven batches"""
    import kevlar_amd
    want = open(data_file('progind.txt')).read().strip().split('\n')
    logger = kevlar_amd.ProgressIndicator('processed {counter} partitions', interval=1, breaks=[10, 100, 1000])
    for _ in range(12000):
        logger.update()
    assert kevlar_log.getvalue().strip().split('\n') == want
    kevlar_log.seek(0); kevlar_log.truncate()
    logger = kevlar_amd.ProgressIndicator('processed {counter} partitions', interval=1, breaks=[10, 100, 1000])
    for n in (5, 1, 94, 4000, 7000, 900):
        logger.update(n)
    assert kevlar_log.getvalue().strip().split('\n') == want


def test_timer_contract():
    """kevlar/tests/test_timer.py:16-38"""
    import time
    from kevlar_amd.timer import Timer
    t = Timer()
    t.start()
    t.start('task1')
    time.sleep(0.01)
    assert t.probe() > 0 and t.probe('task1') > 0.0
    with pytest.raises(ValueError, match=r'No timer started for "task2"'):
        t.probe('task2')
    assert t.stop('task1') > 0.0
    with pytest.raises(ValueError, match=r'No timer started for "task3"'):
        t.stop('task3')
    t.start('task3')
    with pytest.raises(ValueError, match=r'Timer already started for "task3"'):
        t.start('task3')


def test_hit_memory_keeps_its_owner_alive_through_derived_views():
    """arrays over a kv_hits handle's pinned memory (khmer._HitsMemory) must pin the handle for as long as ANY view of them
    lives -- np.asarray() and slices included; a dropped owner means recycled memory under a live array"""
    import ctypes
    import gc
    import numpy as np
    from kevlar_amd import khmer

    class Holder(object):
        alive = 0

        def __init__(self):
            Holder.alive += 1

        def __del__(self):
            Holder.alive -= 1
    block = (ctypes.c_uint32 * 16)(*range(16))
    holder = Holder()
    arr = np.asarray(khmer._HitsMemory(ctypes.addressof(block), (4, 4), np.uint32, holder))
    del holder
    assert arr.shape == (4, 4) and arr[2, 1] == 9
    plain, part, flat = np.asarray(arr), arr[1:3], arr.reshape(-1)[5:]
    del arr
    gc.collect()
    assert Holder.alive == 1
    del plain, part
    gc.collect()
    assert Holder.alive == 1 and flat[0] == 5
    del flat
    gc.collect()
    assert Holder.alive == 0


def test_bench_write_gzip_is_one_valid_member(tmp_path):
    """bench.write_gzip (the pigz-style writer of the end-to-end leg): pieces deflated on several threads make ONE gzip member
    that any reader inflates to the text, CRC-32 and length in the trailer included"""
    import gzip
    import struct
    import sys
    import zlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    try:
        import bench
    finally:
        sys.path.remove(root)
    rng = np.random.default_rng(3)
    text = bytes(rng.choice(np.frombuffer(b'ACGT\n', dtype=np.uint8), 700000)) + b'@tail\n'
    for piece, threads in ((1 << 16, 4), (1 << 20, 1), (123457, 3)):
        path = str(tmp_path / 'w{}.gz'.format(piece))
        bench.write_gzip(path, text, level=4, threads=threads, piece=piece)
        image = open(path, 'rb').read()
        assert gzip.decompress(image) == text
        assert zlib.decompressobj(31).decompress(image) == text                       # one member: nothing left over
        assert struct.unpack('<II', image[-8:]) == (zlib.crc32(text) & 0xffffffff, len(text))
    bench.write_gzip(str(tmp_path / 'empty.gz'), b'', threads=2)
    assert gzip.decompress(open(str(tmp_path / 'empty.gz'), 'rb').read()) == b''


def test_gentrio_cli_writes_a_consistent_trio(tmp_path):
    """kevlar/cli/gentrio.py:17-36, kevlar/gentrio.py:218-257: three two-haplotype FASTA files and a VCF whose genotypes
    explain every difference between a haplotype and the reference; de novo variants are the proband's alone"""
    import numpy as np
    import kevlar_amd
    rng = np.random.default_rng(5)
    genome = {'chr1': ''.join(rng.choice(list('ACGT'), size=20000)), 'chr2': ''.join(rng.choice(list('ACGT'), size=9000))}
    fasta = str(tmp_path / 'genome.fa')
    with open(fasta, 'w') as fh:
        for name, seq in genome.items():
            fh.write('>{} some description\n{}\n'.format(name, seq))
    prefix = str(tmp_path / 'fam')
    args = kevlar_amd.cli.parser().parse_args(['gentrio', '-i', '12', '-d', '5', '--seed', '42', '--prefix', prefix,
                                               '--vcf', str(tmp_path / 'fam.vcf'), fasta])
    kevlar_amd.gentrio.main(args)
    haps = {}
    for ind in ('proband', 'mother', 'father'):
        recs = list(kevlar_amd.parse_augmented_fastx(kevlar_amd.open('{}-{}.fasta'.format(prefix, ind), 'r')))
        assert [r.name for r in recs] == ['chr1_haplo1', 'chr1_haplo2', 'chr2_haplo1', 'chr2_haplo2']
        haps[ind] = {r.name: r.sequence for r in recs}
    rows = [line.rstrip('\n').split('\t') for line in open(str(tmp_path / 'fam.vcf')) if not line.startswith('#')]
    assert len(rows) == 17
    denovo = [r for r in rows if r[10] == '0/0' and r[11] == '0/0']
    assert len(denovo) >= 5 and all(r[9] in ('0/1', '1/0') for r in denovo)
    for col, ind in ((9, 'proband'), (10, 'mother'), (11, 'father')):
        for sid, seq in genome.items():
            for hap in (0, 1):
                carried = sorted((int(r[1]) - 1, r[3], r[4]) for r in rows if r[0] == sid and r[col][2 * hap] == '1')
                assert kevlar_amd.gentrio.haplotype(seq, carried) == haps[ind]['{}_haplo{}'.format(sid, hap + 1)]
    again = str(tmp_path / 'again')
    args = kevlar_amd.cli.parser().parse_args(['gentrio', '-i', '12', '-d', '5', '--seed', '42', '--prefix', again, fasta])
    kevlar_amd.gentrio.main(args)
    assert open(again + '-proband.fasta').read() == open(prefix + '-proband.fasta').read()
    assert kevlar_amd.gentrio.parse_weights('snv=2,del=2') == {'snv': 0.5, 'del': 0.5}


def test_assemble_partitions_matches_the_loop_it_replaced():
    """the array form of partition()'s ordering (largest first, ties by the larger smallest name, members by name, one read per
    sequence up to reverse complement, partitions that dedup leaves below min-abund dropped) against the plain restatement of
    kevlar/partition.py:15-55 + readgraph.py:123-161 -- random names (some shared: the last record of a name is its node's),
    lengths, strands and component labels"""
    import random
    import numpy as np
    import kevlar_amd
    from kevlar_amd.partition import assemble_partitions
    rng = random.Random(9)
    for trial in range(40):
        n = rng.choice([0, 1, 2, 7, 60, 400])
        lengths = [25] if trial % 3 == 0 else [20, 20, 33, 50, 1]           # every third trial: reads of one length (its own path)
        pool = [''.join(rng.choice('ACGTacgtN') for _ in range(rng.choice(lengths))) for _ in range(max(1, n // 3))]
        names, seqs = [], []
        for i in range(n):
            names.append('read{}'.format(rng.randrange(max(1, n))) if rng.random() < 0.15 else 'r{}/{}'.format(i, rng.randrange(3)))
            s = rng.choice(pool)
            seqs.append(kevlar_amd.revcom(s) if rng.random() < 0.4 else s)
        nb = ''.join(names).encode(); no = np.cumsum([0] + [len(x) for x in names]).astype(np.uint64)
        sb = ''.join(seqs).encode(); so = np.cumsum([0] + [len(x) for x in seqs]).astype(np.uint64)
        ncomp = max(1, n // rng.choice([2, 5, 20]))
        seen_nodes = {}

        def component_of(node_of_read, n_nodes):
            lab = np.array([rng.randrange(ncomp) for _ in range(n_nodes)], dtype=np.uint32)
            seen_nodes['node_of_read'], seen_nodes['labels'] = np.asarray(node_of_read), lab
            return lab
        for dedup, minabund in ((True, None), (True, 2), (False, None), (True, 3)):
            rng_state = rng.getstate()
            reads, number = assemble_partitions(nb, no, sb, so, component_of, minabund, dedup)
            rng.setstate(rng_state)
            if n == 0:
                assert len(reads) == 0
                continue
            # the loop: nodes by name, the record of a node is the last read with that name
            node_of_read, labels = seen_nodes['node_of_read'], seen_nodes['labels']
            holder = {}
            for i, name in enumerate(names):
                holder[name] = i
            label_of = {names[i]: int(labels[node_of_read[i]]) for i in range(n)}
            groups = {}
            for name, lab in label_of.items():
                groups.setdefault(lab, []).append(name)
            keyed = sorted(((len(m), sorted(m)) for m in groups.values() if len(m) >= 2), reverse=True)
            want_reads, want_number, num = [], [], 0
            for size, members in keyed:
                rs = [holder[name] for name in members]
                if dedup:
                    seen, kept = set(), []
                    for r in rs:
                        canon = kevlar_amd.revcommin(seqs[r])
                        if canon not in seen:
                            seen.add(canon)
                            kept.append(r)
                    rs = kept
                    if minabund and len(rs) < minabund:
                        continue
                num += 1
                want_reads += rs
                want_number += [num] * len(rs)
            assert reads.tolist() == want_reads and number.tolist() == want_number, (trial, dedup, minabund)


def test_dedup_survives_colliding_hashes(monkeypatch):
    """partition's dedup goes by two 64-bit hashes of the canonical sequence and then CONFIRMS every would-be duplicate against the
    sequence its run started with (kv_canonical_reads_equal: the reference compares the strings, kevlar/partition.py:26-33).  With
    the hashes forced to collide for every read, what is dropped must still be exactly the reads whose canonical sequence was seen
    before in their partition."""
    import random
    import numpy as np
    import kevlar_amd
    from kevlar_amd import partition as part_mod
    rng = random.Random(21)
    pool = [''.join(rng.choice('ACGTacgtN') for _ in range(rng.choice([1, 12, 30]))) for _ in range(25)]      # (revcom upper-cases: not an involution)
    seqs = [kevlar_amd.revcom(s) if rng.random() < 0.5 else s for s in (rng.choice(pool) for _ in range(300))]
    names = ['r{:04d}'.format(i) for i in range(300)]
    nb = ''.join(names).encode(); no = np.cumsum([0] + [len(x) for x in names]).astype(np.uint64)
    sb = ''.join(seqs).encode(); so = np.cumsum([0] + [len(x) for x in seqs]).astype(np.uint64)
    pairs = part_mod._same_canonical(sb, so, np.arange(299), np.arange(1, 300))
    assert pairs.tolist() == [kevlar_amd.revcommin(seqs[i]) == kevlar_amd.revcommin(seqs[i + 1]) for i in range(299)]
    labels = np.array([i % 7 for i in range(300)], dtype=np.uint32)
    want = part_mod.assemble_partitions(nb, no, sb, so, lambda node_of_read, n_nodes: labels, None, True)
    monkeypatch.setattr(part_mod, '_canonical_hashes', lambda s_, o_, reads: (np.zeros(len(reads), dtype=np.uint64), np.zeros(len(reads), dtype=np.uint64)))
    got = part_mod.assemble_partitions(nb, no, sb, so, lambda node_of_read, n_nodes: labels, None, True)
    # with one hash for everybody a run is a whole partition and only its FIRST sequence is confirmed against: copies of that one go,
    # every other read stays -- never a read whose sequence differs from the one it was compared with
    kept = set(got[0].tolist())
    for reads_, number in (got,):
        for p_ in set(number.tolist()):
            members = [r for r, q in zip(reads_.tolist(), number.tolist()) if q == p_]
            first_seq = kevlar_amd.revcommin(seqs[members[0]])
            assert sum(1 for r in members if kevlar_amd.revcommin(seqs[r]) == first_seq) == 1
    assert kept >= set(want[0].tolist())              # nothing the true dedup keeps was dropped


def test_dedup_runs_take_the_exact_order_when_two_groups_share_a_mixed_key():
    """partition's dedup sorts its members ONCE, by a 64-bit mix of partition number and first hash; two different (partition, h1)
    pairs with the same mix would interleave in that order and a duplicate would be missed -- so the runs of equal keys are put into
    the exact (partition, h1, h2, member) order themselves.  Crafted: partition 0 with h1 = X and partition 1 with h1 = X ^ MIX share a key."""
    import numpy as np
    from kevlar_amd.partition import _dedup_runs, _MIX
    X = 0x1234567890abcdef
    part = np.array([0, 1, 0, 1, 0, 2], dtype=np.int64)
    h1 = np.array([X, X ^ _MIX, X, X ^ _MIX, X, 7], dtype=np.uint64)
    h2 = np.array([5, 5, 5, 5, 6, 5], dtype=np.uint64)
    dup, head = _dedup_runs(part, h1, h2)
    assert sorted(zip(dup.tolist(), head.tolist())) == [(2, 0), (3, 1)]      # members 2 and 3 repeat members 0 and 1; member 4 differs in h2
    rng = np.random.default_rng(2)
    part = np.sort(rng.integers(0, 50, size=5000)).astype(np.int64)
    h1 = rng.integers(0, 40, size=5000).astype(np.uint64)
    h2 = rng.integers(0, 3, size=5000).astype(np.uint64)
    dup, head = _dedup_runs(part, h1, h2)
    seen, want = {}, []
    for i, key in enumerate(zip(part.tolist(), h1.tolist(), h2.tolist())):
        if key in seen:
            want.append((i, seen[key]))
        else:
            seen[key] = i
    assert sorted(zip(dup.tolist(), head.tolist())) == want


def test_the_build_knows_every_source_and_header():
    """__graft_entry__.build() recompiles when a listed source or header is newer than the library: a file that is not on the lists
    would change without a rebuild (kv_inflate_device.h was missing until round 4), and a stale library on the GPU box fails every
    test that loads it"""
    import __graft_entry__ as g
    csrc = g.CSRC
    assert sorted(g.HIP_SOURCES) == sorted(f for f in os.listdir(csrc) if f.endswith('.hip'))
    assert sorted(os.path.basename(h) for h in g.HIP_HEADERS if not h.startswith('..')) == sorted(f for f in os.listdir(csrc) if f.endswith('.h'))
    assert any(h.endswith('kvsketch.h') for h in g.HIP_HEADERS)


def test_fixed_width_rows_are_the_strings_nul_padded():
    """partition's name matrix: one NUL-padded row per string, whatever the lengths (ragged: rows gathered from a sliding window;
    one length back to back: the blob reshaped; offsets that start behind the blob's first byte; empty strings; no strings)"""
    import random
    import numpy as np
    from kevlar_amd.partition import _fixed_width
    rng = random.Random(4)
    for trial in range(200):
        n = rng.choice([0, 1, 2, 9, 50])
        same = trial % 3 == 0
        length = rng.randrange(0, 7)
        strings = [bytes(rng.randrange(1, 256) for _ in range(length if same else rng.randrange(0, 9))) for _ in range(n)]
        lead = bytes(rng.randrange(1, 256) for _ in range(rng.randrange(0, 3))) if trial % 4 == 0 else b''
        tail = bytes(rng.randrange(1, 256) for _ in range(rng.randrange(0, 3)))
        blob = lead + b''.join(strings) + tail
        offs = np.cumsum([len(lead)] + [len(s) for s in strings]).astype(np.uint64)
        rows = _fixed_width(blob, offs)
        assert len(rows) == n
        width = max([len(s) for s in strings] + [1])
        if n and blob:
            assert rows.dtype == np.dtype('S{}'.format(width))
        assert [bytes(r) for r in rows.tolist()] == [s for s in strings]        # (numpy strips the padding again)
        assert sorted(range(n), key=lambda i: strings[i]) == np.argsort(rows, kind='stable').tolist() if n else True


def test_canonical_read_hashes_group_reads_like_revcommin():
    """partition's dedup key: reads get the same pair of hashes exactly when kevlar.revcommin() gives the same string -- IUPAC codes,
    both cases, lengths from 0 up, reads addressed in any order, one thread or several"""
    import random
    import numpy as np
    import kevlar_amd
    from kevlar_amd.partition import _canonical_hashes
    rng = random.Random(12)
    for trial, threads in enumerate((None, '1', '3')):
        n = 30000 if threads == '3' else 1500                # (the helper starts a thread per 20 000 reads)
        seqs = [''.join(rng.choice('ACGTNacgtRYKMBDHVu') for _ in range(rng.choice([0, 1, 2, 7, 8, 9, 31, 100]))) for _ in range(n // 3)]
        seqs += [rng.choice(seqs) if rng.random() < 0.5 else kevlar_amd.revcom(rng.choice(seqs)) for _ in range(n - len(seqs))]
        blob = ''.join(seqs).encode('latin-1')
        offs = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        order = list(range(n)); rng.shuffle(order)
        if threads:
            os.environ['KV_AUGFASTX_THREADS'] = threads
        try:
            h1, h2 = _canonical_hashes(blob, offs, order)
        finally:
            os.environ.pop('KV_AUGFASTX_THREADS', None)
        by_key = {}
        for at, i in enumerate(order):
            by_key.setdefault(kevlar_amd.revcommin(seqs[i]), set()).add((int(h1[at]), int(h2[at])))
        assert all(len(v) == 1 for v in by_key.values())
        assert len({next(iter(v)) for v in by_key.values()}) == len(by_key)
    assert len(_canonical_hashes(b'', np.zeros(1, dtype=np.uint64), [])[0]) == 0


def test_odd_reads_are_the_reads_with_bytes_outside_acgt():
    """AnnotatedReads.odd_reads(): the reads the 2-bit form cannot hold -- anything but upper-case A, C, G, T -- found by the library's
    host helper (threads over the reads when there are many), empty reads never among them"""
    import random
    from kevlar_amd.annotated import AnnotatedReads
    from kevlar_amd.sequence import Record
    rng = random.Random(21)
    for n in (0, 1, 7, 400, 45000):
        seqs = [''.join(rng.choice('ACGT' * 40 + 'Nacgt-*') for _ in range(rng.choice([0, 1, 25, 60]))) for _ in range(n)]
        reads = AnnotatedReads([Record(name='r{}'.format(i), sequence=s) for i, s in enumerate(seqs)])
        want = [i for i, s in enumerate(seqs) if any(c not in 'ACGT' for c in s)]
        assert reads.odd_reads().tolist() == want
        assert not reads.seqs or reads.odd_reads() is reads.odd_reads()             # (kept: filter and partition ask more than once)


def test_console_script_is_the_reference_s():
    """reference setup.py:69-71: console_scripts kevlar = kevlar.__main__:main -- here pyproject.toml's kevlar = kevlar_amd.__main__:main,
    and that callable is the dispatcher `python -m kevlar_amd` runs; the product's build does not touch the oracle"""
    import importlib
    import inspect
    text = open(os.path.join(ROOT, 'pyproject.toml')).read()
    assert 'kevlar = "kevlar_amd.__main__:main"' in text
    mod = importlib.import_module('kevlar_amd.__main__')
    assert callable(mod.main)
    import __graft_entry__
    body = inspect.getsource(__graft_entry__.build_product).split('"""')[2]          # (the code, not the docstring that says so)
    assert 'oracle' not in body and 'okhmer' not in body
    assert 'build_product()' in open(os.path.join(ROOT, 'bench.py')).read()


def test_exchange_plans_are_host_arithmetic_every_rank_repeats():
    """kv_mex_plan_make / kv_mex_plan_short need no device: the plan of a sample's minimizer-sharded exchange depends on the sample's global
    size only, so every rank derives the same one.  Its split points cover the coarse buckets evenly; the short form (16-byte records
    without read positions) exists for k = 31 and reads the lane-per-read cut takes, keeps the segment geometry and shrinks the words;
    config 4's size ends at the geometry's limit (248 x 4096 buckets) and still has a short form."""
    import ctypes
    from kevlar_amd import _lib
    lib = _lib.load()

    def plan(k, n_reads, read_len, ndest, short=False):
        p = _lib.MexPlan()
        assert lib.kv_mex_plan_make(0, k, n_reads, read_len, ndest, ctypes.byref(p)) == 0, _lib.last_error()
        rc = lib.kv_mex_plan_short(ctypes.byref(p)) if short else 0
        return p, rc
    for ndest in (1, 2, 3, 8):
        p, _ = plan(31, 7_500_000, 100, ndest)
        lo = [int(p.c_lo[d]) for d in range(ndest + 1)]
        assert lo[0] == 0 and lo[-1] == int(p.C1) and all(b > a for a, b in zip(lo, lo[1:]))
        assert int(p.seg_words) == int(p.C1) * int(p.nwg1) * int(p.cap1) * int(p.recw) and int(p.cnt_entries) == int(p.C1) * int(p.nwg1)
        assert int(p.recw) == 3 and int(p.flags) == 0
        q, rc = plan(31, 7_500_000, 100, ndest, short=True)
        assert rc == 0 and int(q.flags) & 1 and int(q.recw) == 2 and int(q.seg_words) * 3 == int(p.seg_words) * 2
        assert (int(q.C1), int(q.F2), int(q.nwg1), int(q.cap1)) == (int(p.C1), int(p.F2), int(p.nwg1), int(p.cap1))
    assert plan(31, 7_500_000, 150, 8, short=True)[1] == 0              # two workgroups of the cut per CU up to 224 bases
    for k, read_len in ((31, 250), (51, 150), (25, 100)):                # reads the cut does not take, two-word keys, another window
        p, rc = plan(k, 7_500_000, read_len, 8, short=True)
        assert rc == _lib.KV_ERR_NOTIMPL and int(p.flags) == 0 and int(p.recw) == (4 if k > 32 else 3)
    big, rc = plan(31, 900_000_000, 100, 8, short=True)
    assert rc == 0 and (int(big.C1), int(big.F2), int(big.recw)) == (248, 4096, 2)
    p = _lib.MexPlan()
    assert lib.kv_mex_plan_make(0, 12, 1000, 100, 8, ctypes.byref(p)) != 0          # k below the super-k-mer front end's range


def test_every_environment_switch_is_in_the_one_registry_of_two_classes(monkeypatch):
    """kevlar_amd/csrc/kv_knobs.h: the library and its wrapper look at the environment through ONE table (kv_host.hip).  No source
    calls getenv() beside the registry; every name a source asks for is registered with a class and a description; a TUNING switch is
    ignored unless KV_TUNING=1 -- a stray KV_* in a user's shell changes nothing -- and the phase-skip switches of old timing
    experiments (wrong results) are gone: not registered, not listed, not asked for."""
    import glob
    from kevlar_amd import _lib
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    assert _lib.load().kv_knobs_describe(1, buf, len(buf)) == 0
    table = {}
    for line in buf.value.decode().splitlines():
        name, cls, doc = line.split('\t')
        assert name not in table and cls in ('setting', 'tuning') and len(doc) > 10, line
        table[name] = cls
    asked = set()
    csrc = os.path.join(ROOT, 'kevlar_amd', 'csrc')
    for path in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h')):
        text = open(path).read()
        raw = [m.start() for m in re.finditer(r'\bgetenv\s*\(', text)]
        if os.path.basename(path) == 'kv_host.hip':
            # the registry's own three: the KV_TUNING switch, the lookup, the listing
            assert len(raw) == 3 and all(text.index('// ---- the knob registry') < at for at in raw), path
        elif os.path.basename(path) != 'kv_knobs.h':
            assert not raw, '{} calls getenv() beside the registry'.format(path)
        asked |= set(re.findall(r'kv_knob\(\s*"([A-Z_0-9]+)"', text))
        asked |= set(re.findall(r'kv_knob\([^")]*\?\s*"([A-Z_0-9]+)"\s*:\s*"([A-Z_0-9]+)"', text)[0]) if 'kv_knob(for_scan' in text else set()
    for path in glob.glob(os.path.join(ROOT, 'kevlar_amd', '*.py')) + glob.glob(os.path.join(ROOT, 'kevlar_amd', 'cli', '*.py')):
        text = open(path).read()
        asked |= set(re.findall(r"_lib\.knob\(\s*'([A-Z_0-9]+)'", text))
        # the wrapper's only direct looks at the environment: where the library is, which GPU this rank takes
        for name in re.findall(r"environ(?:\.get\(|\[)\s*'([A-Z_0-9]+)'", text):
            assert name in ('KV_LIB_PATH', 'LOCAL_RANK'), '{} reads {} beside the registry'.format(path, name)
    assert asked and asked <= set(table), sorted(asked - set(table))
    assert set(table) - asked <= set(), 'registered but never asked for: {}'.format(sorted(set(table) - asked))
    # a tuning switch exists only while something holds its branch to the oracle: a test other than this file, or a fuzzer
    users = [p for p in glob.glob(os.path.join(ROOT, 'tests', '**', '*.py'), recursive=True) if os.path.basename(p) != 'test_host_logic.py']
    users += glob.glob(os.path.join(ROOT, 'scratch', 'fuzz_*.py'))
    used = set()
    for path in users:
        used |= set(re.findall(r'\bKV_[A-Z_0-9]+\b', open(path).read()))
    unset = sorted(name for name, cls in table.items() if cls == 'tuning' and name not in used)
    assert not unset, 'tuning switches that no test and no fuzzer sets: {}'.format(unset)

    for name in list(os.environ):
        if name.startswith('KV_'):
            monkeypatch.delenv(name)
    assert _lib.knobs_active() == ''
    monkeypatch.setenv('KV_COUNT_PATH', 'atomic')
    monkeypatch.setenv('KV_TABLE_CACHE_GB', '1')
    monkeypatch.setenv('KV_SKM_DEBUG', '3')
    assert _lib.knob('KV_COUNT_PATH') is None and _lib.knob('KV_TABLE_CACHE_GB') == '1'
    assert sorted(_lib.knobs_active().split()) == ['KV_TABLE_CACHE_GB=1', 'ignored:KV_COUNT_PATH=atomic']
    with pytest.raises(ValueError):
        _lib.knob('KV_SKM_DEBUG')
    monkeypatch.setenv('KV_TUNING', '1')
    assert _lib.knob('KV_COUNT_PATH') == 'atomic'
    assert sorted(_lib.knobs_active().split()) == ['KV_COUNT_PATH=atomic', 'KV_TABLE_CACHE_GB=1']
    with pytest.raises(ValueError):
        _lib.knob('KV_SKM_DEBUG')
    with pytest.raises(ValueError):
        _lib.knob('KV_NO_SUCH_SWITCH')
    # no compile-time switch of the kernels changes results or picks a variant either
    for path in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h')):
        text = open(path).read()
        for word in ('SKM_HACK', 'SKM_LANE_DISSECT', 'KV_EXPERIMENTS', 'SKM_DBG', 'SKM_LINEAR_PROBE', 'SKM_LANE_FULL', 'SKM_LANE_BRANCHFREE',
                     'KV_FASTMOD_NO_FP'):
            assert word not in text, (path, word)


def test_bench_clock_watch_never_raises_and_reports_nothing_without_a_card():
    """bench.py samples the shader clock and power of the card it computes on (its hwmon files, found by PCI address) beside the timed
    steps; on a host without a GPU -- or where the files are not readable -- the field is null, never an error"""
    import sys
    import time
    sys.path.insert(0, ROOT)
    import bench
    watch = bench.ClockWatch(0, period=0.005)
    time.sleep(0.03)
    got = watch.stop()
    assert got is None or (set(got) >= {'sclk_mhz', 'power_w', 'samples'} and got['samples'] > 0)
