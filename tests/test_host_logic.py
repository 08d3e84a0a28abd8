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


# kv_mex_plan_make over k x reads x read length x destinations, as the library answered before its bucket planner was written once:
# ((k, reads, read length, ndest), (C1, F2, fbits, nwg1, cap1, recw, m, seg_words, cnt_entries, c_lo[0..ndest], flags),
#  what kv_mex_plan_short returns for it, (recw, seg_words, flags) after that call)
_MEX_PLANS = (
    ((16,1,16,1),(1,1,0,1,2384,3,8,7152,1,(0,1),0),-5,(3,7152,0)),
    ((16,1,16,2),(2,1,0,1,1280,3,8,7680,2,(0,1,2),0),-5,(3,7680,0)),
    ((16,1,16,3),(3,1,0,1,896,3,8,8064,3,(0,1,2,3),0),-5,(3,8064,0)),
    ((16,1,16,8),(8,1,0,1,416,3,8,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((16,1,100,1),(1,1,0,1,2416,3,8,7248,1,(0,1),0),-5,(3,7248,0)),
    ((16,1,100,2),(2,1,0,1,1296,3,8,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((16,1,100,3),(3,1,0,1,912,3,8,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((16,1,100,8),(8,1,0,1,416,3,8,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((16,1,150,1),(1,1,0,1,2448,3,8,7344,1,(0,1),0),-5,(3,7344,0)),
    ((16,1,150,2),(2,1,0,1,1312,3,8,7872,2,(0,1,2),0),-5,(3,7872,0)),
    ((16,1,150,3),(3,1,0,1,928,3,8,8352,3,(0,1,2,3),0),-5,(3,8352,0)),
    ((16,1,150,8),(8,1,0,1,432,3,8,10368,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,10368,0)),
    ((16,1,251,1),(1,1,0,1,2480,3,8,7440,1,(0,1),0),-5,(3,7440,0)),
    ((16,1,251,2),(2,1,0,1,1328,3,8,7968,2,(0,1,2),0),-5,(3,7968,0)),
    ((16,1,251,3),(3,1,0,1,944,3,8,8496,3,(0,1,2,3),0),-5,(3,8496,0)),
    ((16,1,251,8),(8,1,0,1,432,3,8,10368,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,10368,0)),
    ((16,1000,16,1),(1,1,0,2,2576,3,8,15456,2,(0,1),0),-5,(3,15456,0)),
    ((16,1000,16,2),(2,1,0,1,1936,3,8,11616,2,(0,1,2),0),-5,(3,11616,0)),
    ((16,1000,16,3),(3,1,0,1,1200,3,8,10800,3,(0,1,2,3),0),-5,(3,10800,0)),
    ((16,1000,16,8),(8,1,0,1,464,3,8,11136,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,11136,0)),
    ((16,1000,100,1),(3,4,2,2,7456,3,8,134208,6,(0,3),0),-5,(3,134208,0)),
    ((16,1000,100,2),(4,4,2,1,5920,3,8,71040,4,(0,2,4),0),-5,(3,71040,0)),
    ((16,1000,100,3),(3,4,2,1,5536,3,8,49824,3,(0,1,2,3),0),-5,(3,49824,0)),
    ((16,1000,100,8),(8,4,2,1,1104,3,8,26496,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,26496,0)),
    ((16,1000,150,1),(3,8,3,2,11232,3,8,202176,6,(0,3),0),-5,(3,202176,0)),
    ((16,1000,150,2),(4,8,3,1,8768,3,8,105216,4,(0,2,4),0),-5,(3,105216,0)),
    ((16,1000,150,3),(3,8,3,1,8080,3,8,72720,3,(0,1,2,3),0),-5,(3,72720,0)),
    ((16,1000,150,8),(8,8,3,1,1488,3,8,35712,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,35712,0)),
    ((16,1000,251,1),(4,8,3,2,14208,3,8,340992,8,(0,4),0),-5,(3,340992,0)),
    ((16,1000,251,2),(4,8,3,1,14480,3,8,173760,4,(0,2,4),0),-5,(3,173760,0)),
    ((16,1000,251,3),(6,8,3,1,6752,3,8,121536,6,(0,2,4,6),0),-5,(3,121536,0)),
    ((16,1000,251,8),(8,8,3,1,2224,3,8,53376,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,53376,0)),
    ((16,2000000,16,1),(16,16,4,256,1456,3,8,17891328,4096,(0,16),0),-5,(3,17891328,0)),
    ((16,2000000,16,2),(16,16,4,256,800,3,8,9830400,4096,(0,8,16),0),-5,(3,9830400,0)),
    ((16,2000000,16,3),(18,16,4,256,528,3,8,7299072,4608,(0,6,12,18),0),-5,(3,7299072,0)),
    ((16,2000000,16,8),(16,16,4,256,288,3,8,3538944,4096,(0,2,4,6,8,10,12,14,16),0),-5,(3,3538944,0)),
    ((16,2000000,100,1),(82,256,8,256,4176,3,8,262987776,20992,(0,82),0),-5,(3,262987776,0)),
    ((16,2000000,100,2),(82,256,8,256,2192,3,8,138043392,20992,(0,41,82),0),-5,(3,138043392,0)),
    ((16,2000000,100,3),(84,256,8,256,1488,3,8,95993856,21504,(0,28,56,84),0),-5,(3,95993856,0)),
    ((16,2000000,100,8),(88,256,8,256,624,3,8,42172416,22528,(0,11,22,33,44,55,66,77,88),0),-5,(3,42172416,0)),
    ((16,2000000,150,1),(129,256,8,256,4128,3,8,408969216,33024,(0,129),0),-5,(3,408969216,0)),
    ((16,2000000,150,2),(130,256,8,256,2160,3,8,215654400,33280,(0,65,130),0),-5,(3,215654400,0)),
    ((16,2000000,150,3),(129,256,8,256,1504,3,8,149004288,33024,(0,43,86,129),0),-5,(3,149004288,0)),
    ((16,2000000,150,8),(136,256,8,256,624,3,8,65175552,34816,(0,17,34,51,68,85,102,119,136),0),-5,(3,65175552,0)),
    ((16,2000000,251,1),(226,256,8,256,4064,3,8,705380352,57856,(0,226),0),-5,(3,705380352,0)),
    ((16,2000000,251,2),(226,256,8,256,2144,3,8,372129792,57856,(0,113,226),0),-5,(3,372129792,0)),
    ((16,2000000,251,3),(228,256,8,256,1472,3,8,257753088,58368,(0,76,152,228),0),-5,(3,257753088,0)),
    ((16,2000000,251,8),(232,256,8,256,640,3,8,114032640,59392,(0,29,58,87,116,145,174,203,232),0),-5,(3,114032640,0)),
    ((16,7500000,16,1),(29,32,5,256,2816,3,8,62717952,7424,(0,29),0),-5,(3,62717952,0)),
    ((16,7500000,16,2),(30,32,5,256,1456,3,8,33546240,7680,(0,15,30),0),-5,(3,33546240,0)),
    ((16,7500000,16,3),(30,32,5,256,1024,3,8,23592960,7680,(0,10,20,30),0),-5,(3,23592960,0)),
    ((16,7500000,16,8),(32,32,5,256,448,3,8,11010048,8192,(0,4,8,12,16,20,24,28,32),0),-5,(3,11010048,0)),
    ((16,7500000,100,1),(152,512,9,256,8160,3,8,952565760,38912,(0,152),0),-5,(3,952565760,0)),
    ((16,7500000,100,2),(152,512,9,256,4224,3,8,493092864,38912,(0,76,152),0),-5,(3,493092864,0)),
    ((16,7500000,100,3),(153,512,9,256,2864,3,8,336531456,39168,(0,51,102,153),0),-5,(3,336531456,0)),
    ((16,7500000,100,8),(152,512,9,256,1200,3,8,140083200,38912,(0,19,38,57,76,95,114,133,152),0),-5,(3,140083200,0)),
    ((16,7500000,150,1),(242,512,9,256,7984,3,8,1483874304,61952,(0,242),0),-5,(3,1483874304,0)),
    ((16,7500000,150,2),(242,512,9,256,4128,3,8,767213568,61952,(0,121,242),0),-5,(3,767213568,0)),
    ((16,7500000,150,3),(243,512,9,256,2816,3,8,525533184,62208,(0,81,162,243),0),-5,(3,525533184,0)),
    ((16,7500000,150,8),(248,512,9,256,1152,3,8,219414528,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,219414528,0)),
    ((16,7500000,251,1),(212,1024,10,256,15376,3,8,2503458816,54272,(0,212),0),-5,(3,2503458816,0)),
    ((16,7500000,251,2),(212,1024,10,256,7872,3,8,1281687552,54272,(0,106,212),0),-5,(3,1281687552,0)),
    ((16,7500000,251,3),(213,1024,10,256,5312,3,8,868958208,54528,(0,71,142,213),0),-5,(3,868958208,0)),
    ((16,7500000,251,8),(216,1024,10,256,2112,3,8,350355456,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,350355456,0)),
    ((16,900000000,16,1),(215,512,9,256,41104,3,8,6787092480,55040,(0,215),0),-5,(3,6787092480,0)),
    ((16,900000000,16,2),(216,512,9,256,20720,3,8,3437199360,55296,(0,108,216),0),-5,(3,3437199360,0)),
    ((16,900000000,16,3),(216,512,9,256,13952,3,8,2314469376,55296,(0,72,144,216),0),-5,(3,2314469376,0)),
    ((16,900000000,16,8),(216,512,9,256,5440,3,8,902430720,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,902430720,0)),
    ((16,900000000,100,1),(255,4096,12,256,547440,3,8,107210649600,65280,(0,255),0),-5,(3,107210649600,0)),
    ((16,900000000,100,2),(254,4096,12,256,275696,3,8,53780570112,65024,(0,127,254),0),-5,(3,53780570112,0)),
    ((16,900000000,100,3),(255,4096,12,256,183552,3,8,35946823680,65280,(0,85,170,255),0),-5,(3,35946823680,0)),
    ((16,900000000,100,8),(248,4096,12,256,71376,3,8,13594558464,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,13594558464,0)),
    ((16,900000000,150,1),(255,4096,12,256,851776,3,8,166811811840,65280,(0,255),0),-5,(3,166811811840,0)),
    ((16,900000000,150,2),(254,4096,12,256,428672,3,8,83621904384,65024,(0,127,254),0),-5,(3,83621904384,0)),
    ((16,900000000,150,3),(255,4096,12,256,285248,3,8,55862968320,65280,(0,85,170,255),0),-5,(3,55862968320,0)),
    ((16,900000000,150,8),(248,4096,12,256,110736,3,8,21091221504,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,21091221504,0)),
    ((16,900000000,251,1),(255,4096,12,256,1466096,3,8,287120240640,65280,(0,255),0),-5,(3,287120240640,0)),
    ((16,900000000,251,2),(254,4096,12,256,737376,3,8,143841411072,65024,(0,127,254),0),-5,(3,143841411072,0)),
    ((16,900000000,251,3),(255,4096,12,256,490416,3,8,96043069440,65280,(0,85,170,255),0),-5,(3,96043069440,0)),
    ((16,900000000,251,8),(248,4096,12,256,190064,3,8,36200349696,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,36200349696,0)),
    ((25,1,25,1),(1,1,0,1,2384,3,12,7152,1,(0,1),0),-5,(3,7152,0)),
    ((25,1,25,2),(2,1,0,1,1280,3,12,7680,2,(0,1,2),0),-5,(3,7680,0)),
    ((25,1,25,3),(3,1,0,1,896,3,12,8064,3,(0,1,2,3),0),-5,(3,8064,0)),
    ((25,1,25,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((25,1,100,1),(1,1,0,1,2400,3,12,7200,1,(0,1),0),-5,(3,7200,0)),
    ((25,1,100,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((25,1,100,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((25,1,100,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((25,1,150,1),(1,1,0,1,2416,3,12,7248,1,(0,1),0),-5,(3,7248,0)),
    ((25,1,150,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((25,1,150,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((25,1,150,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((25,1,251,1),(1,1,0,1,2448,3,12,7344,1,(0,1),0),-5,(3,7344,0)),
    ((25,1,251,2),(2,1,0,1,1312,3,12,7872,2,(0,1,2),0),-5,(3,7872,0)),
    ((25,1,251,3),(3,1,0,1,928,3,12,8352,3,(0,1,2,3),0),-5,(3,8352,0)),
    ((25,1,251,8),(8,1,0,1,432,3,12,10368,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,10368,0)),
    ((25,1000,25,1),(1,1,0,2,2512,3,12,15072,2,(0,1),0),-5,(3,15072,0)),
    ((25,1000,25,2),(2,1,0,1,1888,3,12,11328,2,(0,1,2),0),-5,(3,11328,0)),
    ((25,1000,25,3),(3,1,0,1,1184,3,12,10656,3,(0,1,2,3),0),-5,(3,10656,0)),
    ((25,1000,25,8),(8,1,0,1,464,3,12,11136,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,11136,0)),
    ((25,1000,100,1),(3,4,2,2,4832,3,12,86976,6,(0,3),0),-5,(3,86976,0)),
    ((25,1000,100,2),(4,4,2,1,3952,3,12,47424,4,(0,2,4),0),-5,(3,47424,0)),
    ((25,1000,100,3),(3,4,2,1,3792,3,12,34128,3,(0,1,2,3),0),-5,(3,34128,0)),
    ((25,1000,100,8),(8,4,2,1,848,3,12,20352,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,20352,0)),
    ((25,1000,150,1),(4,4,2,2,5600,3,12,134400,8,(0,4),0),-5,(3,134400,0)),
    ((25,1000,150,2),(4,4,2,1,5872,3,12,70464,4,(0,2,4),0),-5,(3,70464,0)),
    ((25,1000,150,3),(6,4,2,1,2864,3,12,51552,6,(0,2,4,6),0),-5,(3,51552,0)),
    ((25,1000,150,8),(8,4,2,1,1104,3,12,26496,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,26496,0)),
    ((25,1000,251,1),(4,8,3,2,9424,3,12,226176,8,(0,4),0),-5,(3,226176,0)),
    ((25,1000,251,2),(4,8,3,1,9696,3,12,116352,4,(0,2,4),0),-5,(3,116352,0)),
    ((25,1000,251,3),(6,8,3,1,4592,3,12,82656,6,(0,2,4,6),0),-5,(3,82656,0)),
    ((25,1000,251,8),(8,8,3,1,1600,3,12,38400,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,38400,0)),
    ((25,2000000,25,1),(16,16,4,256,1376,3,12,16908288,4096,(0,16),0),-5,(3,16908288,0)),
    ((25,2000000,25,2),(16,16,4,256,768,3,12,9437184,4096,(0,8,16),0),-5,(3,9437184,0)),
    ((25,2000000,25,3),(18,16,4,256,512,3,12,7077888,4608,(0,6,12,18),0),-5,(3,7077888,0)),
    ((25,2000000,25,8),(16,16,4,256,272,3,12,3342336,4096,(0,2,4,6,8,10,12,14,16),0),-5,(3,3342336,0)),
    ((25,2000000,100,1),(73,256,8,256,2960,3,12,165949440,18688,(0,73),0),-5,(3,165949440,0)),
    ((25,2000000,100,2),(74,256,8,256,1552,3,12,88203264,18944,(0,37,74),0),-5,(3,88203264,0)),
    ((25,2000000,100,3),(75,256,8,256,1072,3,12,61747200,19200,(0,25,50,75),0),-5,(3,61747200,0)),
    ((25,2000000,100,8),(80,256,8,256,464,3,12,28508160,20480,(0,10,20,30,40,50,60,70,80),0),-5,(3,28508160,0)),
    ((25,2000000,150,1),(121,256,8,256,2864,3,12,266145792,30976,(0,121),0),-5,(3,266145792,0)),
    ((25,2000000,150,2),(122,256,8,256,1520,3,12,142417920,31232,(0,61,122),0),-5,(3,142417920,0)),
    ((25,2000000,150,3),(123,256,8,256,1056,3,12,99753984,31488,(0,41,82,123),0),-5,(3,99753984,0)),
    ((25,2000000,150,8),(128,256,8,256,464,3,12,45613056,32768,(0,16,32,48,64,80,96,112,128),0),-5,(3,45613056,0)),
    ((25,2000000,251,1),(217,256,8,256,2816,3,12,469303296,55552,(0,217),0),-5,(3,469303296,0)),
    ((25,2000000,251,2),(218,256,8,256,1504,3,12,251805696,55808,(0,109,218),0),-5,(3,251805696,0)),
    ((25,2000000,251,3),(219,256,8,256,1056,3,12,177610752,56064,(0,73,146,219),0),-5,(3,177610752,0)),
    ((25,2000000,251,8),(224,256,8,256,464,3,12,79822848,57344,(0,28,56,84,112,140,168,196,224),0),-5,(3,79822848,0)),
    ((25,7500000,25,1),(29,32,5,256,2656,3,12,59154432,7424,(0,29),0),-5,(3,59154432,0)),
    ((25,7500000,25,2),(30,32,5,256,1376,3,12,31703040,7680,(0,15,30),0),-5,(3,31703040,0)),
    ((25,7500000,25,3),(30,32,5,256,976,3,12,22487040,7680,(0,10,20,30),0),-5,(3,22487040,0)),
    ((25,7500000,25,8),(32,32,5,256,432,3,12,10616832,8192,(0,4,8,12,16,20,24,28,32),0),-5,(3,10616832,0)),
    ((25,7500000,100,1),(136,512,9,256,5712,3,12,596606976,34816,(0,136),0),-5,(3,596606976,0)),
    ((25,7500000,100,2),(136,512,9,256,2976,3,12,310837248,34816,(0,68,136),0),-5,(3,310837248,0)),
    ((25,7500000,100,3),(138,512,9,256,2032,3,12,215359488,35328,(0,46,92,138),0),-5,(3,215359488,0)),
    ((25,7500000,100,8),(136,512,9,256,864,3,12,90243072,34816,(0,17,34,51,68,85,102,119,136),0),-5,(3,90243072,0)),
    ((25,7500000,150,1),(226,512,9,256,5520,3,12,958095360,57856,(0,226),0),-5,(3,958095360,0)),
    ((25,7500000,150,2),(226,512,9,256,2880,3,12,499875840,57856,(0,113,226),0),-5,(3,499875840,0)),
    ((25,7500000,150,3),(228,512,9,256,1968,3,12,344604672,58368,(0,76,152,228),0),-5,(3,344604672,0)),
    ((25,7500000,150,8),(232,512,9,256,832,3,12,148242432,59392,(0,29,58,87,116,145,174,203,232),0),-5,(3,148242432,0)),
    ((25,7500000,251,1),(203,1024,10,256,10528,3,12,1641357312,51968,(0,203),0),-5,(3,1641357312,0)),
    ((25,7500000,251,2),(204,1024,10,256,5392,3,12,844775424,52224,(0,102,204),0),-5,(3,844775424,0)),
    ((25,7500000,251,3),(204,1024,10,256,3680,3,12,576552960,52224,(0,68,136,204),0),-5,(3,576552960,0)),
    ((25,7500000,251,8),(208,1024,10,256,1472,3,12,235143168,53248,(0,26,52,78,104,130,156,182,208),0),-5,(3,235143168,0)),
    ((25,900000000,25,1),(215,512,9,256,38672,3,12,6385520640,55040,(0,215),0),-5,(3,6385520640,0)),
    ((25,900000000,25,2),(216,512,9,256,19504,3,12,3235479552,55296,(0,108,216),0),-5,(3,3235479552,0)),
    ((25,900000000,25,3),(216,512,9,256,13152,3,12,2181758976,55296,(0,72,144,216),0),-5,(3,2181758976,0)),
    ((25,900000000,25,8),(216,512,9,256,5120,3,12,849346560,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,849346560,0)),
    ((25,900000000,100,1),(255,4096,12,256,338272,3,12,66247188480,65280,(0,255),0),-5,(3,66247188480,0)),
    ((25,900000000,100,2),(254,4096,12,256,170512,3,12,33262116864,65024,(0,127,254),0),-5,(3,33262116864,0)),
    ((25,900000000,100,3),(255,4096,12,256,113600,3,12,22247424000,65280,(0,85,170,255),0),-5,(3,22247424000,0)),
    ((25,900000000,100,8),(248,4096,12,256,44288,3,12,8435269632,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,8435269632,0)),
    ((25,900000000,150,1),(255,4096,12,256,541344,3,12,106016808960,65280,(0,255),0),-5,(3,106016808960,0)),
    ((25,900000000,150,2),(254,4096,12,256,272624,3,12,53181308928,65024,(0,127,254),0),-5,(3,53181308928,0)),
    ((25,900000000,150,3),(255,4096,12,256,181504,3,12,35545743360,65280,(0,85,170,255),0),-5,(3,35545743360,0)),
    ((25,900000000,150,8),(248,4096,12,256,70592,3,12,13445234688,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,13445234688,0)),
    ((25,900000000,251,1),(255,4096,12,256,951168,3,12,186276741120,65280,(0,255),0),-5,(3,186276741120,0)),
    ((25,900000000,251,2),(254,4096,12,256,478624,3,12,93366140928,65024,(0,127,254),0),-5,(3,93366140928,0)),
    ((25,900000000,251,3),(255,4096,12,256,318448,3,12,62364856320,65280,(0,85,170,255),0),-5,(3,62364856320,0)),
    ((25,900000000,251,8),(248,4096,12,256,123584,3,12,23538302976,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,23538302976,0)),
    ((31,1,31,1),(1,1,0,1,2384,3,12,7152,1,(0,1),0),0,(2,4768,1)),
    ((31,1,31,2),(2,1,0,1,1280,3,12,7680,2,(0,1,2),0),0,(2,5120,1)),
    ((31,1,31,3),(3,1,0,1,896,3,12,8064,3,(0,1,2,3),0),0,(2,5376,1)),
    ((31,1,31,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),0,(2,6656,1)),
    ((31,1,100,1),(1,1,0,1,2400,3,12,7200,1,(0,1),0),0,(2,4800,1)),
    ((31,1,100,2),(2,1,0,1,1280,3,12,7680,2,(0,1,2),0),0,(2,5120,1)),
    ((31,1,100,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),0,(2,5472,1)),
    ((31,1,100,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),0,(2,6656,1)),
    ((31,1,150,1),(1,1,0,1,2400,3,12,7200,1,(0,1),0),0,(2,4800,1)),
    ((31,1,150,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),0,(2,5184,1)),
    ((31,1,150,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),0,(2,5472,1)),
    ((31,1,150,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),0,(2,6656,1)),
    ((31,1,251,1),(1,1,0,1,2432,3,12,7296,1,(0,1),0),-5,(3,7296,0)),
    ((31,1,251,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((31,1,251,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((31,1,251,8),(8,1,0,1,432,3,12,10368,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,10368,0)),
    ((31,1000,31,1),(1,1,0,2,2464,3,12,14784,2,(0,1),0),0,(2,9856,1)),
    ((31,1000,31,2),(2,1,0,1,1872,3,12,11232,2,(0,1,2),0),0,(2,7488,1)),
    ((31,1000,31,3),(3,1,0,1,1168,3,12,10512,3,(0,1,2,3),0),0,(2,7008,1)),
    ((31,1000,31,8),(8,1,0,1,464,3,12,11136,8,(0,1,2,3,4,5,6,7,8),0),0,(2,7424,1)),
    ((31,1000,100,1),(3,4,2,2,3504,3,12,63072,6,(0,3),0),0,(2,42048,1)),
    ((31,1000,100,2),(4,4,2,1,2960,3,12,35520,4,(0,2,4),0),0,(2,23680,1)),
    ((31,1000,100,3),(3,4,2,1,2896,3,12,26064,3,(0,1,2,3),0),0,(2,17376,1)),
    ((31,1000,100,8),(8,4,2,1,720,3,12,17280,8,(0,1,2,3,4,5,6,7,8),0),0,(2,11520,1)),
    ((31,1000,150,1),(4,4,2,2,4064,3,12,97536,8,(0,4),0),0,(2,65024,1)),
    ((31,1000,150,2),(4,4,2,1,4336,3,12,52032,4,(0,2,4),0),0,(2,34688,1)),
    ((31,1000,150,3),(6,4,2,1,2160,3,12,38880,6,(0,2,4,6),0),0,(2,25920,1)),
    ((31,1000,150,8),(8,4,2,1,896,3,12,21504,8,(0,1,2,3,4,5,6,7,8),0),0,(2,14336,1)),
    ((31,1000,251,1),(4,8,3,2,6816,3,12,163584,8,(0,4),0),-5,(3,163584,0)),
    ((31,1000,251,2),(4,8,3,1,7072,3,12,84864,4,(0,2,4),0),-5,(3,84864,0)),
    ((31,1000,251,3),(6,8,3,1,3408,3,12,61344,6,(0,2,4,6),0),-5,(3,61344,0)),
    ((31,1000,251,8),(8,8,3,1,1264,3,12,30336,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,30336,0)),
    ((31,2000000,31,1),(16,16,4,256,1344,3,12,16515072,4096,(0,16),0),0,(2,11010048,1)),
    ((31,2000000,31,2),(16,16,4,256,736,3,12,9043968,4096,(0,8,16),0),0,(2,6029312,1)),
    ((31,2000000,31,3),(18,16,4,256,496,3,12,6856704,4608,(0,6,12,18),0),0,(2,4571136,1)),
    ((31,2000000,31,8),(16,16,4,256,272,3,12,3342336,4096,(0,2,4,6,8,10,12,14,16),0),0,(2,2228224,1)),
    ((31,2000000,100,1),(67,256,8,256,2256,3,12,116084736,17152,(0,67),0),0,(2,77389824,1)),
    ((31,2000000,100,2),(68,256,8,256,1200,3,12,62668800,17408,(0,34,68),0),0,(2,41779200,1)),
    ((31,2000000,100,3),(69,256,8,256,848,3,12,44937216,17664,(0,23,46,69),0),0,(2,29958144,1)),
    ((31,2000000,100,8),(72,256,8,256,384,3,12,21233664,18432,(0,9,18,27,36,45,54,63,72),0),0,(2,14155776,1)),
    ((31,2000000,150,1),(115,256,8,256,2160,3,12,190771200,29440,(0,115),0),0,(2,127180800,1)),
    ((31,2000000,150,2),(116,256,8,256,1152,3,12,102629376,29696,(0,58,116),0),0,(2,68419584,1)),
    ((31,2000000,150,3),(117,256,8,256,816,3,12,73322496,29952,(0,39,78,117),0),0,(2,48881664,1)),
    ((31,2000000,150,8),(120,256,8,256,384,3,12,35389440,30720,(0,15,30,45,60,75,90,105,120),0),0,(2,23592960,1)),
    ((31,2000000,251,1),(211,256,8,256,2096,3,12,339652608,54016,(0,211),0),-5,(3,339652608,0)),
    ((31,2000000,251,2),(212,256,8,256,1136,3,12,184958976,54272,(0,106,212),0),-5,(3,184958976,0)),
    ((31,2000000,251,3),(213,256,8,256,800,3,12,130867200,54528,(0,71,142,213),0),-5,(3,130867200,0)),
    ((31,2000000,251,8),(216,256,8,256,368,3,12,61046784,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,61046784,0)),
    ((31,7500000,31,1),(29,32,5,256,2576,3,12,57372672,7424,(0,29),0),0,(2,38248448,1)),
    ((31,7500000,31,2),(30,32,5,256,1328,3,12,30597120,7680,(0,15,30),0),0,(2,20398080,1)),
    ((31,7500000,31,3),(30,32,5,256,944,3,12,21749760,7680,(0,10,20,30),0),0,(2,14499840,1)),
    ((31,7500000,31,8),(32,32,5,256,416,3,12,10223616,8192,(0,4,8,12,16,20,24,28,32),0),0,(2,6815744,1)),
    ((31,7500000,100,1),(251,256,8,256,2272,3,12,437968896,64256,(0,251),0),0,(2,291979264,1)),
    ((31,7500000,100,2),(252,256,8,256,1216,3,12,235339776,64512,(0,126,252),0),0,(2,156893184,1)),
    ((31,7500000,100,3),(252,256,8,256,864,3,12,167215104,64512,(0,84,168,252),0),0,(2,111476736,1)),
    ((31,7500000,100,8),(248,256,8,256,400,3,12,76185600,63488,(0,31,62,93,124,155,186,217,248),0),0,(2,50790400,1)),
    ((31,7500000,150,1),(215,512,9,256,4112,3,12,678973440,55040,(0,215),0),0,(2,452648960,1)),
    ((31,7500000,150,2),(216,512,9,256,2160,3,12,358318080,55296,(0,108,216),0),0,(2,238878720,1)),
    ((31,7500000,150,3),(216,512,9,256,1504,3,12,249495552,55296,(0,72,144,216),0),0,(2,166330368,1)),
    ((31,7500000,150,8),(216,512,9,256,656,3,12,108822528,55296,(0,27,54,81,108,135,162,189,216),0),0,(2,72548352,1)),
    ((31,7500000,251,1),(198,1024,10,256,7696,3,12,1170284544,50688,(0,198),0),-5,(3,1170284544,0)),
    ((31,7500000,251,2),(198,1024,10,256,3984,3,12,605822976,50688,(0,99,198),0),-5,(3,605822976,0)),
    ((31,7500000,251,3),(198,1024,10,256,2736,3,12,416047104,50688,(0,66,132,198),0),-5,(3,416047104,0)),
    ((31,7500000,251,8),(200,1024,10,256,1120,3,12,172032000,51200,(0,25,50,75,100,125,150,175,200),0),-5,(3,172032000,0)),
    ((31,900000000,31,1),(215,512,9,256,37280,3,12,6155673600,55040,(0,215),0),0,(2,4103782400,1)),
    ((31,900000000,31,2),(216,512,9,256,18816,3,12,3121348608,55296,(0,108,216),0),0,(2,2080899072,1)),
    ((31,900000000,31,3),(216,512,9,256,12672,3,12,2102132736,55296,(0,72,144,216),0),0,(2,1401421824,1)),
    ((31,900000000,31,8),(216,512,9,256,4944,3,12,820150272,55296,(0,27,54,81,108,135,162,189,216),0),0,(2,546766848,1)),
    ((31,900000000,100,1),(255,4096,12,256,232560,3,12,45544550400,65280,(0,255),0),0,(2,30363033600,1)),
    ((31,900000000,100,2),(254,4096,12,256,117328,3,12,22887407616,65024,(0,127,254),0),0,(2,15258271744,1)),
    ((31,900000000,100,3),(255,4096,12,256,78224,3,12,15319388160,65280,(0,85,170,255),0),0,(2,10212925440,1)),
    ((31,900000000,100,8),(248,4096,12,256,30576,3,12,5823627264,63488,(0,31,62,93,124,155,186,217,248),0),0,(2,3882418176,1)),
    ((31,900000000,150,1),(255,4096,12,256,377744,3,12,73977384960,65280,(0,255),0),0,(2,49318256640,1)),
    ((31,900000000,150,2),(254,4096,12,256,190368,3,12,37135466496,65024,(0,127,254),0),0,(2,24756977664,1)),
    ((31,900000000,150,3),(255,4096,12,256,126800,3,12,24832512000,65280,(0,85,170,255),0),0,(2,16555008000,1)),
    ((31,900000000,150,8),(248,4096,12,256,49408,3,12,9410445312,63488,(0,31,62,93,124,155,186,217,248),0),0,(2,6273630208,1)),
    ((31,900000000,251,1),(255,4096,12,256,670656,3,12,131341271040,65280,(0,255),0),-5,(3,131341271040,0)),
    ((31,900000000,251,2),(254,4096,12,256,337632,3,12,65862549504,65024,(0,127,254),0),-5,(3,65862549504,0)),
    ((31,900000000,251,3),(255,4096,12,256,224720,3,12,44009164800,65280,(0,85,170,255),0),-5,(3,44009164800,0)),
    ((31,900000000,251,8),(248,4096,12,256,87328,3,12,16632840192,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,16632840192,0)),
    ((32,1,32,1),(1,1,0,1,2384,3,12,7152,1,(0,1),0),-5,(3,7152,0)),
    ((32,1,32,2),(2,1,0,1,1280,3,12,7680,2,(0,1,2),0),-5,(3,7680,0)),
    ((32,1,32,3),(3,1,0,1,896,3,12,8064,3,(0,1,2,3),0),-5,(3,8064,0)),
    ((32,1,32,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((32,1,100,1),(1,1,0,1,2384,3,12,7152,1,(0,1),0),-5,(3,7152,0)),
    ((32,1,100,2),(2,1,0,1,1280,3,12,7680,2,(0,1,2),0),-5,(3,7680,0)),
    ((32,1,100,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((32,1,100,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((32,1,150,1),(1,1,0,1,2400,3,12,7200,1,(0,1),0),-5,(3,7200,0)),
    ((32,1,150,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((32,1,150,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((32,1,150,8),(8,1,0,1,416,3,12,9984,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,9984,0)),
    ((32,1,251,1),(1,1,0,1,2416,3,12,7248,1,(0,1),0),-5,(3,7248,0)),
    ((32,1,251,2),(2,1,0,1,1296,3,12,7776,2,(0,1,2),0),-5,(3,7776,0)),
    ((32,1,251,3),(3,1,0,1,912,3,12,8208,3,(0,1,2,3),0),-5,(3,8208,0)),
    ((32,1,251,8),(8,1,0,1,432,3,12,10368,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,10368,0)),
    ((32,1000,32,1),(1,1,0,2,2448,3,12,14688,2,(0,1),0),-5,(3,14688,0)),
    ((32,1000,32,2),(2,1,0,1,1872,3,12,11232,2,(0,1,2),0),-5,(3,11232,0)),
    ((32,1000,32,3),(3,1,0,1,1168,3,12,10512,3,(0,1,2,3),0),-5,(3,10512,0)),
    ((32,1000,32,8),(8,1,0,1,464,3,12,11136,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,11136,0)),
    ((32,1000,100,1),(3,4,2,2,3360,3,12,60480,6,(0,3),0),-5,(3,60480,0)),
    ((32,1000,100,2),(4,4,2,1,2848,3,12,34176,4,(0,2,4),0),-5,(3,34176,0)),
    ((32,1000,100,3),(3,4,2,1,2800,3,12,25200,3,(0,1,2,3),0),-5,(3,25200,0)),
    ((32,1000,100,8),(8,4,2,1,704,3,12,16896,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,16896,0)),
    ((32,1000,150,1),(4,4,2,2,3888,3,12,93312,8,(0,4),0),-5,(3,93312,0)),
    ((32,1000,150,2),(4,4,2,1,4160,3,12,49920,4,(0,2,4),0),-5,(3,49920,0)),
    ((32,1000,150,3),(6,4,2,1,2080,3,12,37440,6,(0,2,4,6),0),-5,(3,37440,0)),
    ((32,1000,150,8),(8,4,2,1,880,3,12,21120,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,21120,0)),
    ((32,1000,251,1),(4,8,3,2,6512,3,12,156288,8,(0,4),0),-5,(3,156288,0)),
    ((32,1000,251,2),(4,8,3,1,6784,3,12,81408,4,(0,2,4),0),-5,(3,81408,0)),
    ((32,1000,251,3),(6,8,3,1,3280,3,12,59040,6,(0,2,4,6),0),-5,(3,59040,0)),
    ((32,1000,251,8),(8,8,3,1,1216,3,12,29184,8,(0,1,2,3,4,5,6,7,8),0),-5,(3,29184,0)),
    ((32,2000000,32,1),(16,16,4,256,1328,3,12,16318464,4096,(0,16),0),-5,(3,16318464,0)),
    ((32,2000000,32,2),(16,16,4,256,736,3,12,9043968,4096,(0,8,16),0),-5,(3,9043968,0)),
    ((32,2000000,32,3),(18,16,4,256,496,3,12,6856704,4608,(0,6,12,18),0),-5,(3,6856704,0)),
    ((32,2000000,32,8),(16,16,4,256,272,3,12,3342336,4096,(0,2,4,6,8,10,12,14,16),0),-5,(3,3342336,0)),
    ((32,2000000,100,1),(66,256,8,256,2192,3,12,111108096,16896,(0,66),0),-5,(3,111108096,0)),
    ((32,2000000,100,2),(66,256,8,256,1184,3,12,60014592,16896,(0,33,66),0),-5,(3,60014592,0)),
    ((32,2000000,100,3),(66,256,8,256,832,3,12,42172416,16896,(0,22,44,66),0),-5,(3,42172416,0)),
    ((32,2000000,100,8),(72,256,8,256,368,3,12,20348928,18432,(0,9,18,27,36,45,54,63,72),0),-5,(3,20348928,0)),
    ((32,2000000,150,1),(114,256,8,256,2080,3,12,182108160,29184,(0,114),0),-5,(3,182108160,0)),
    ((32,2000000,150,2),(114,256,8,256,1120,3,12,98058240,29184,(0,57,114),0),-5,(3,98058240,0)),
    ((32,2000000,150,3),(114,256,8,256,800,3,12,70041600,29184,(0,38,76,114),0),-5,(3,70041600,0)),
    ((32,2000000,150,8),(120,256,8,256,368,3,12,33914880,30720,(0,15,30,45,60,75,90,105,120),0),-5,(3,33914880,0)),
    ((32,2000000,251,1),(210,256,8,256,2016,3,12,325140480,53760,(0,210),0),-5,(3,325140480,0)),
    ((32,2000000,251,2),(210,256,8,256,1088,3,12,175472640,53760,(0,105,210),0),-5,(3,175472640,0)),
    ((32,2000000,251,3),(210,256,8,256,784,3,12,126443520,53760,(0,70,140,210),0),-5,(3,126443520,0)),
    ((32,2000000,251,8),(216,256,8,256,368,3,12,61046784,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,61046784,0)),
    ((32,7500000,32,1),(29,32,5,256,2560,3,12,57016320,7424,(0,29),0),-5,(3,57016320,0)),
    ((32,7500000,32,2),(30,32,5,256,1328,3,12,30597120,7680,(0,15,30),0),-5,(3,30597120,0)),
    ((32,7500000,32,3),(30,32,5,256,944,3,12,21749760,7680,(0,10,20,30),0),-5,(3,21749760,0)),
    ((32,7500000,32,8),(32,32,5,256,416,3,12,10223616,8192,(0,4,8,12,16,20,24,28,32),0),-5,(3,10223616,0)),
    ((32,7500000,100,1),(247,256,8,256,2192,3,12,415813632,63232,(0,247),0),-5,(3,415813632,0)),
    ((32,7500000,100,2),(248,256,8,256,1184,3,12,225509376,63488,(0,124,248),0),-5,(3,225509376,0)),
    ((32,7500000,100,3),(249,256,8,256,832,3,12,159105024,63744,(0,83,166,249),0),-5,(3,159105024,0)),
    ((32,7500000,100,8),(248,256,8,256,384,3,12,73138176,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,73138176,0)),
    ((32,7500000,150,1),(213,512,9,256,3952,3,12,646483968,54528,(0,213),0),-5,(3,646483968,0)),
    ((32,7500000,150,2),(214,512,9,256,2080,3,12,341852160,54784,(0,107,214),0),-5,(3,341852160,0)),
    ((32,7500000,150,3),(213,512,9,256,1456,3,12,238178304,54528,(0,71,142,213),0),-5,(3,238178304,0)),
    ((32,7500000,150,8),(216,512,9,256,624,3,12,103514112,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,103514112,0)),
    ((32,7500000,251,1),(197,1024,10,256,7376,3,12,1115959296,50432,(0,197),0),-5,(3,1115959296,0)),
    ((32,7500000,251,2),(198,1024,10,256,3808,3,12,579059712,50688,(0,99,198),0),-5,(3,579059712,0)),
    ((32,7500000,251,3),(198,1024,10,256,2608,3,12,396582912,50688,(0,66,132,198),0),-5,(3,396582912,0)),
    ((32,7500000,251,8),(200,1024,10,256,1072,3,12,164659200,51200,(0,25,50,75,100,125,150,175,200),0),-5,(3,164659200,0)),
    ((32,900000000,32,1),(215,512,9,256,37120,3,12,6129254400,55040,(0,215),0),-5,(3,6129254400,0)),
    ((32,900000000,32,2),(216,512,9,256,18736,3,12,3108077568,55296,(0,108,216),0),-5,(3,3108077568,0)),
    ((32,900000000,32,3),(216,512,9,256,12624,3,12,2094170112,55296,(0,72,144,216),0),-5,(3,2094170112,0)),
    ((32,900000000,32,8),(216,512,9,256,4928,3,12,817496064,55296,(0,27,54,81,108,135,162,189,216),0),-5,(3,817496064,0)),
    ((32,900000000,100,1),(255,4096,12,256,220544,3,12,43191336960,65280,(0,255),0),-5,(3,43191336960,0)),
    ((32,900000000,100,2),(254,4096,12,256,111280,3,12,21707612160,65024,(0,127,254),0),-5,(3,21707612160,0)),
    ((32,900000000,100,3),(255,4096,12,256,74208,3,12,14532894720,65280,(0,85,170,255),0),-5,(3,14532894720,0)),
    ((32,900000000,100,8),(248,4096,12,256,29008,3,12,5524979712,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,5524979712,0)),
    ((32,900000000,150,1),(255,4096,12,256,359136,3,12,70333194240,65280,(0,255),0),-5,(3,70333194240,0)),
    ((32,900000000,150,2),(254,4096,12,256,181008,3,12,35309592576,65024,(0,127,254),0),-5,(3,35309592576,0)),
    ((32,900000000,150,3),(255,4096,12,256,120592,3,12,23616737280,65280,(0,85,170,255),0),-5,(3,23616737280,0)),
    ((32,900000000,150,8),(248,4096,12,256,46992,3,12,8950284288,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,8950284288,0)),
    ((32,900000000,251,1),(255,4096,12,256,638768,3,12,125096325120,65280,(0,255),0),-5,(3,125096325120,0)),
    ((32,900000000,251,2),(254,4096,12,256,321600,3,12,62735155200,65024,(0,127,254),0),-5,(3,62735155200,0)),
    ((32,900000000,251,3),(255,4096,12,256,214064,3,12,41922293760,65280,(0,85,170,255),0),-5,(3,41922293760,0)),
    ((32,900000000,251,8),(248,4096,12,256,83200,3,12,15846604800,63488,(0,31,62,93,124,155,186,217,248),0),-5,(3,15846604800,0)),
    ((33,1,33,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((33,1,33,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((33,1,33,3),(3,1,0,1,896,4,12,10752,3,(0,1,2,3),0),-5,(4,10752,0)),
    ((33,1,33,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((33,1,100,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((33,1,100,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((33,1,100,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((33,1,100,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((33,1,150,1),(1,1,0,1,2400,4,12,9600,1,(0,1),0),-5,(4,9600,0)),
    ((33,1,150,2),(2,1,0,1,1296,4,12,10368,2,(0,1,2),0),-5,(4,10368,0)),
    ((33,1,150,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((33,1,150,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((33,1,251,1),(1,1,0,1,2416,4,12,9664,1,(0,1),0),-5,(4,9664,0)),
    ((33,1,251,2),(2,1,0,1,1296,4,12,10368,2,(0,1,2),0),-5,(4,10368,0)),
    ((33,1,251,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((33,1,251,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((33,1000,33,1),(1,1,0,2,2448,4,12,19584,2,(0,1),0),-5,(4,19584,0)),
    ((33,1000,33,2),(2,1,0,1,1872,4,12,14976,2,(0,1,2),0),-5,(4,14976,0)),
    ((33,1000,33,3),(3,1,0,1,1168,4,12,14016,3,(0,1,2,3),0),-5,(4,14016,0)),
    ((33,1000,33,8),(8,1,0,1,464,4,12,14848,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,14848,0)),
    ((33,1000,100,1),(3,8,3,2,3216,4,12,77184,6,(0,3),0),-5,(4,77184,0)),
    ((33,1000,100,2),(4,8,3,1,2736,4,12,43776,4,(0,2,4),0),-5,(4,43776,0)),
    ((33,1000,100,3),(3,8,3,1,2704,4,12,32448,3,(0,1,2,3),0),-5,(4,32448,0)),
    ((33,1000,100,8),(8,8,3,1,688,4,12,22016,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,22016,0)),
    ((33,1000,150,1),(5,8,3,2,3024,4,12,120960,10,(0,5),0),-5,(4,120960,0)),
    ((33,1000,150,2),(6,8,3,1,2736,4,12,65664,6,(0,3,6),0),-5,(4,65664,0)),
    ((33,1000,150,3),(6,8,3,1,2016,4,12,48384,6,(0,2,4,6),0),-5,(4,48384,0)),
    ((33,1000,150,8),(8,8,3,1,848,4,12,27136,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,27136,0)),
    ((33,1000,251,1),(5,16,4,2,5056,4,12,202240,10,(0,5),0),-5,(4,202240,0)),
    ((33,1000,251,2),(6,16,4,1,4432,4,12,106368,6,(0,3,6),0),-5,(4,106368,0)),
    ((33,1000,251,3),(6,16,4,1,3152,4,12,75648,6,(0,2,4,6),0),-5,(4,75648,0)),
    ((33,1000,251,8),(8,16,4,1,1184,4,12,37888,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,37888,0)),
    ((33,2000000,33,1),(21,32,5,256,1056,4,12,22708224,5376,(0,21),0),-5,(4,22708224,0)),
    ((33,2000000,33,2),(22,32,5,256,576,4,12,12976128,5632,(0,11,22),0),-5,(4,12976128,0)),
    ((33,2000000,33,3),(21,32,5,256,432,4,12,9289728,5376,(0,7,14,21),0),-5,(4,9289728,0)),
    ((33,2000000,33,8),(24,32,5,256,208,4,12,5111808,6144,(0,3,6,9,12,15,18,21,24),0),-5,(4,5111808,0)),
    ((33,2000000,100,1),(173,256,8,256,896,4,12,158728192,44288,(0,173),0),-5,(4,158728192,0)),
    ((33,2000000,100,2),(174,256,8,256,512,4,12,91226112,44544,(0,87,174),0),-5,(4,91226112,0)),
    ((33,2000000,100,3),(174,256,8,256,384,4,12,68419584,44544,(0,58,116,174),0),-5,(4,68419584,0)),
    ((33,2000000,100,8),(176,256,8,256,208,4,12,37486592,45056,(0,22,44,66,88,110,132,154,176),0),-5,(4,37486592,0)),
    ((33,2000000,150,1),(151,512,9,256,1552,4,12,239976448,38656,(0,151),0),-5,(4,239976448,0)),
    ((33,2000000,150,2),(152,512,9,256,848,4,12,131989504,38912,(0,76,152),0),-5,(4,131989504,0)),
    ((33,2000000,150,3),(153,512,9,256,608,4,12,95256576,39168,(0,51,102,153),0),-5,(4,95256576,0)),
    ((33,2000000,150,8),(152,512,9,256,304,4,12,47316992,38912,(0,19,38,57,76,95,114,133,152),0),-5,(4,47316992,0)),
    ((33,2000000,251,1),(140,1024,10,256,2800,4,12,401408000,35840,(0,140),0),-5,(4,401408000,0)),
    ((33,2000000,251,2),(140,1024,10,256,1488,4,12,213319680,35840,(0,70,140),0),-5,(4,213319680,0)),
    ((33,2000000,251,3),(141,1024,10,256,1040,4,12,150159360,36096,(0,47,94,141),0),-5,(4,150159360,0)),
    ((33,2000000,251,8),(144,1024,10,256,464,4,12,68419584,36864,(0,18,36,54,72,90,108,126,144),0),-5,(4,68419584,0)),
    ((33,7500000,33,1),(39,64,6,256,1952,4,12,77955072,9984,(0,39),0),-5,(4,77955072,0)),
    ((33,7500000,33,2),(40,64,6,256,1040,4,12,42598400,10240,(0,20,40),0),-5,(4,42598400,0)),
    ((33,7500000,33,3),(39,64,6,256,752,4,12,30031872,9984,(0,13,26,39),0),-5,(4,30031872,0)),
    ((33,7500000,33,8),(40,64,6,256,352,4,12,14417920,10240,(0,5,10,15,20,25,30,35,40),0),-5,(4,14417920,0)),
    ((33,7500000,100,1),(163,1024,10,256,3056,4,12,510083072,41728,(0,163),0),-5,(4,510083072,0)),
    ((33,7500000,100,2),(164,1024,10,256,1616,4,12,271384576,41984,(0,82,164),0),-5,(4,271384576,0)),
    ((33,7500000,100,3),(165,1024,10,256,1120,4,12,189235200,42240,(0,55,110,165),0),-5,(4,189235200,0)),
    ((33,7500000,100,8),(168,1024,10,256,496,4,12,85327872,43008,(0,21,42,63,84,105,126,147,168),0),-5,(4,85327872,0)),
    ((33,7500000,150,1),(141,2048,11,256,5584,4,12,806240256,36096,(0,141),0),-5,(4,806240256,0)),
    ((33,7500000,150,2),(142,2048,11,256,2896,4,12,421101568,36352,(0,71,142),0),-5,(4,421101568,0)),
    ((33,7500000,150,3),(141,2048,11,256,2000,4,12,288768000,36096,(0,47,94,141),0),-5,(4,288768000,0)),
    ((33,7500000,150,8),(144,2048,11,256,832,4,12,122683392,36864,(0,18,36,54,72,90,108,126,144),0),-5,(4,122683392,0)),
    ((33,7500000,251,1),(131,4096,12,256,10448,4,12,1401536512,33536,(0,131),0),-5,(4,1401536512,0)),
    ((33,7500000,251,2),(132,4096,12,256,5344,4,12,722337792,33792,(0,66,132),0),-5,(4,722337792,0)),
    ((33,7500000,251,3),(132,4096,12,256,3648,4,12,493092864,33792,(0,44,88,132),0),-5,(4,493092864,0)),
    ((33,7500000,251,8),(136,4096,12,256,1440,4,12,200540160,34816,(0,17,34,51,68,85,102,119,136),0),-5,(4,200540160,0)),
    ((33,900000000,33,1),(144,2048,11,256,54880,4,12,8092385280,36864,(0,144),0),-5,(4,8092385280,0)),
    ((33,900000000,33,2),(144,2048,11,256,27744,4,12,4091019264,36864,(0,72,144),0),-5,(4,4091019264,0)),
    ((33,900000000,33,3),(144,2048,11,256,18656,4,12,2750939136,36864,(0,48,96,144),0),-5,(4,2750939136,0)),
    ((33,900000000,33,8),(144,2048,11,256,7216,4,12,1064042496,36864,(0,18,36,54,72,90,108,126,144),0),-5,(4,1064042496,0)),
    ((33,900000000,100,1),(255,4096,12,256,209568,4,12,54722396160,65280,(0,255),0),-5,(4,54722396160,0)),
    ((33,900000000,100,2),(254,4096,12,256,105760,4,12,27507752960,65024,(0,127,254),0),-5,(4,27507752960,0)),
    ((33,900000000,100,3),(255,4096,12,256,70528,4,12,18416271360,65280,(0,85,170,255),0),-5,(4,18416271360,0)),
    ((33,900000000,100,8),(248,4096,12,256,27584,4,12,7005011968,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,7005011968,0)),
    ((33,900000000,150,1),(255,4096,12,256,342160,4,12,89344819200,65280,(0,255),0),-5,(4,89344819200,0)),
    ((33,900000000,150,2),(254,4096,12,256,172464,4,12,44857196544,65024,(0,127,254),0),-5,(4,44857196544,0)),
    ((33,900000000,150,3),(255,4096,12,256,114896,4,12,30001643520,65280,(0,85,170,255),0),-5,(4,30001643520,0)),
    ((33,900000000,150,8),(248,4096,12,256,44800,4,12,11377049600,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,11377049600,0)),
    ((33,900000000,251,1),(255,4096,12,256,609648,4,12,159191285760,65280,(0,255),0),-5,(4,159191285760,0)),
    ((33,900000000,251,2),(254,4096,12,256,306976,4,12,79843229696,65024,(0,127,254),0),-5,(4,79843229696,0)),
    ((33,900000000,251,3),(255,4096,12,256,204336,4,12,53356216320,65280,(0,85,170,255),0),-5,(4,53356216320,0)),
    ((33,900000000,251,8),(248,4096,12,256,79424,4,12,20169883648,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,20169883648,0)),
    ((51,1,51,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((51,1,51,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((51,1,51,3),(3,1,0,1,896,4,12,10752,3,(0,1,2,3),0),-5,(4,10752,0)),
    ((51,1,51,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((51,1,100,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((51,1,100,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((51,1,100,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((51,1,100,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((51,1,150,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((51,1,150,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((51,1,150,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((51,1,150,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((51,1,251,1),(1,1,0,1,2400,4,12,9600,1,(0,1),0),-5,(4,9600,0)),
    ((51,1,251,2),(2,1,0,1,1296,4,12,10368,2,(0,1,2),0),-5,(4,10368,0)),
    ((51,1,251,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((51,1,251,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((51,1000,51,1),(1,1,0,2,2400,4,12,19200,2,(0,1),0),-5,(4,19200,0)),
    ((51,1000,51,2),(2,1,0,1,1840,4,12,14720,2,(0,1,2),0),-5,(4,14720,0)),
    ((51,1000,51,3),(3,1,0,1,1152,4,12,13824,3,(0,1,2,3),0),-5,(4,13824,0)),
    ((51,1000,51,8),(8,1,0,1,464,4,12,14848,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,14848,0)),
    ((51,1000,100,1),(3,8,3,2,1872,4,12,44928,6,(0,3),0),-5,(4,44928,0)),
    ((51,1000,100,2),(4,8,3,1,1712,4,12,27392,4,(0,2,4),0),-5,(4,27392,0)),
    ((51,1000,100,3),(3,8,3,1,1792,4,12,21504,3,(0,1,2,3),0),-5,(4,21504,0)),
    ((51,1000,100,8),(8,8,3,1,544,4,12,17408,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,17408,0)),
    ((51,1000,150,1),(5,8,3,2,1760,4,12,70400,10,(0,5),0),-5,(4,70400,0)),
    ((51,1000,150,2),(6,8,3,1,1680,4,12,40320,6,(0,3,6),0),-5,(4,40320,0)),
    ((51,1000,150,3),(6,8,3,1,1312,4,12,31488,6,(0,2,4,6),0),-5,(4,31488,0)),
    ((51,1000,150,8),(8,8,3,1,640,4,12,20480,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,20480,0)),
    ((51,1000,251,1),(5,16,4,2,2912,4,12,116480,10,(0,5),0),-5,(4,116480,0)),
    ((51,1000,251,2),(6,16,4,1,2656,4,12,63744,6,(0,3,6),0),-5,(4,63744,0)),
    ((51,1000,251,3),(6,16,4,1,1952,4,12,46848,6,(0,2,4,6),0),-5,(4,46848,0)),
    ((51,1000,251,8),(8,16,4,1,832,4,12,26624,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,26624,0)),
    ((51,2000000,51,1),(21,32,5,256,1008,4,12,21676032,5376,(0,21),0),-5,(4,21676032,0)),
    ((51,2000000,51,2),(22,32,5,256,560,4,12,12615680,5632,(0,11,22),0),-5,(4,12615680,0)),
    ((51,2000000,51,3),(21,32,5,256,432,4,12,9289728,5376,(0,7,14,21),0),-5,(4,9289728,0)),
    ((51,2000000,51,8),(24,32,5,256,208,4,12,5111808,6144,(0,3,6,9,12,15,18,21,24),0),-5,(4,5111808,0)),
    ((51,2000000,100,1),(128,256,8,256,640,4,12,83886080,32768,(0,128),0),-5,(4,83886080,0)),
    ((51,2000000,100,2),(128,256,8,256,384,4,12,50331648,32768,(0,64,128),0),-5,(4,50331648,0)),
    ((51,2000000,100,3),(129,256,8,256,288,4,12,38043648,33024,(0,43,86,129),0),-5,(4,38043648,0)),
    ((51,2000000,100,8),(128,256,8,256,176,4,12,23068672,32768,(0,16,32,48,64,80,96,112,128),0),-5,(4,23068672,0)),
    ((51,2000000,150,1),(255,256,8,256,576,4,12,150405120,65280,(0,255),0),-5,(4,150405120,0)),
    ((51,2000000,150,2),(254,256,8,256,352,4,12,91553792,65024,(0,127,254),0),-5,(4,91553792,0)),
    ((51,2000000,150,3),(255,256,8,256,272,4,12,71024640,65280,(0,85,170,255),0),-5,(4,71024640,0)),
    ((51,2000000,150,8),(248,256,8,256,160,4,12,40632320,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,40632320,0)),
    ((51,2000000,251,1),(128,1024,10,256,1728,4,12,226492416,32768,(0,128),0),-5,(4,226492416,0)),
    ((51,2000000,251,2),(128,1024,10,256,944,4,12,123731968,32768,(0,64,128),0),-5,(4,123731968,0)),
    ((51,2000000,251,3),(129,1024,10,256,672,4,12,88768512,33024,(0,43,86,129),0),-5,(4,88768512,0)),
    ((51,2000000,251,8),(128,1024,10,256,320,4,12,41943040,32768,(0,16,32,48,64,80,96,112,128),0),-5,(4,41943040,0)),
    ((51,7500000,51,1),(39,64,6,256,1872,4,12,74760192,9984,(0,39),0),-5,(4,74760192,0)),
    ((51,7500000,51,2),(40,64,6,256,1008,4,12,41287680,10240,(0,20,40),0),-5,(4,41287680,0)),
    ((51,7500000,51,3),(39,64,6,256,736,4,12,29392896,9984,(0,13,26,39),0),-5,(4,29392896,0)),
    ((51,7500000,51,8),(40,64,6,256,336,4,12,13762560,10240,(0,5,10,15,20,25,30,35,40),0),-5,(4,13762560,0)),
    ((51,7500000,100,1),(239,512,9,256,1136,4,12,278020096,61184,(0,239),0),-5,(4,278020096,0)),
    ((51,7500000,100,2),(240,512,9,256,640,4,12,157286400,61440,(0,120,240),0),-5,(4,157286400,0)),
    ((51,7500000,100,3),(240,512,9,256,464,4,12,114032640,61440,(0,80,160,240),0),-5,(4,114032640,0)),
    ((51,7500000,100,8),(240,512,9,256,240,4,12,58982400,61440,(0,30,60,90,120,150,180,210,240),0),-5,(4,58982400,0)),
    ((51,7500000,150,1),(239,1024,10,256,1856,4,12,454230016,61184,(0,239),0),-5,(4,454230016,0)),
    ((51,7500000,150,2),(240,1024,10,256,1008,4,12,247726080,61440,(0,120,240),0),-5,(4,247726080,0)),
    ((51,7500000,150,3),(240,1024,10,256,720,4,12,176947200,61440,(0,80,160,240),0),-5,(4,176947200,0)),
    ((51,7500000,150,8),(240,1024,10,256,352,4,12,86507520,61440,(0,30,60,90,120,150,180,210,240),0),-5,(4,86507520,0)),
    ((51,7500000,251,1),(240,2048,11,256,3248,4,12,798228480,61440,(0,240),0),-5,(4,798228480,0)),
    ((51,7500000,251,2),(240,2048,11,256,1728,4,12,424673280,61440,(0,120,240),0),-5,(4,424673280,0)),
    ((51,7500000,251,3),(240,2048,11,256,1200,4,12,294912000,61440,(0,80,160,240),0),-5,(4,294912000,0)),
    ((51,7500000,251,8),(240,2048,11,256,544,4,12,133693440,61440,(0,30,60,90,120,150,180,210,240),0),-5,(4,133693440,0)),
    ((51,900000000,51,1),(144,2048,11,256,52800,4,12,7785676800,36864,(0,144),0),-5,(4,7785676800,0)),
    ((51,900000000,51,2),(144,2048,11,256,26704,4,12,3937665024,36864,(0,72,144),0),-5,(4,3937665024,0)),
    ((51,900000000,51,3),(144,2048,11,256,17968,4,12,2649489408,36864,(0,48,96,144),0),-5,(4,2649489408,0)),
    ((51,900000000,51,8),(144,2048,11,256,6960,4,12,1026293760,36864,(0,18,36,54,72,90,108,126,144),0),-5,(4,1026293760,0)),
    ((51,900000000,100,1),(255,4096,12,256,103424,4,12,27006074880,65280,(0,255),0),-5,(4,27006074880,0)),
    ((51,900000000,100,2),(254,4096,12,256,52320,4,12,13608222720,65024,(0,127,254),0),-5,(4,13608222720,0)),
    ((51,900000000,100,3),(255,4096,12,256,34960,4,12,9128755200,65280,(0,85,170,255),0),-5,(4,9128755200,0)),
    ((51,900000000,100,8),(248,4096,12,256,13776,4,12,3498442752,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,3498442752,0)),
    ((51,900000000,150,1),(255,4096,12,256,177968,4,12,46471004160,65280,(0,255),0),-5,(4,46471004160,0)),
    ((51,900000000,150,2),(254,4096,12,256,89856,4,12,23371186176,65024,(0,127,254),0),-5,(4,23371186176,0)),
    ((51,900000000,150,3),(255,4096,12,256,59952,4,12,15654666240,65280,(0,85,170,255),0),-5,(4,15654666240,0)),
    ((51,900000000,150,8),(248,4096,12,256,23488,4,12,5964824576,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,5964824576,0)),
    ((51,900000000,251,1),(255,4096,12,256,328256,4,12,85714206720,65280,(0,255),0),-5,(4,85714206720,0)),
    ((51,900000000,251,2),(254,4096,12,256,165472,4,12,43038605312,65024,(0,127,254),0),-5,(4,43038605312,0)),
    ((51,900000000,251,3),(255,4096,12,256,110256,4,12,28790046720,65280,(0,85,170,255),0),-5,(4,28790046720,0)),
    ((51,900000000,251,8),(248,4096,12,256,42992,4,12,10917904384,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,10917904384,0)),
    ((64,1,64,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((64,1,64,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((64,1,64,3),(3,1,0,1,896,4,12,10752,3,(0,1,2,3),0),-5,(4,10752,0)),
    ((64,1,64,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((64,1,100,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((64,1,100,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((64,1,100,3),(3,1,0,1,896,4,12,10752,3,(0,1,2,3),0),-5,(4,10752,0)),
    ((64,1,100,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((64,1,150,1),(1,1,0,1,2384,4,12,9536,1,(0,1),0),-5,(4,9536,0)),
    ((64,1,150,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((64,1,150,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((64,1,150,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((64,1,251,1),(1,1,0,1,2400,4,12,9600,1,(0,1),0),-5,(4,9600,0)),
    ((64,1,251,2),(2,1,0,1,1280,4,12,10240,2,(0,1,2),0),-5,(4,10240,0)),
    ((64,1,251,3),(3,1,0,1,912,4,12,10944,3,(0,1,2,3),0),-5,(4,10944,0)),
    ((64,1,251,8),(8,1,0,1,416,4,12,13312,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,13312,0)),
    ((64,1000,64,1),(1,1,0,2,2400,4,12,19200,2,(0,1),0),-5,(4,19200,0)),
    ((64,1000,64,2),(2,1,0,1,1840,4,12,14720,2,(0,1,2),0),-5,(4,14720,0)),
    ((64,1000,64,3),(3,1,0,1,1152,4,12,13824,3,(0,1,2,3),0),-5,(4,13824,0)),
    ((64,1000,64,8),(8,1,0,1,448,4,12,14336,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,14336,0)),
    ((64,1000,100,1),(4,4,2,2,1120,4,12,35840,8,(0,4),0),-5,(4,35840,0)),
    ((64,1000,100,2),(4,4,2,1,1408,4,12,22528,4,(0,2,4),0),-5,(4,22528,0)),
    ((64,1000,100,3),(6,4,2,1,832,4,12,19968,6,(0,2,4,6),0),-5,(4,19968,0)),
    ((64,1000,100,8),(8,4,2,1,512,4,12,16384,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,16384,0)),
    ((64,1000,150,1),(4,8,3,2,1680,4,12,53760,8,(0,4),0),-5,(4,53760,0)),
    ((64,1000,150,2),(4,8,3,1,1952,4,12,31232,4,(0,2,4),0),-5,(4,31232,0)),
    ((64,1000,150,3),(6,8,3,1,1088,4,12,26112,6,(0,2,4,6),0),-5,(4,26112,0)),
    ((64,1000,150,8),(8,8,3,1,576,4,12,18432,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,18432,0)),
    ((64,1000,251,1),(8,8,3,2,1472,4,12,94208,16,(0,8),0),-5,(4,94208,0)),
    ((64,1000,251,2),(8,8,3,1,1616,4,12,51712,8,(0,4,8),0),-5,(4,51712,0)),
    ((64,1000,251,3),(9,8,3,1,1104,4,12,39744,9,(0,3,6,9),0),-5,(4,39744,0)),
    ((64,1000,251,8),(8,8,3,1,720,4,12,23040,8,(0,1,2,3,4,5,6,7,8),0),-5,(4,23040,0)),
    ((64,2000000,64,1),(21,32,5,256,1008,4,12,21676032,5376,(0,21),0),-5,(4,21676032,0)),
    ((64,2000000,64,2),(22,32,5,256,544,4,12,12255232,5632,(0,11,22),0),-5,(4,12255232,0)),
    ((64,2000000,64,3),(21,32,5,256,416,4,12,8945664,5376,(0,7,14,21),0),-5,(4,8945664,0)),
    ((64,2000000,64,8),(24,32,5,256,208,4,12,5111808,6144,(0,3,6,9,12,15,18,21,24),0),-5,(4,5111808,0)),
    ((64,2000000,100,1),(95,256,8,256,592,4,12,57589760,24320,(0,95),0),-5,(4,57589760,0)),
    ((64,2000000,100,2),(96,256,8,256,352,4,12,34603008,24576,(0,48,96),0),-5,(4,34603008,0)),
    ((64,2000000,100,3),(96,256,8,256,272,4,12,26738688,24576,(0,32,64,96),0),-5,(4,26738688,0)),
    ((64,2000000,100,8),(96,256,8,256,160,4,12,15728640,24576,(0,12,24,36,48,60,72,84,96),0),-5,(4,15728640,0)),
    ((64,2000000,150,1),(222,256,8,256,496,4,12,112754688,56832,(0,222),0),-5,(4,112754688,0)),
    ((64,2000000,150,2),(222,256,8,256,304,4,12,69107712,56832,(0,111,222),0),-5,(4,69107712,0)),
    ((64,2000000,150,3),(222,256,8,256,240,4,12,54558720,56832,(0,74,148,222),0),-5,(4,54558720,0)),
    ((64,2000000,150,8),(224,256,8,256,144,4,12,33030144,57344,(0,28,56,84,112,140,168,196,224),0),-5,(4,33030144,0)),
    ((64,2000000,251,1),(240,512,9,256,768,4,12,188743680,61440,(0,240),0),-5,(4,188743680,0)),
    ((64,2000000,251,2),(240,512,9,256,448,4,12,110100480,61440,(0,120,240),0),-5,(4,110100480,0)),
    ((64,2000000,251,3),(240,512,9,256,336,4,12,82575360,61440,(0,80,160,240),0),-5,(4,82575360,0)),
    ((64,2000000,251,8),(240,512,9,256,192,4,12,47185920,61440,(0,30,60,90,120,150,180,210,240),0),-5,(4,47185920,0)),
    ((64,7500000,64,1),(39,64,6,256,1856,4,12,74121216,9984,(0,39),0),-5,(4,74121216,0)),
    ((64,7500000,64,2),(40,64,6,256,992,4,12,40632320,10240,(0,20,40),0),-5,(4,40632320,0)),
    ((64,7500000,64,3),(39,64,6,256,720,4,12,28753920,9984,(0,13,26,39),0),-5,(4,28753920,0)),
    ((64,7500000,64,8),(40,64,6,256,336,4,12,13762560,10240,(0,5,10,15,20,25,30,35,40),0),-5,(4,13762560,0)),
    ((64,7500000,100,1),(177,512,9,256,1072,4,12,194297856,45312,(0,177),0),-5,(4,194297856,0)),
    ((64,7500000,100,2),(178,512,9,256,592,4,12,107905024,45568,(0,89,178),0),-5,(4,107905024,0)),
    ((64,7500000,100,3),(177,512,9,256,448,4,12,81199104,45312,(0,59,118,177),0),-5,(4,81199104,0)),
    ((64,7500000,100,8),(184,512,9,256,224,4,12,42205184,47104,(0,23,46,69,92,115,138,161,184),0),-5,(4,42205184,0)),
    ((64,7500000,150,1),(208,1024,10,256,1552,4,12,330563584,53248,(0,208),0),-5,(4,330563584,0)),
    ((64,7500000,150,2),(208,1024,10,256,848,4,12,180617216,53248,(0,104,208),0),-5,(4,180617216,0)),
    ((64,7500000,150,3),(210,1024,10,256,608,4,12,130744320,53760,(0,70,140,210),0),-5,(4,130744320,0)),
    ((64,7500000,150,8),(208,1024,10,256,304,4,12,64749568,53248,(0,26,52,78,104,130,156,182,208),0),-5,(4,64749568,0)),
    ((64,7500000,251,1),(225,2048,11,256,2592,4,12,597196800,57600,(0,225),0),-5,(4,597196800,0)),
    ((64,7500000,251,2),(226,2048,11,256,1376,4,12,318439424,57856,(0,113,226),0),-5,(4,318439424,0)),
    ((64,7500000,251,3),(225,2048,11,256,976,4,12,224870400,57600,(0,75,150,225),0),-5,(4,224870400,0)),
    ((64,7500000,251,8),(232,2048,11,256,432,4,12,102629376,59392,(0,29,58,87,116,145,174,203,232),0),-5,(4,102629376,0)),
    ((64,900000000,64,1),(144,2048,11,256,52160,4,12,7691304960,36864,(0,144),0),-5,(4,7691304960,0)),
    ((64,900000000,64,2),(144,2048,11,256,26384,4,12,3890479104,36864,(0,72,144),0),-5,(4,3890479104,0)),
    ((64,900000000,64,3),(144,2048,11,256,17744,4,12,2616459264,36864,(0,48,96,144),0),-5,(4,2616459264,0)),
    ((64,900000000,64,8),(144,2048,11,256,6880,4,12,1014497280,36864,(0,18,36,54,72,90,108,126,144),0),-5,(4,1014497280,0)),
    ((64,900000000,100,1),(255,4096,12,256,70704,4,12,18462228480,65280,(0,255),0),-5,(4,18462228480,0)),
    ((64,900000000,100,2),(254,4096,12,256,35824,4,12,9317679104,65024,(0,127,254),0),-5,(4,9317679104,0)),
    ((64,900000000,100,3),(255,4096,12,256,23968,4,12,6258524160,65280,(0,85,170,255),0),-5,(4,6258524160,0)),
    ((64,900000000,100,8),(248,4096,12,256,9488,4,12,2409496576,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,2409496576,0)),
    ((64,900000000,150,1),(255,4096,12,256,127376,4,12,33260421120,65280,(0,255),0),-5,(4,33260421120,0)),
    ((64,900000000,150,2),(254,4096,12,256,64384,4,12,16746020864,65024,(0,127,254),0),-5,(4,16746020864,0)),
    ((64,900000000,150,3),(255,4096,12,256,42992,4,12,11226071040,65280,(0,85,170,255),0),-5,(4,11226071040,0)),
    ((64,900000000,150,8),(248,4096,12,256,16896,4,12,4290772992,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,4290772992,0)),
    ((64,900000000,251,1),(255,4096,12,256,241600,4,12,63086592000,65280,(0,255),0),-5,(4,63086592000,0)),
    ((64,900000000,251,2),(254,4096,12,256,121888,4,12,31702581248,65024,(0,127,254),0),-5,(4,31702581248,0)),
    ((64,900000000,251,3),(255,4096,12,256,81248,4,12,21215477760,65280,(0,85,170,255),0),-5,(4,21215477760,0)),
    ((64,900000000,251,8),(248,4096,12,256,31744,4,12,8061452288,63488,(0,31,62,93,124,155,186,217,248),0),-5,(4,8061452288,0)),
)


def test_exchange_plans_are_the_recorded_ones_field_by_field():
    """The planner's arithmetic (fine buckets -> C1 x F2, records per segment, writers) is pinned against a recorded table: k on both
    sides of the one-word key, one read to 900 M, reads of exactly k bases to 251, 1 to 8 destinations; the short form where the
    shape has one, KV_ERR_NOTIMPL and an untouched plan where it has not."""
    import ctypes
    from kevlar_amd import _lib
    lib = _lib.load()
    names = ('C1', 'F2', 'fbits', 'nwg1', 'cap1', 'recw', 'm', 'seg_words', 'cnt_entries')
    assert len(_MEX_PLANS) == 7 * 5 * 4 * 4
    for (k, n_reads, read_len, ndest), want, short_rc, (short_recw, short_seg_words, short_flags) in _MEX_PLANS:
        case = 'k {} reads {} length {} ndest {}'.format(k, n_reads, read_len, ndest)
        p = _lib.MexPlan()
        assert lib.kv_mex_plan_make(0, k, n_reads, read_len, ndest, ctypes.byref(p)) == 0, case
        for name, value in zip(names, want):
            assert int(getattr(p, name)) == value, (case, name)
        assert tuple(int(p.c_lo[d]) for d in range(ndest + 1)) == want[9], case
        assert int(p.flags) == want[10], case
        assert lib.kv_mex_plan_short(ctypes.byref(p)) == short_rc, case
        assert short_rc in (0, _lib.KV_ERR_NOTIMPL), case
        assert (int(p.recw), int(p.seg_words), int(p.flags)) == (short_recw, short_seg_words, short_flags), case
        for name, value in zip(names, want):                      # the short form keeps everything else
            if name not in ('recw', 'seg_words'):
                assert int(getattr(p, name)) == value, (case, name, 'short')
        assert tuple(int(p.c_lo[d]) for d in range(ndest + 1)) == want[9], case


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
    # a tuning switch exists only while something the suite runs holds its branch to the oracle: a test other than this file
    # (a fuzzer under scratch/ does not count)
    users = [p for p in glob.glob(os.path.join(ROOT, 'tests', '**', '*.py'), recursive=True) if os.path.basename(p) != 'test_host_logic.py']
    used = set()
    for path in users:
        used |= set(re.findall(r'\bKV_[A-Z_0-9]+\b', open(path).read()))
    unset = sorted(name for name, cls in table.items() if cls == 'tuning' and name not in used)
    assert not unset, 'tuning switches that no test sets: {}'.format(unset)

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
