"""`kevlar localize` without a GPU: the host logic (Localizer, seeds, ReferenceCutout) against the results the reference's
kevlar/tests/test_localize.py and test_reference.py record, and the plain-Python restatement of the matching rule
(tests/localize_common.py) against the recorded deflines, partition ids and target counts -- so the restatement the GPU tests
compare the device with is itself held to the reference."""
from io import StringIO

import pytest

import kevlar_amd
from kevlar_amd.localize import (KevlarRefrSeqNotFoundError, Localizer, contigs_2_seeds, decompose_seeds)
from kevlar_amd.reference import (KevlarDeflineSequenceLengthMismatchError, KevlarInvalidCutoutDeflineError, ReferenceCutout,
                                  load_refr_cutouts)
from kevlar_amd.sequence import Record

from conftest import data_file
import localize_common as lc


def simple_genome():
    with open(lc.fixture('simple-genome-ctrl1.fa'), 'r') as stream:
        return kevlar_amd.seqio.parse_seq_dict(stream)


def test_localizer_simple():
    intervals = Localizer(seedsize=25)
    assert list(intervals.get_cutouts()) == []
    for seqid, pos in [('chr1', 100), ('chr1', 115), ('chr2', 200), ('chr2', 205), ('chr2', 207), ('chr2', 235008), ('chr2', 235075)]:
        intervals.add_seed_match(seqid, pos)
    assert len(intervals) == 7
    assert [c.interval for c in intervals.get_cutouts()] == [('chr1', 100, 140), ('chr2', 200, 232), ('chr2', 235008, 235100)]


def test_localizer_incl_excl():
    intervals = Localizer(seedsize=25)
    for seqid, pos in [('1', 100), ('1', 120), ('12', 200), ('12', 209), ('12', 213), ('X', 1234), ('X', 1245), ('Un', 13579),
                       ('Un', 13597)]:
        intervals.add_seed_match(seqid, pos)
    assert sorted(c.interval for c in intervals.get_cutouts()) == [('1', 100, 145), ('12', 200, 238), ('Un', 13579, 13622),
                                                                   ('X', 1234, 1270)]
    intervals.exclpattern = 'Un'
    assert sorted(c.interval for c in intervals.get_cutouts()) == [('1', 100, 145), ('12', 200, 238), ('X', 1234, 1270)]
    assert len(intervals) == 7
    intervals.inclpattern = r'^\d+$'
    assert sorted(c.interval for c in intervals.get_cutouts()) == [('1', 100, 145), ('12', 200, 238)]
    assert len(intervals) == 5


def test_get_cutouts_basic():
    intervals = Localizer(seedsize=10)
    intervals.add_seed_match('bogus-genome-chr2', 10)
    with open(data_file('bogus-genome/refr.fa'), 'r') as stream:
        seqs = kevlar_amd.seqio.parse_seq_dict(stream)
    cutouts = list(intervals.get_cutouts(refrseqs=seqs))
    assert len(cutouts) == 1
    assert cutouts[0].defline == 'bogus-genome-chr2_10-20'
    assert cutouts[0].sequence == 'GTTACATTAC'


def test_get_cutouts_basic_2():
    intervals = Localizer(seedsize=21)
    for pos in (49, 52, 59):
        intervals.add_seed_match('simple', pos)
    cutouts = list(intervals.get_cutouts(refrseqs=simple_genome(), delta=5))
    assert len(cutouts) == 1
    assert cutouts[0].defline == 'simple_44-85'
    assert cutouts[0].sequence == 'AATACTATGCCGATTTATTCTTACACAATTAAATTGCTAGT'


def test_get_cutouts_basic_3():
    intervals = Localizer(seedsize=21)
    for pos in (40, 80, 120, 500):
        intervals.add_seed_match('simple', pos)
    cutouts = list(intervals.get_cutouts(refrseqs=simple_genome(), clusterdist=None, delta=10))
    assert len(cutouts) == 1
    assert cutouts[0].defline == 'simple_30-531'
    assert len(cutouts[0].sequence) == 501


def test_get_cutouts_large_span():
    seqs = simple_genome()
    intervals = Localizer(seedsize=21)
    intervals.add_seed_match('simple', 100)
    intervals.add_seed_match('simple', 200)
    assert [c.defline for c in intervals.get_cutouts(refrseqs=seqs, clusterdist=50, delta=25)] == ['simple_75-146', 'simple_175-246']
    assert [c.defline for c in intervals.get_cutouts(refrseqs=seqs, clusterdist=100, delta=50)] == ['simple_50-271']


def test_get_cutouts_missing_seq():
    intervals = Localizer(seedsize=21)
    for seqid, pos in [('simple', 100), ('simple', 200), ('TheCakeIsALie', 42), ('TheCakeIsALie', 100), ('TheCakeIsALie', 77)]:
        intervals.add_seed_match(seqid, pos)
    with pytest.raises(KevlarRefrSeqNotFoundError, match=r'TheCakeIsALie'):
        list(intervals.get_cutouts(refrseqs=simple_genome()))


def test_extract_regions_boundaries():
    seqs = simple_genome()
    intervals = Localizer(seedsize=31)
    intervals.add_seed_match('simple', 15)
    cutouts = list(intervals.get_cutouts(refrseqs=seqs, delta=20))
    assert [c.defline for c in cutouts] == ['simple_0-66']
    intervals = Localizer(seedsize=31)
    for pos in (925, 955, 978):
        intervals.add_seed_match('simple', pos)
    cutouts = list(intervals.get_cutouts(refrseqs=seqs, delta=20))
    assert [c.defline for c in cutouts] == ['simple_905-1000']
    assert len(cutouts[0].sequence) == 95


def test_decompose_seeds():
    assert list(decompose_seeds('GATTACA', 5)) == ['GATTA', 'ATTAC', 'TTACA']
    assert list(decompose_seeds('GATTACA', 3)) == ['GAT', 'ATT', 'TTA', 'TAC', 'ACA']
    assert list(decompose_seeds('GAT', 5)) == []


def test_contigs_2_seeds(kevlar_log):
    seedfile = StringIO()
    contigs_2_seeds([[Record(name='seq', sequence='GATTACA')]], seedfile, seedsize=5)
    assert seedfile.getvalue() == '>seed0\nATTAC\n>seed1\nGATTA\n>seed2\nTGTAA\n'
    log = kevlar_log.getvalue()
    assert 'decomposing contigs into seeds of length 5' in log
    assert 'contigs decomposed into 2 seeds' in log           # the index of the last seed, as the reference prints it


def test_reference_cutout_deflines():
    cutout = ReferenceCutout('chr7_1234-1244', 'ACGTACGTAC')
    assert cutout.interval == ('chr7', 1234, 1244)
    assert len(cutout) == 10
    assert cutout.local_to_global(3) == 1237
    assert ReferenceCutout('scaffold_12_5-9').interval == ('scaffold_12', 5, 9)
    assert ReferenceCutout().interval == (None, None, None)
    with pytest.raises(KevlarInvalidCutoutDeflineError, match='chr7:1234'):
        ReferenceCutout('chr7:1234')
    with pytest.raises(KevlarDeflineSequenceLengthMismatchError, match='defline length: 10, sequence length: 4'):
        ReferenceCutout('chr7_1234-1244', 'ACGT')
    loaded = list(load_refr_cutouts(StringIO('>chr1_10-14 kvcc=3\nACGT\n>chr2_0-2\nAC\n')))
    assert [c.interval for c in loaded] == [('chr1', 10, 14), ('chr2', 0, 2)]
    assert loaded[0].defline == 'chr1_10-14 kvcc=3' and loaded[0].sequence == 'ACGT'


@pytest.fixture(scope='module')
def fiveparts():
    records = lc.read_fasta(lc.fixture('fiveparts-refr.fa.gz'))
    partitions = lc.partitions_of(lc.read_contigs(lc.fixture('fiveparts.contigs.augfasta.gz')))
    return records, partitions


def test_restatement_on_fiveparts(fiveparts):
    records, partitions = fiveparts
    contigs = [seq for pid, part in partitions for name, seq in part]
    assert len(lc.seeds_of(contigs, 51)) == 937
    assert len(lc.restated_matches(contigs, records, 51)) == 401
    targets = lc.restated_localize(partitions, records, 51)
    assert [pid for pid, defline, seq in targets] == ['1', '1', '2', '3', '4', '5']
    assert sorted(defline for pid, defline, seq in targets) == sorted([
        'seq1_284663-284950', 'seq1_1924681-1925049', 'seq1_1660589-1660884', 'seq1_2315741-2316037', 'seq1_2321099-2321322',
        'seq1_593102-593389'])


@pytest.fixture(scope='module')
def maxdiff_case():
    records = lc.read_fasta(lc.fixture('maxdiff-refr.fa.gz'))
    partitions = lc.partitions_of(lc.read_contigs(lc.fixture('maxdiff-contig.augfasta')))
    return records, partitions


def test_restatement_counts_on_maxdiff(maxdiff_case):
    records, partitions = maxdiff_case
    contigs = [seq for pid, part in partitions for name, seq in part]
    assert len(lc.seeds_of(contigs, 51)) == 143
    assert len(lc.restated_matches(contigs, records, 51)) == 945


@pytest.mark.parametrize('X,numtargets', [(100000, 1), (10000, 5), (1000, 33), (0, 1), (None, 33)])
def test_restatement_maxdiff(maxdiff_case, X, numtargets):
    records, partitions = maxdiff_case
    assert len(lc.restated_localize(partitions, records, 51, delta=50, maxdiff=X)) == numtargets


def test_restatement_matches_the_recorded_seed_dictionary(fiveparts):
    records, partitions = fiveparts
    seeds = ['ATCTGTTCTTGGCCAATAGAAAAAGCAAGGAGCCCTGAAAGACTCACAGTG', 'AAAAGGAAATGTTAACAACAAAATCACACAGATAAACCATCACAAGATCTG',
             'GATTCTAGGAGCTTGTTACTGCTGCTGAAAAAGGAAATGTTAACAACAAAA', 'AACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTTGGCCAATAGAA',
             'TTGTGTGTAAAAACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTT', 'AAGATACTATAATATGTTTCCCTGAGCACACCCCTTCGAAAGAGCAGAATT']
    assert lc.restated_matches(seeds, records, 51) == {
        ('AACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTTGGCCAATAGAA', 'seq1', 284819),
        ('AAGATACTATAATATGTTTCCCTGAGCACACCCCTTCGAAAGAGCAGAATT', 'seq1', 284722),
        ('ATCTGTTCTTGGCCAATAGAAAAAGCAAGGAGCCCTGAAAGACTCACAGTG', 'seq1', 284849),
        ('AAGAACAGATTATATATACTTCTGTGGACCTCTATTGGTTTTTACACACAA', 'seq1', 284808)}
    assert lc.restated_matches(seeds[1:3], records, 51) == set()


def test_cli_knows_localize_with_the_reference_s_defaults():
    args = kevlar_amd.cli.parser().parse_args(['localize', 'refr.fa', 'a.augfasta', 'b.augfasta'])
    assert (args.delta, args.part_id, args.out, args.seed_size, args.max_diff, args.include, args.exclude, args.max_occ) == \
        (50, None, '-', 51, None, None, None, 5000)
    assert (args.refr, args.contigs) == ('refr.fa', ['a.augfasta', 'b.augfasta'])
    args = kevlar_amd.cli.parser().parse_args(['localize', '-d', '7', '-p', '3', '-o', 'x.fa', '-z', '23', '-x', '0', '--include', 'chr',
                                               '--exclude', 'Un', '--max-occ', '9', 'refr.fa', 'a'])
    assert (args.delta, args.part_id, args.out, args.seed_size, args.max_diff, args.include, args.exclude, args.max_occ) == \
        (7, '3', 'x.fa', 23, 0, 'chr', 'Un', 9)
    assert kevlar_amd.cli.downstream_mains == {'localize': kevlar_amd.localize.main}
    assert 'localize' in kevlar_amd.cli.parser().format_help()
