"""`kevlar localize` on the device: the seed scan (kevlar_amd/csrc/kv_localize.hip) as sets of (seed, seqid, position) against the
plain-Python restatement of tests/localize_common.py -- never against itself -- and `localize()` / the command line against the
outputs the reference's kevlar/tests/test_localize.py records."""
import random

import numpy as np
import pytest

import kevlar_amd
from kevlar_amd.localize import Genome, SeedMatches, SeedSet, get_seed_matches, localize
from kevlar_amd.sequence import Record

import localize_common as lc

pytestmark = pytest.mark.gpu


def device_matches(contigs, records, z, max_occ=5000, **scan):
    """({(seed, seqid, position)}, number of (seed id, position) pairs the scan reported and max_occ kept, occurrences per seed)"""
    genome = Genome(records)
    with SeedSet(contigs, z) as seedset:
        matches = SeedMatches(seedset, genome, max_occ=max_occ, **scan)
        occurrences = {seedset.sequence(i): int(c) for i, c in enumerate(matches.counts) if c}
    return matches.triples(), int(matches.indptr[-1]), occurrences


def agree(contigs, records, z, max_occ=5000, **scan):
    """the device's matches equal the restatement's, none reported twice; returns them"""
    hits = lc.restated_hits(contigs, records, z)
    want = lc.capped(hits, max_occ)
    got, n_pairs, occurrences = device_matches(contigs, records, z, max_occ, **scan)
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    assert n_pairs == len(want)
    assert occurrences == {seed: len(where) for seed, where in hits.items()}      # counted before the cap
    return want


def partstream(partitions):
    return [(pid, [Record(name=name, sequence=seq) for name, seq in part]) for pid, part in partitions]


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------
FIVEPARTS = [lc.fixture('fiveparts-refr.fa.gz'), lc.fixture('fiveparts.contigs.augfasta.gz')]
PART2 = ('>seq1_1660589-1660884 kvcc=2\n'
         'GATAGATCTCCAAGAATTTTATACAGCAGGGCCCTGAGAATGAGCATGGAAGTGAATTTATTAGCCAGT'
         'GACAGTCACTTCACACTCTTCCTATATCAAAATTGAAGCCCAGGCTGGAGGTGGGCAGGGGTAGTACTT'
         'TTATGGACTGGACAGGGCGTAATCCCACCTGGGCGTGGGAGGAATATAAAAATAACCTTTAATTAATTC'
         'TGTCTGTAATTTATCTATGGGATGGGGTTGTTCAGAGAAGACTTCAATACCAGTTATTTAAGCCTGACC'
         'CTGGCTTGCCTTGACCCCA\n')


def fiveparts_stream(partid=None):
    contigs = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(FIVEPARTS[1], 'r'))
    return kevlar_amd.parse_single_partition(contigs, partid) if partid else kevlar_amd.parse_partitioned_reads(contigs)


def test_fiveparts_through_localize(hk, kevlar_log):
    targets = list(localize(fiveparts_stream(), FIVEPARTS[0], seedsize=51, debug=True))
    assert [partid for partid, gdna in targets] == ['1', '1', '2', '3', '4', '5']
    assert sorted(gdna.defline for partid, gdna in targets) == sorted([
        'seq1_284663-284950', 'seq1_1924681-1925049', 'seq1_1660589-1660884', 'seq1_2315741-2316037', 'seq1_2321099-2321322',
        'seq1_593102-593389'])
    assert all(len(gdna.sequence) == len(gdna) for partid, gdna in targets)
    log = kevlar_log.getvalue()
    for line in ('decomposing contigs into seeds of length 51', 'contigs decomposed into 936 seeds', 'computing seed matches',
                 'found positions for 401 seeds', 'loading reference sequences into memory',
                 'computing the reference target sequence for each partition'):
        assert line in log, line
    assert 'seeds written to' not in log and 'BWA' not in log


@pytest.mark.parametrize('partid,deflines', [('1', ['seq1_1924681-1925049', 'seq1_284663-284950']), ('4', ['seq1_2321099-2321322'])])
def test_fiveparts_single_partition(hk, partid, deflines):
    targets = list(localize(fiveparts_stream(partid), FIVEPARTS[0], seedsize=51))
    assert sorted(gdna.defline for pid, gdna in targets) == deflines
    assert {pid for pid, gdna in targets} == {partid}


def test_fiveparts_cli(hk, capsys, kevlar_log):          # (kevlar_log: run() redirects the log; the fixture puts it back)
    kevlar_amd.cli.run(['localize', '--part-id', '2'] + FIVEPARTS)
    out, err = capsys.readouterr()
    assert out == PART2
    kevlar_amd.localize.main(kevlar_amd.cli.parser().parse_args(['localize'] + FIVEPARTS))
    out, err = capsys.readouterr()
    assert len(out.strip().split('\n')) == 12


def test_fiveparts_cli_to_a_file(hk, tmp_path, kevlar_log):
    out = str(tmp_path / 'targets.fa')
    kevlar_amd.cli.run(['localize', '--part-id', '2', '-o', out] + FIVEPARTS)
    assert open(out).read() == PART2


def test_get_seed_matches(hk, tmp_path, kevlar_log):
    seeds = ['ATCTGTTCTTGGCCAATAGAAAAAGCAAGGAGCCCTGAAAGACTCACAGTG', 'AAAAGGAAATGTTAACAACAAAATCACACAGATAAACCATCACAAGATCTG',
             'GATTCTAGGAGCTTGTTACTGCTGCTGAAAAAGGAAATGTTAACAACAAAA', 'AACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTTGGCCAATAGAA',
             'TTGTGTGTAAAAACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTT', 'AAGATACTATAATATGTTTCCCTGAGCACACCCCTTCGAAAGAGCAGAATT']
    seedfile = str(tmp_path / 'seeds.fa')
    with open(seedfile, 'w') as stream:
        print(''.join('>seed{}\n{}\n'.format(n, seed) for n, seed in enumerate(seeds)), file=stream)
    assert get_seed_matches(seedfile, FIVEPARTS[0], seedsize=51) == {
        'AACCAATAGAGGTCCACAGAAGTATATATAATCTGTTCTTGGCCAATAGAA': {('seq1', 284819)},
        'AAGATACTATAATATGTTTCCCTGAGCACACCCCTTCGAAAGAGCAGAATT': {('seq1', 284722)},
        'ATCTGTTCTTGGCCAATAGAAAAAGCAAGGAGCCCTGAAAGACTCACAGTG': {('seq1', 284849)},
        'AAGAACAGATTATATATACTTCTGTGGACCTCTATTGGTTTTTACACACAA': {('seq1', 284808)}}
    assert 'found positions for 4 seeds' in kevlar_log.getvalue()
    with open(seedfile, 'w') as stream:
        print(''.join('>seed{}\n{}\n'.format(n, seed) for n, seed in enumerate(seeds[1:3])), file=stream)
    assert get_seed_matches(seedfile, FIVEPARTS[0], seedsize=51) == {}


@pytest.mark.parametrize('incl,excl,output', [(None, None, '>seq1_10-191'), (r'seq1', None, '>seq1_10-191'),
                                              (None, 'seq1', 'WARNING: no reference matches'),
                                              (r'chr[XY]', None, 'WARNING: no reference matches'), (None, r'b0Gu$', '>seq1_10-191')])
def test_main_include_exclude(hk, incl, excl, output, capsys, kevlar_log):
    arglist = ['localize', '--seed-size', '23', '--delta', '50', lc.fixture('localize-refr.fa'), lc.fixture('localize-contig.fa')]
    args = kevlar_amd.cli.parser().parse_args(arglist)
    args.include, args.exclude = incl, excl
    kevlar_amd.localize.main(args)
    out, err = capsys.readouterr()
    assert output in out or output in kevlar_log.getvalue()
    assert ('>' in out) == output.startswith('>')


def test_no_matches_warn_on_the_log(hk, capsys, kevlar_log):
    args = kevlar_amd.cli.parser().parse_args(['localize', '--seed-size', '23', lc.fixture('localize-refr.fa'),
                                               lc.fixture('localize-contig-bad.fa')])
    kevlar_amd.localize.main(args)
    out, err = capsys.readouterr()
    assert out == '' and kevlar_log.getvalue().count('WARNING: no reference matches') == 1
    contigs = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(lc.fixture('wasp-pass.contig.augfasta'), 'r'))
    assert list(localize(kevlar_amd.parse_partitioned_reads(contigs), FIVEPARTS[0], seedsize=41, debug=True)) == []
    assert kevlar_log.getvalue().count('WARNING: no reference matches') == 2


@pytest.mark.parametrize('X,numtargets', [(100000, 1), (10000, 5), (1000, 33), (0, 1), (None, 33)])
def test_maxdiff_fixture(hk, X, numtargets):
    contigs = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(lc.fixture('maxdiff-contig.augfasta'), 'r'))
    targets = list(localize(kevlar_amd.parse_partitioned_reads(contigs), lc.fixture('maxdiff-refr.fa.gz'), seedsize=51, delta=50,
                            maxdiff=X))
    assert len(targets) == numtargets


def test_fixture_matches_equal_the_restatement(hk):
    records = lc.read_fasta(FIVEPARTS[0])
    contigs = [seq for name, seq in lc.read_contigs(FIVEPARTS[1])]
    assert len(agree(contigs, records, 51)) == 401
    records = lc.read_fasta(lc.fixture('maxdiff-refr.fa.gz'))                 # holds a run of 100 N
    contigs = [seq for name, seq in lc.read_contigs(lc.fixture('maxdiff-contig.augfasta'))]
    assert len(agree(contigs, records, 51)) == 945


# ---- 2. key arithmetic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('z', [13, 23, 31, 32, 33, 51, 63, 64, 65, 96, 97, 127, 128])
def test_key_arithmetic(hk, z):
    records, seeds, palindromes, planted = lc.key_arithmetic_case(z)
    want = agree(seeds, records, z)
    matched = {seed for seed, seqid, pos in want}
    assert matched == set(planted) | set(palindromes)            # both strands of the planted ones, none of the near misses
    for palindrome in palindromes:
        assert sorted(pos for seed, seqid, pos in want if seed == palindrome) == [5000, 12345]


def test_seed_size_bounds(hk):
    for z in (0, 129):
        with pytest.raises(ValueError):
            SeedSet(['ACGT' * 40], z)
    assert agree(['ACGT'], [('s', 'AACGTT')], 1) == {('A', 's', 0), ('A', 's', 1), ('C', 's', 2), ('C', 's', 3), ('A', 's', 4),
                                                     ('A', 's', 5)}


# ---- 3. validity ----------------------------------------------------------------------------------------------------------
def test_validity_is_per_position(hk):
    rng = random.Random(3)
    z = 51
    a, b, c, d, e = (lc.random_dna(rng, n) for n in (300, 200, 400, 250, 300))
    genome = a + 'N' + b + 'N' * 100 + c.lower() + 'R' + d + 'y' + e[:150] + e[150:].lower()
    records = [('chr', genome)]
    at = {'before N': len(a) - z, 'after N': len(a) + 1, 'before Ns': len(a) + 1 + len(b) - z, 'after Ns': len(a) + 1 + len(b) + 100,
          'lower': len(a) + 1 + len(b) + 100 + 77, 'after R': len(a) + 1 + len(b) + 100 + len(c) + 1,
          'mixed case': len(genome) - 150 - 20}
    seeds = [genome[p:p + z].upper() for p in at.values()]
    # windows that overlap an N by one base, with the N read as each base: they must not match
    over_left = genome[len(a) - z + 1:len(a) + 1]               # ends on the N
    over_right = genome[len(a):len(a) + z]                       # starts on the N
    for base in 'ACGT':
        seeds += [over_left.replace('N', base), over_right.replace('N', base)]
    seeds.append(lc.rc(genome[at['lower']:at['lower'] + z].upper()))          # the other strand of a lower-case stretch
    seeds.append('acgt' * 13)                                                   # a lower-case contig window is a seed like any other
    seeds.append(genome[10:10 + z // 2] + 'N' + genome[10 + z // 2 + 1:10 + z])  # a contig window with N yields no seed
    want = agree(seeds, records, z)
    positions = {pos for seed, seqid, pos in want}
    assert positions == set(at.values())
    with SeedSet(seeds, z) as seedset:
        assert seedset.seed_of_window[-1] == 0xFFFFFFFF
        assert seedset.n_distinct == len(lc.seeds_of(seeds, z))
        assert (seedset.seed_of_window[:-1] != 0xFFFFFFFF).all()
    want = agree(['acgtacgtacgtaNcgtacgtaacgtacgtacgtatcgtacgtagg'], [('s', 'ACGTACGTACGTA'), ('t', 'cgtacgtaacgtac')], 13)
    assert {(seqid, pos) for seed, seqid, pos in want} >= {('s', 0), ('t', 0), ('t', 1)}


# ---- 4. sequence boundaries -------------------------------------------------------------------------------------------------
def test_sequence_boundaries(hk, tmp_path):
    rng = random.Random(4)
    z = 31
    seqs = [lc.random_dna(rng, n) for n in (500, 30, 0, 31, 700, 5, 90)]
    deflines = ['first some description', 'short', 'empty', 'exact\ttabbed', 'fifth x=1', 'tiny', 'last']
    ids = ['first', 'short', 'empty', 'exact', 'fifth', 'tiny', 'last']
    records = list(zip(ids, seqs))
    seeds = [seqs[0][:z], seqs[0][-z:], seqs[3], lc.rc(seqs[4][:z]), seqs[4][-z:], seqs[6][:z], seqs[6][-z:]]
    seeds.append(seqs[0][-15:] + seqs[1][:16])                   # exists only across a junction
    seeds.append(seqs[3][-20:] + seqs[4][:11])
    seeds.append(seqs[0][-15:] + '>' + seqs[1][:15])             # ... or with the separator byte itself
    want = agree(seeds, records, z)
    assert {(seqid, pos) for seed, seqid, pos in want} == {('first', 0), ('first', 500 - z), ('exact', 0), ('fifth', 0),
                                                           ('fifth', 700 - z), ('last', 0), ('last', 90 - z)}
    fasta = str(tmp_path / 'refr.fa')
    with open(fasta, 'w') as stream:
        for defline, seq in zip(deflines, seqs):
            stream.write('>{}\n'.format(defline))
            for i in range(0, len(seq), 60):
                stream.write(seq[i:i + 60] + '\n')
    genome = Genome.from_file(fasta)
    assert genome.ids == ids and genome.seqs == seqs
    with SeedSet(seeds, z) as seedset:
        assert SeedMatches(seedset, genome).triples() == want


# ---- 5. chunk and run edges ---------------------------------------------------------------------------------------------------
CHUNK_Z = 23


@pytest.fixture(scope='module')
def chunk_case():
    z = CHUNK_Z
    records, seeds, positions = lc.chunk_edge_case(z, (z, z + 1, 4096, 4097))
    return records, seeds, positions, lc.restated_matches(seeds, records, z)


@pytest.mark.parametrize('chunk', ['Z', 'Z+1', 4096, 4097, 'whole'])
def test_chunk_and_run_edges(hk, chunk_case, chunk):
    z = CHUNK_Z
    records, seeds, positions, want = chunk_case
    assert {pos for seed, seqid, pos in want} >= set(positions)
    chunk_bytes = {'Z': z, 'Z+1': z + 1, 'whole': 1 << 20}.get(chunk, chunk)
    genome = Genome(records)
    with SeedSet(seeds, z) as seedset:
        ids, pos = seedset.scan(genome.text, chunk_bytes=chunk_bytes)
        pairs = sorted(zip(ids.tolist(), pos.tolist()))
        assert len(pairs) == len(set(pairs)) == len(want)        # each window exactly once
        assert {(seedset.sequence(i), 'chr', p) for i, p in pairs} == want
        assert int(seedset.counts().sum()) == len(want)


# ---- 6. repeats and the cap ---------------------------------------------------------------------------------------------------
def test_repeats(hk):
    z = 51
    want = agree(['A' * z], [('polyA', 'A' * 5000), ('polyT', 't' * 100)], z, chunk_bytes=700)
    assert len(want) == 5000 - z + 1 + 100 - z + 1
    want = agree(['ACG' * 17, 'T' * z], [('tandem', 'ACG' * 1000 + 'CGT' * 500)], z, chunk_bytes=1000)
    assert len(want) == 984 + 484                                # every third window, both strands
    assert agree(['ACG' * 17], [('polyA', 'A' * 5000 + 'ACG' * 40)], z, max_occ=5) == set()      # 24 occurrences


def test_the_cap_counts_across_chunks(hk):
    rng = random.Random(6)
    z = 51
    five, six = lc.random_dna(rng, z), lc.random_dna(rng, z)
    parts = []
    for n in range(6):
        parts += [lc.random_dna(rng, 900), five if n < 5 else lc.random_dna(rng, z), lc.random_dna(rng, 333),
                  lc.rc(six) if n % 2 else six]
    records = [('one', ''.join(parts[:10])), ('two', ''.join(parts[10:]))]
    for chunk_bytes in (1 << 20, 1500, 257):
        want = agree([five, six], records, z, max_occ=5, chunk_bytes=chunk_bytes)
        assert {seed for seed, seqid, pos in want} == {lc.minseq(five)} and len(want) == 5
        assert len(agree([five, six], records, z, max_occ=6, chunk_bytes=chunk_bytes)) == 11
        assert len(agree([five, six], records, z, max_occ=None, chunk_bytes=chunk_bytes)) == 11


# ---- 7. output overflow ---------------------------------------------------------------------------------------------------------
def test_output_overflow_repeats_the_chunk_without_counting_twice(hk):
    rng = random.Random(7)
    z = 51
    text = lc.random_dna(rng, 60000)
    records = [('chr', text)]
    contigs = [text[20000:30000 + z - 1]]                        # 10 000 windows, each in the genome
    want = lc.restated_matches(contigs, records, z)
    assert len(want) >= 10000
    genome = Genome(records)
    results = {}
    for name, scan in (('ample', dict(capacity=1 << 16)), ('tight', dict(capacity=64)),
                       ('tight chunks', dict(capacity=64, chunk_bytes=7000))):
        with SeedSet(contigs, z) as seedset:
            ids, pos = seedset.scan(genome.text, **scan)
            pairs = sorted(zip(ids.tolist(), pos.tolist()))
            assert len(pairs) == len(set(pairs)) == len(want), name
            assert {(seedset.sequence(i), 'chr', p) for i, p in pairs} == want, name
            counts = seedset.counts()
            results[name] = {seedset.sequence(i): int(c) for i, c in enumerate(counts) if c}
            assert int(counts.sum()) == len(want), name
            assert seedset.stats()[2] == len(want), name
    assert results['tight'] == results['ample'] == results['tight chunks']


# ---- 8. scale of the table --------------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_seeds(hk):
    rng = np.random.default_rng(8)
    z, n_seeds, n_planted = 51, 200000, 10000
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    text = letters[rng.integers(0, 4, size=2000000)].tobytes().decode()
    starts = rng.choice(2000000 - z, size=n_planted, replace=False)
    seeds = [text[s:s + z] if n % 2 else lc.rc(text[s:s + z]) for n, s in enumerate(starts.tolist())]
    blob = letters[rng.integers(0, 4, size=(n_seeds - n_planted) * z)].tobytes().decode()
    seeds += [blob[i:i + z] for i in range(0, len(blob), z)]
    want = agree(seeds, [('chr', text)], z)
    assert len(want) >= n_planted


# ---- 9. Localizer agreement -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def partition_case(tmp_path_factory):
    records, deflined, partitions = lc.partition_case()
    fasta = str(tmp_path_factory.mktemp('localize') / 'refr.fa')
    with open(fasta, 'w') as stream:
        for defline, seq in deflined:
            stream.write('>{}\n'.format(defline))
            for i in range(0, len(seq), 80):
                stream.write(seq[i:i + 80] + '\n')
    hits = lc.restated_hits([seq for pid, part in partitions for name, seq in part], records, 51)
    return records, partitions, fasta, hits


@pytest.mark.parametrize('delta,maxdiff,excl', [(0, None, None), (50, None, None), (50, 0, None), (50, 500, None),
                                                (50, None, 'scaffold'), (0, 500, r'^chrB$')])
def test_localize_equals_the_restatement(hk, partition_case, delta, maxdiff, excl):
    records, partitions, fasta, hits = partition_case
    want = lc.restated_localize(partitions, records, 51, delta=delta, maxdiff=maxdiff, excl=excl, hits=hits)
    assert len(want) >= 15
    got = [(partid, gdna.defline, gdna.sequence)
           for partid, gdna in localize(partstream(partitions), fasta, seedsize=51, delta=delta, maxdiff=maxdiff, exclpattern=excl,
                                        chunk_bytes=300001)]
    assert got == want
