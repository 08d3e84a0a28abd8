"""Contig-to-cutout alignment on the device (kevlar_amd/csrc/kv_align.hip through kevlar_amd.alignment): scores and CIGAR strings
against the plain-Python restatement of tests/align_common.py or against what the reference's compiled align() returned
(tests/golden/align/recorded.json) -- never against itself.  Every job of every batch is compared."""
import pytest

import kevlar_amd
from kevlar_amd import alignment
from kevlar_amd.sequence import Record

import align_common as ac
import localize_common as lc

pytestmark = pytest.mark.gpu
W = ac.ALIGN_STRIP


@pytest.fixture(scope='module', autouse=True)
def device(hk):
    assert alignment.ALIGN_STRIP == W
    return hk


@pytest.fixture(scope='module')
def records():
    return ac.recorded()


def agree_with_restatement(pairs, scorings=ac.SCORINGS, **kwargs):
    """one forward-strand batch per scoring over all (target, query) pairs; every job against the restatement"""
    targets = [t for t, q in pairs]
    queries = [q for t, q in pairs]
    index = [(k, k) for k in range(len(pairs))]
    for scoring in scorings:
        got = alignment.align_batch(targets, queries, index, *scoring, both_strands=False, **kwargs)
        assert len(got) == len(pairs)
        for k, (target, query) in enumerate(pairs):
            cigar, score = ac.restated_align(target, query, *scoring)
            assert got[k] == (score, cigar), (k, scoring, target, query)


# ---- 1. the reference's fixtures and records --------------------------------------------------------------------------------
def test_the_pair_of_the_reference_test_align():
    assert kevlar_amd.align(ac.LITERAL_TARGET, ac.LITERAL_QUERY) == ac.LITERAL_RESULT
    assert alignment.contig_align(ac.LITERAL_TARGET, ac.LITERAL_QUERY) == ac.LITERAL_RESULT


def test_fixture_pairs_both_strands_four_scorings(records):
    pairs = ac.fixture_pairs()
    targets = [t for key, t, q in pairs]
    queries = [q for key, t, q in pairs]
    revcoms = [ac.rc(q) for q in queries]
    index = [(k, k) for k in range(len(pairs))]
    for scoring in ac.SCORINGS:
        # the forward strand, the reverse strand uploaded as its own sequence, and both through the device's reversal
        forward = alignment.align_batch(targets, queries, index, *scoring, both_strands=False)
        reverse = alignment.align_batch(targets, revcoms, index, *scoring, both_strands=False)
        both = alignment.align_batch(targets, queries, index, *scoring)
        for k, (key, target, query) in enumerate(pairs):
            cigar1, score1 = records['pairs'][ac.record_key(key, 1, scoring)]
            cigar2, score2 = records['pairs'][ac.record_key(key, -1, scoring)]
            assert forward[k] == (score1, cigar1), (key, scoring)
            assert reverse[k] == (score2, cigar2), (key, scoring)
            assert both[k] == ((score2, cigar2, -1) if score2 > score1 else (score1, cigar1, 1)), (key, scoring)


def test_align_both_strands_takes_records(records):
    strands = set()
    for key, target, query in ac.fixture_pairs():
        cigar1, score1 = records['pairs'][ac.record_key(key, 1, ac.SCORINGS[0])]
        cigar2, score2 = records['pairs'][ac.record_key(key, -1, ac.SCORINGS[0])]
        want = (score2, cigar2, -1) if score2 > score1 else (score1, cigar1, 1)
        assert alignment.align_both_strands(Record(name='t', sequence=target), Record(name='q', sequence=query)) == want, key
        strands.add(want[2])
    assert strands == {1, -1}
    winners = {key.split(':')[0]: [] for key, t, q in ac.fixture_pairs()}
    for key, target, query in ac.fixture_pairs():
        winners[key.split(':')[0]].append(alignment.align_batch([target], [query], [(0, 0)])[0][1])
    for name, cigar in records['test_call'].items():
        assert cigar in winners[name]


def test_a_tie_between_the_strands_keeps_the_forward_one():
    half = 'ACGGTCATTGCA'
    query = half + ac.rc(half)
    assert ac.rc(query) == query
    target = 'TTGA' + query + 'GGC'
    want = ac.restated_both_strands(target, query)
    assert want[2] == 1
    assert alignment.align_batch([target], [query], [(0, 0)]) == [want]
    (s1, c1), = alignment.align_batch([target], [query], [(0, 0)], both_strands=False)
    assert (s1, c1, 1) == want


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------
def test_shape_edges_of_the_strip():
    cases = ac.shape_edge_pairs()
    lengths = {(len(t), len(q)) for label, t, q in cases}
    assert {(1, 1), (1, 2 * W + 1), (2 * W + 1, 1), (2, W), (W - 1, 2), (W + 1, 2), (2, W + 1)} <= lengths
    assert all(len(t) * len(q) < 40000 for label, t, q in cases)
    agree_with_restatement([(t, q) for label, t, q in cases])


def test_fuzz_300_pairs_four_scorings():
    pairs = ac.fuzz_pairs(300)
    assert len(pairs) == 300 and all(1 <= len(t) <= 150 and 1 <= len(q) <= 150 for t, q in pairs)
    agree_with_restatement(pairs)


# ---- 3. batches ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mixed():
    """1-cell jobs around a 1 500 x 600 job, a few small ones between: (targets, queries, pairs, expected)"""
    import random
    rng = random.Random(99)
    big_t = ac.random_dna(rng, 1500)
    big_q = ac.edited(rng, big_t[400:1000], 8)[:600]
    targets = ['A', 'C', big_t, 'G', ac.random_dna(rng, 70), 'N', ac.random_dna(rng, W + 3)]
    queries = ['A', big_q, 'T', ac.random_dna(rng, 33), 'a', ac.random_dna(rng, 2 * W + 5)]
    # the five (6, 5) jobs together need more direction bytes than the big one: a budget of the big job's size makes three launches
    pairs = [(0, 0), (1, 2), (6, 5), (2, 1), (3, 0), (0, 4), (6, 5), (4, 3), (5, 0), (1, 0), (6, 5), (6, 3), (4, 5), (6, 5), (3, 2), (0, 2),
             (6, 5)]
    known = {}
    for t, q in pairs:
        if (t, q) not in known:
            cigar, score = ac.restated_align(targets[t], queries[q])
            known[(t, q)] = (score, cigar)
    return targets, queries, pairs, [known[pair] for pair in pairs]


def test_mixed_batch(mixed):
    targets, queries, pairs, expected = mixed
    assert alignment.align_batch(targets, queries, pairs, both_strands=False) == expected
    assert alignment.last_stats()[0] == 1
    assert alignment.last_stats()[3] == sum(len(targets[t]) * len(queries[q]) for t, q in pairs)


def test_a_small_z_budget_cuts_the_batch_into_launches(mixed):
    targets, queries, pairs, expected = mixed
    budget = alignment.z_bytes(1500, len(queries[1]))
    assert alignment.align_batch(targets, queries, pairs, both_strands=False, z_budget=budget) == expected
    assert alignment.last_stats()[0] >= 3
    assert 5 * alignment.z_bytes(W + 3, 2 * W + 5) > budget
    with pytest.raises(ValueError):
        alignment.align_batch(targets, queries, pairs, both_strands=False, z_budget=budget - 1)


def test_a_run_pool_of_one_is_repeated_with_room(mixed):
    targets, queries, pairs, expected = mixed
    assert alignment.align_batch(targets, queries, pairs, both_strands=False, run_capacity=1) == expected


# ---- 4. the large recorded pairs ---------------------------------------------------------------------------------------------
def test_large_recorded_pairs(records):
    """30 M direction bytes per job, about 50 strips between them; expected values from the reference's align()"""
    seqs = {kind: ac.large_pair(kind, seed) for kind, seed in ac.LARGE}
    targets = [seqs[kind][0] for kind, seed in ac.LARGE]
    queries = [seqs[kind][1] for kind, seed in ac.LARGE]
    revcoms = [ac.rc(q) for q in queries]
    by = {(r['kind'], r['strand']): (r['score'], r['cigar']) for r in records['large']}
    forward = alignment.align_batch(targets, queries, [(0, 0), (1, 1)], both_strands=False)
    reverse = alignment.align_batch(targets, revcoms, [(0, 0), (1, 1)], both_strands=False)
    both = alignment.align_batch(targets, queries, [(0, 0), (1, 1)])
    for k, (kind, seed) in enumerate(ac.LARGE):
        assert forward[k] == by[(kind, 1)], kind
        assert reverse[k] == by[(kind, -1)], kind
        assert by[(kind, 1)][0] > by[(kind, -1)][0]
        assert both[k] == by[(kind, 1)] + (1,), kind
    # the reverse strand as the winner: the same pairs with the reverse complement uploaded
    assert alignment.align_batch(targets, revcoms, [(0, 0)]) == [by[('deletion', 1)] + (-1,)]


# ---- 5. partition streams -----------------------------------------------------------------------------------------------------
def test_align_partitions_on_fiveparts(kevlar_log):
    from kevlar_amd.localize import localize
    refr, contigfile = lc.fixture('fiveparts-refr.fa.gz'), lc.fixture('fiveparts.contigs.augfasta.gz')

    def partstream():
        return kevlar_amd.parse_partitioned_reads(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(contigfile, 'r')))

    cutouts = {}
    for partid, gdna in localize(partstream(), refr, seedsize=51):
        cutouts.setdefault(partid, []).append(gdna)
    assert sorted(cutouts) == ['1', '2', '3', '4', '5'] and len(cutouts['1']) == 2
    contigs = list(partstream())
    got = list(alignment.align_partitions(contigs, cutouts))
    assert [partid for partid, contig, cutout, score, cigar, strand in got] == ['1', '1', '2', '3', '4', '5']
    for partid, part in contigs:
        mine = [(contig.name, cutout.defline) for p, contig, cutout, score, cigar, strand in got if p == partid]
        assert mine == [(contig.name, cutout.defline) for contig in sorted(part, reverse=True, key=len)
                        for cutout in sorted(cutouts[partid], key=lambda c: c.defline)]
    for partid, contig, cutout, score, cigar, strand in got:
        assert (score, cigar, strand) == ac.restated_both_strands(cutout.sequence, contig.sequence), (partid, cutout.defline)
    # a limit below every cutout: nothing is aligned
    assert [(score, cigar, strand) for p, c, t, score, cigar, strand in alignment.align_partitions(contigs, cutouts, maxtargetlen=10)] \
        == [(0, None, 1)] * len(got)
