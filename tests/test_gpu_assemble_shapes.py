"""kv_assemble.hip where random DNA does not take it: repeats, hairpins, rings and unitigs equal to their own reverse complement
(ac.structured_partition; tests/test_assemble_reference.py holds the restatement to the rule on the same inputs and states their
census), the same graph in many partitions of one call, more windows, runs and heads than one grid of 4096 x 256 covers, reads
and partitions that end on the edges of a run, a wave and a chunk, and a planned launch without a window.  Every case compares the
full unitig set of every partition and the six stats with the restatement (ac.agree): strings and integers, equal or not."""
import random

import pytest

from kevlar_amd import assemble as asm

import assemble_common as ac

pytestmark = pytest.mark.gpu
ONE_GRID = 4096 * ac.THREADS                        # ASM_MAX_GRID workgroups of ASM_THREADS: 1 048 576


def both(cases):
    """(partitions, the restatement's answers) of structured_answers rows"""
    return [reads for _, reads, _, _ in cases], [(found, stats) for _, _, found, stats in cases]


# ---- 1. the structured fuzz: 600 partitions a call ------------------------------------------------------------------------------
@pytest.mark.parametrize('min_count', [1, 2, 3])
@pytest.mark.parametrize('K', [13, 15, 31, 33, 63])
def test_structured_fuzz(hk, K, min_count):
    parts, want = both(ac.structured_answers(K, min_count))
    assert len(parts) == 600
    found, stats = ac.agree(parts, K, min_count, launches=1, want=want)
    assert stats['unitigs'] > 0


@pytest.mark.parametrize('K', [33, 61, 63])
def test_hairpins_and_own_reverse_complements_in_two_words(hk, K):
    # (a read of the fuzz has at most 69 bases: none of its unitigs is its own reverse complement at K = 63)
    rng = random.Random(K)
    parts = []
    for loop in (0, 1, 2, 3):
        stem = ac.random_dna(rng, 70 + loop)
        seq = ac.random_dna(rng, 40) + stem + ac.random_dna(rng, loop) + ac.rc(stem) + ac.random_dna(rng, 40)
        parts.append(ac.tiled_reads(seq, 100, 3, copies=2))
        own = stem + ac.rc(stem)
        parts.append([own, own, own[:90]])
        parts.append(ac.tiled_reads(stem[:35] * 2 + own + ac.random_dna(rng, 30), 90, 5, copies=2))
    want = [ac.unitigs(reads, K, 2) for reads in parts]
    for reads, (found, stats) in zip(parts, want):
        ac.check_unitigs(reads, K, 2, found, stats)
    assert sum(1 for found, _ in want for u in found if u == ac.rc(u)) >= 8
    ac.agree(parts, K, 2, want=want)


# ---- 2. the same graph in many partitions of one call ----------------------------------------------------------------------------
def near_copy(rng, reads):
    """the reads with one left out and one base of another replaced by A or C: most K-mers stay"""
    reads = list(reads)
    del reads[rng.randrange(len(reads))]
    r = rng.randrange(len(reads))
    at = rng.randrange(len(reads[r]))
    reads[r] = reads[r][:at] + ('C' if reads[r][at] == 'A' else 'A') + reads[r][at + 1:]
    return reads


@pytest.mark.parametrize('K,min_count', [(13, 1), (13, 2), (15, 2), (33, 1), (33, 2)])
def test_same_shapes_beside_each_other(hk, K, min_count):
    # Equal keys in many partitions of one table: a match must be (partition, key).  A partition five times, its reads
    # reverse-complemented twice, and four near copies in between; the first of them an alpha2 partition, whose near copies are
    # alpha2 partitions too.  Every partition is held to the restatement, which gives equal partitions equal answers.
    rng = random.Random(1000 * K + min_count)
    parts, same, near = [], [], []
    for first in range(len(ac.KINDS)):              # one of every kind, of reads long enough to hold some windows
        seed = next(s for s in range(first, 600, len(ac.KINDS)) if len(ac.structured_partition(s)[1][0]) >= K + 12)
        kind, base = ac.structured_partition(seed)
        at = len(parts)
        for what in 'base other near base near other base near base near base'.split():
            (near if what == 'near' else same).append((at, len(parts)))
            parts.append(list(base) if what == 'base' else [ac.rc(read) for read in base] if what == 'other' else near_copy(rng, base))
    assert len(parts) == 66 and len(same) == 42
    found, stats = ac.agree(parts, K, min_count, launches=1)
    assert all(found[p] == found[at] for at, p in same)                 # (the strand of a read says nothing)
    assert any(found[at] for at, p in same) and any(found[p] != found[at] for at, p in near)


# ---- 3. more windows, runs and heads than one grid covers --------------------------------------------------------------------------
def test_more_than_one_grid_of_windows_runs_and_heads(hk):
    K, min_count, repeats = 13, 1, 110
    rng = random.Random(4096)
    distinct = [ac.structured_partition(seed)[1] for seed in range(20)]
    distinct += [[ac.random_dna(rng, K) for _ in range(500)] for _ in range(20)]       # a window and a run a read; isolated nodes
    answers = [ac.unitigs(reads, K, min_count) for reads in distinct]
    runs_of = [sum((max(len(r) - K + 1, 0) + ac.RUN - 1) // ac.RUN for r in reads) for reads in distinct]
    assert all(stats['heads'] >= 2 * 495 and stats['unitigs'] >= 495 for _, stats in answers[20:])
    order = list(range(len(distinct))) * repeats
    rng.shuffle(order)
    parts, want = [distinct[i] for i in order], [answers[i] for i in order]
    total = ac.add_stats([stats for _, stats in want])
    runs = sum(runs_of[i] for i in order)
    # every grid-stride loop goes round again: windows (group, degree; heads and compact by chunks), runs (keys), heads (both walks),
    # and the prefix sum over the chunks' head counts has more than 4096 of them
    assert total['windows'] > ONE_GRID and runs > ONE_GRID and total['heads'] > ONE_GRID
    sizes = [ac.partition_size([len(r) for r in reads], K) for reads in distinct]
    planned = [sum(sizes[i][j] for i in order) for j in range(3)]       # (windows with an N in them too)
    assert planned[0] >= total['windows'] and ac.launch_bytes(planned[0], planned[1], planned[2], K) < 1 << 30
    ac.agree(parts, K, min_count, launches=1, want=want)


# ---- 4. the edges of a run, a wave and a chunk -------------------------------------------------------------------------------------
WINDOW_COUNTS = (31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize('K', [31, 33])
def test_reads_that_end_on_a_run_and_an_n_at_every_run_edge(hk, K):
    assert ac.RUN == 32 and ac.THREADS == 256
    rng = random.Random(K)
    reads = [ac.random_dna(rng, n + K - 1) for n in WINDOW_COUNTS]
    assert [len(r) - K + 1 for r in reads] == list(WINDOW_COUNTS)
    parts = [[read] for read in reads] + [reads, reads + reads[::-1]]
    ac.agree(parts, K, 1)
    ac.agree(parts, K, 2)
    # one N; the windows over base p are p - K + 1 .. p, so the last invalid window is p: the last of a run, the first of the next,
    # and K - 2 and K - 1 windows on, where the N is the last base the next run reads before its first window, and the first after
    with_n = []
    for read in reads:
        for edge in range(ac.RUN, len(read) - K + 2, ac.RUN):
            for p in (edge - 1, edge, edge + K - 2, edge + K - 1):
                if p < len(read):
                    with_n.append([read[:p] + 'N' + read[p + 1:]])
    assert len(with_n) > 80
    found, stats = ac.agree(with_n, K, 1)
    assert all(len(u) <= 2 for u in found) and sum(1 for u in found if len(u) == 2) > 40      # what is left on either side of the N
    ac.agree([part * 2 for part in with_n] + [[part[0] for part in with_n]], K, 2)


def two_reads_of(rng, K, windows):
    """a partition of `windows` windows: two overlapping reads of one random sequence"""
    a = windows // 2 + 3
    seq = ac.random_dna(rng, windows + K)
    reads = [seq[:a + K - 1], seq[9:9 + (windows - a) + K - 1]]
    assert sum(len(r) - K + 1 for r in reads) == windows
    return reads


@pytest.mark.parametrize('K', [31, 33])
def test_partition_bounds_around_a_chunk(hk, K):
    rng = random.Random(2 * K)
    # separately: the second partition starts at window 255, 256, 257, 511, 512, 513
    for windows in (255, 256, 257, 511, 512, 513):
        ac.agree([two_reads_of(rng, K, windows), ac.seeded_partition(windows, 8, 70, 150)], K, 1)
    # and in one call: bounds at 255, 512, 769, 1024, 1279 and 1537
    parts = [two_reads_of(rng, K, n) for n in (255, 257, 257, 255, 255, 258, 100)]
    ac.agree(parts, K, 1)
    ac.agree([reads * 2 for reads in parts], K, 2)


@pytest.mark.parametrize('K', [31, 33])
def test_isolated_nodes_at_the_end_of_a_wave_and_of_a_chunk(hk, K):
    # a read of K bases alone in its partition is a node without an edge: both its strands are heads, and the lane writes two
    # entries of the head list, the second behind the first: windows 63 | 64 are the last and first lane of two waves,
    # 255 | 256 those of two chunks
    rng = random.Random(3 * K)
    for filler in ('path', 'none'):                 # with heads in front (a path has two) and with none (63 windows over N)
        def fill(n):
            return [ac.random_dna(rng, n + K - 1) if filler == 'path' else 'N' * (n + K - 1)]
        parts = [fill(63), [ac.random_dna(rng, K)], [ac.random_dna(rng, K)], fill(190), [ac.random_dna(rng, K)], [ac.random_dna(rng, K)], fill(40)]
        first = [sum(max(len(r) - K + 1, 0) for reads in parts[:p] for r in reads) for p in range(len(parts))]
        assert [first[p] for p in (1, 2, 4, 5)] == [63, 64, 255, 256]
        found, stats = ac.agree(parts, K, 1)
        assert [len(found[p]) for p in (1, 2, 4, 5)] == [1, 1, 1, 1]
        assert stats['heads'] == (14 if filler == 'path' else 8)


# ---- 5. a planned launch without a window ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [31, 33])
def test_a_planned_launch_that_holds_no_window(hk, K):
    big = ac.seeded_partition(50 + K, 20, 100, 260)
    small = ac.seeded_partition(60 + K, 6, 60, 120)
    short = ['ACGT' * 5, 'ACGTTGCA' * 3 + 'ACGTTG']                     # 20 and 30 bases: no window at K >= 31
    assert max(len(r) for r in short) == 30 < K
    parts = [big, short, [], [r.lower() for r in short], list(big), small]
    lengths = [[len(r) for r in reads] for reads in parts]
    budget = ac.launch_bytes(*ac.partition_size(lengths[0], K), K)      # what the largest partition needs alone
    ends = ac.plan(lengths, K, budget)
    assert ends == [1, 4, 5, 6]                     # big | three partitions without a window | big | small
    holds = [sum(ac.partition_size(ls, K)[0] for ls in lengths[a:b]) > 0 for a, b in zip([0] + ends, ends)]
    assert holds == [True, False, True, True]
    assert ac.device_plan(parts, K, budget) == (0, ends)                # KV_OK, and every planned launch, the empty one too
    whole, _ = ac.agree(parts, K, 2, launches=1)
    ac.agree(parts, K, 2, mem_budget=budget, launches=sum(holds))       # a planned launch without a window is not launched
    assert whole[0] and whole[0] == whole[4] and whole[1] == whole[2] == whole[3] == []
    at_once, in_four = asm.unitigs_batch(parts, K, 2)[0], asm.unitigs_batch(parts, K, 2, budget)[0]
    assert [sorted(u) for u in at_once] == [sorted(u) for u in in_four] == whole
    # nothing but such partitions: no launch at all
    found, stats = ac.agree([short, [], short], K, 2, launches=0)
    assert found == [[], [], []]
