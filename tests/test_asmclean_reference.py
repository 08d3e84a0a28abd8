"""The cleaning rule of `kevlar assemble --clean` without a GPU: the restatement in tests/asmclean_common.py against today's
restatement at limits 0, 0, against the fixtures under tests/golden/assemble (every one keeps its contigs but pico-var/cc2, whose
two contigs become one that holds the recorded ALT), against hand-built graphs whose answer is written out, against itself under
shuffling, strand and partition order, the census of the planted generator (asserted, not measured), the cleaning-aware planner of
kevlar_amd/csrc/kv_asm_plan.h through tests/harness/asm_clean_plan_host.cpp, and the new flags of the two parsers."""
import ctypes
import os
import random
import subprocess

import pytest

import assemble_common as ac
import asmclean_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kevlar_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'harness', 'asm_clean_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libasm_clean_plan_host.so')
HEADERS = [os.path.join(CSRC, name) for name in ('kv_require.h', 'kv_asm_plan.h')]
KV_OK, KV_ERR_ARG, KV_ERR_CAPACITY = 0, -1, -6
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
READ_FIXTURES = sorted(name for name in ac.recorded()['files']
                       if name.endswith(('.afq.gz', '.augfastq.gz', '.augfastq', '.fq.gz')) and name != 'pico-var/cc2.afq.gz')
CC2_CONTIG = 337            # as the restatement gives it: tips of at most 31 nodes, min_count 2, one round


def numbers(clean):
    return tuple(clean[name] for name in cc.CLEAN_NAMES)


# ---- limits 0, 0: today's answer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [13, 31])
def test_no_limits_is_todays_restatement_on_the_structured_fuzz(K):
    for kind, reads, found, stats in ac.structured_answers(K, 2):
        assert cc.clean_unitigs(reads, K, 2, 0, 0) == (found, stats, dict.fromkeys(cc.CLEAN_NAMES, 0))


@pytest.mark.parametrize('name', READ_FIXTURES + ['pico-var/cc2.afq.gz'])
def test_fixtures_without_and_with_cleaning(name):
    assert len(READ_FIXTURES) == 22
    for partid, reads in ac.read_partitions(name):
        today = ac.unitigs(reads)
        assert cc.clean_unitigs(reads, 31, 2, 0, 0)[:2] == today
        cleaned, stats, clean = cc.clean_unitigs(reads, 31, 2, *cc.clean_limits(31))
        assert stats['solid'] == today[1]['solid'] and stats['windows'] == today[1]['windows']
        if name != 'pico-var/cc2.afq.gz':               # the contigs it gives today: six of none, cc231's none, fiveparts 1-5, ...
            assert ac.contigs_of(cleaned, reads) == ac.contigs_of(today[0], reads), (name, partid)
            continue
        # three tips (34 keys) go in one round and the two contigs on either side of the insertion join
        assert [len(c) for c in ac.contigs_of(today[0], reads)] == [165, 162]
        assert numbers(clean) == (3, 34, 0, 0, 1)
        contigs = ac.contigs_of(cleaned, reads)
        assert [len(c) for c in contigs] == [CC2_CONTIG]
        row = [r for r in ac.recorded()['pico_calls'] if r['cc'] == 2][0]
        assert len(row['alt']) == 161
        assert row['alt'] not in contigs[0] and ac.rc(contigs[0]).find(row['alt']) == 80           # 80 bases of flank in front of it
        # the third tip has 23 nodes: with tips of at most 15 two go (11 keys), one contig grows and the two do not join, so the
        # default has to be about K
        short = cc.clean_unitigs(reads, 31, 2, 15, 62)
        assert numbers(short[2]) == (2, 11, 0, 0, 1) and [len(c) for c in ac.contigs_of(short[0], reads)] == [202, 165]


# ---- hand-built cases, the answer written out --------------------------------------------------------------------------------------
HAND_NAMES = ('snp', 'tie_id', 'indel', 'tie_length', 'three', 'two_on_one', 'two_on_two', 'tip', 'tip_on_arm', 'hairpin', 'arm_at_limit',
              'arm_beyond_limit', 'tip_at_limit', 'tip_beyond_limit', 'fork_two_tips', 'edge_beside_arm', 'ring_with_tip')


@pytest.mark.parametrize('K', [13, 31])
@pytest.mark.parametrize('name', HAND_NAMES)
def test_hand_built(name, K):
    cases = cc.hand_cases(K)
    assert tuple(cases) == HAND_NAMES
    reads, want, clean = cases[name]
    today = ac.unitigs(reads, K, 2)
    events = {}
    found, stats, got = cc.clean_unitigs(reads, K, 2, K, 2 * K, events=events)
    assert found == (today[0] if want is None else sorted(want))
    assert numbers(got) == clean
    assert stats['solid'] == today[1]['solid']                          # solid before cleaning
    live = stats['solid'] - got['tip_keys'] - got['arm_keys']
    assert stats['cycle_keys'] == (live if name == 'ring_with_tip' else 0)
    if want is None:
        assert (found, stats) == today and len(found) >= 3              # the graph has forks, and nothing goes
    if name == 'ring_with_tip':
        assert today[1]['cycle_keys'] == 0 and stats['cycle_keys'] == K + 7 and stats['heads'] == 0     # the ring, whole
    assert (events['three_arms'] > 0) == (name == 'three')
    assert (events['mean_tie'] > 0) == (name in ('tie_id', 'tie_length'))
    assert (events['hairpin_self'] > 0) == (name == 'hairpin')


@pytest.mark.parametrize('K', [13, 31])
def test_one_round_against_two_on_the_tip_on_an_arm(K):
    reads, want, clean = cc.hand_cases(K)['tip_on_arm']
    one = cc.clean_unitigs(reads, K, 2, K, 2 * K, clean_rounds=1)
    two = cc.clean_unitigs(reads, K, 2, K, 2 * K, clean_rounds=2)
    assert numbers(one[2]) == (1, 4, 0, 0, 1) and numbers(two[2]) == clean == (1, 4, 1, K, 2)
    assert len(one[0]) == 4 and two[0] == sorted(want) and two == cc.clean_unitigs(reads, K, 2, K, 2 * K, clean_rounds=8)
    # after the one round the graph is the bubble without the tip
    assert one[0] == cc.clean_unitigs(cc.hand_cases(K)['snp'][0], K, 2, 0, 0)[0]


def test_only_the_limit_that_is_set_cleans():
    cases = cc.hand_cases(13)
    assert numbers(cc.clean_unitigs(cases['tip'][0], 13, 2, 0, 26)[2]) == (0, 0, 0, 0, 0)
    assert numbers(cc.clean_unitigs(cases['snp'][0], 13, 2, 13, 0)[2]) == (0, 0, 0, 0, 0)
    assert numbers(cc.clean_unitigs(cases['tip'][0], 13, 2, 4, 0)[2]) == (1, 4, 0, 0, 1)
    assert numbers(cc.clean_unitigs(cases['tip'][0], 13, 2, 3, 0)[2]) == (0, 0, 0, 0, 0)
    assert numbers(cc.clean_unitigs(cases['snp'][0], 13, 2, 0, 13)[2]) == (0, 0, 1, 13, 1)
    assert numbers(cc.clean_unitigs(cases['snp'][0], 13, 2, 0, 12)[2]) == (0, 0, 0, 0, 0)


# ---- invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [13, 31])
def test_read_order_strand_and_partition_order_say_nothing(K):
    rows = cc.planted_answers(K, 2, range(300))
    rng = random.Random(K)
    again = []
    for kind, reads, found, stats, clean in rows:
        other = [read if 'N' in read.upper() else ac.rc(read) for read in reads]
        rng.shuffle(other)
        again.append(cc.clean_unitigs(other, K, 2, K, 2 * K))
        assert again[-1] == (found, stats, clean), kind
    order = list(range(len(rows)))
    rng.shuffle(order)
    assert cc.add_clean([again[i][2] for i in order]) == cc.add_clean([row[4] for row in rows])
    assert ac.add_stats([again[i][1] for i in order]) == ac.add_stats([row[3] for row in rows])


# ---- the census of the planted generator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [13, 31])
def test_census_of_the_planted_partitions(K):
    seen = dict.fromkeys(('arm', 'tip', 'two_rounds', 'mean_tie', 'three_arms', 'hairpin_self', 'one_round_differs'), 0)
    kinds = set()
    for seed, (kind, reads, found, stats, clean) in zip(cc.PLANTED_SEEDS, cc.planted_answers(K, 2)):
        events = cc.planted_events[K, 2, seed]
        kinds.add(kind)
        seen['arm'] += clean['arms'] > 0
        seen['tip'] += clean['tips'] > 0
        seen['two_rounds'] += clean['rounds'] >= 2
        seen['mean_tie'] += events['mean_tie'] > 0
        seen['three_arms'] += events['three_arms'] > 0
        seen['hairpin_self'] += events['hairpin_self'] > 0
        if clean['rounds'] >= 2:                        # (one removing round or none: the first round is all there is)
            seen['one_round_differs'] += cc.clean_unitigs(reads, K, 2, K, 2 * K, clean_rounds=1)[0] != found
    assert kinds == set(cc.PLANTED) and len(cc.PLANTED_SEEDS) == 600
    # each K alone meets what the two together are asked for (when written, at K = 13 and 31: 362 and 368 cases with an arm
    # removed, 163 and 163 with a tip, 50 and 50 of two rounds, 152 and 148 mean ties, 50 and 50 of three arms, 37 and 37 hairpins)
    for name, least in (('arm', 100), ('tip', 100), ('two_rounds', 30), ('mean_tie', 20), ('three_arms', 20), ('hairpin_self', 10),
                        ('one_round_differs', 10)):
        assert seen[name] >= least, (name, seen)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.hc_last_error.restype = ctypes.c_char_p
    L.hc_launch_bytes.restype = U64
    L.hc_launch_bytes.argtypes = [U64, U64, U64, ctypes.c_int, U32, U32]
    L.hc_check_clean.restype = ctypes.c_int
    L.hc_check_clean.argtypes = [U32, U32, U32]
    L.hc_plan.restype = ctypes.c_int
    L.hc_plan.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_int, U64, U32, U32, U32, ctypes.c_void_p, ctypes.c_void_p]
    return L


def arrays(lengths_per_part):
    lengths = [n for part in lengths_per_part for n in part]
    read_off = (U64 * (len(lengths) + 1))()
    for i, n in enumerate(lengths):
        read_off[i + 1] = read_off[i] + n
    part_first = (U64 * (len(lengths_per_part) + 1))()
    for p, part in enumerate(lengths_per_part):
        part_first[p + 1] = part_first[p] + len(part)
    return read_off, len(lengths), part_first, len(lengths_per_part)


def harness_plan(lib, lengths_per_part, K, budget, tip_nodes, bubble_nodes, clean_rounds=8):
    read_off, n_reads, part_first, n_parts = arrays(lengths_per_part)
    rows = (U64 * (9 * max(n_parts, 1)))()
    n = U64(0)
    rc_ = lib.hc_plan(read_off, n_reads, part_first, n_parts, K, budget, tip_nodes, bubble_nodes, clean_rounds, rows, ctypes.byref(n))
    return rc_, [[int(v) for v in rows[9 * l:9 * l + 9]] for l in range(n.value)]


def test_harness_and_mirror_share_their_constants(lib):
    out = (U64 * 2)()
    lib.hc_constants(out)
    assert [int(v) for v in out] == [cc.CLEAN_BYTES_PER_WINDOW, 8]
    for K in (31, 33):
        for windows, bases, reads in ((0, 0, 0), (1, 31, 1), (255, 1000, 3), (256, 4000, 9), (257, 90000, 700), (10 ** 7, 10 ** 8, 10 ** 6)):
            plain = lib.hc_launch_bytes(windows, bases, reads, K, 0, 0)
            assert plain == ac.launch_bytes(windows, bases, reads, K) == cc.clean_launch_bytes(windows, bases, reads, K, False)
            for limits in ((1, 0), (0, 1), (31, 62)):
                assert lib.hc_launch_bytes(windows, bases, reads, K, *limits) == cc.clean_launch_bytes(windows, bases, reads, K, True) == plain + 12 * windows


def test_cleaning_arguments_are_refused(lib):
    assert lib.hc_check_clean(0, 0, 0) == KV_OK                         # no cleaning: the rounds say nothing
    assert lib.hc_check_clean(31, 62, 1) == KV_OK and lib.hc_check_clean(0, 1, 8) == KV_OK
    for limits in ((1, 0), (0, 1), (31, 62)):
        assert lib.hc_check_clean(limits[0], limits[1], 0) == KV_ERR_ARG
        assert b'clean_rounds' in lib.hc_last_error()
    assert harness_plan(lib, [[100, 100]], 31, 1 << 30, 31, 62, clean_rounds=0)[0] == KV_ERR_ARG
    assert harness_plan(lib, [[100, 100]], 30, 1 << 30, 31, 62)[0] == KV_ERR_ARG


@pytest.mark.parametrize('K', [31, 33])
def test_plan_with_cleaning_equals_its_mirror(lib, K):
    rng = random.Random(5 * K)
    cut_differs = 0
    for trial in range(60):
        lengths = [[rng.randrange(0, 300) for _ in range(rng.randrange(0, 30))] for _ in range(rng.randrange(1, 40))]
        sizes = [ac.partition_size(part, K) for part in lengths]
        alone = max(cc.clean_launch_bytes(w, b, r, K, True) for w, b, r in sizes)
        everything = cc.clean_launch_bytes(*[sum(s[j] for s in sizes) for j in range(3)], K, True)
        budget = alone + (everything - alone) * rng.randrange(0, 101) // 100
        ends = {}
        for limits in ((0, 0), (K, 2 * K), (0, 5)):
            rc_, rows = harness_plan(lib, lengths, K, budget, *limits)
            want = cc.clean_plan(lengths, K, budget, *limits)
            assert rc_ == KV_OK and [row[1] for row in rows] == want
            assert [row[0] for row in rows] == [0] + want[:-1]
            for row in rows:
                part = [sum(s[j] for s in sizes[row[0]:row[1]]) for j in range(3)]
                assert row[5] == part[0] and row[4] == part[1] and row[3] - row[2] == part[2]
                assert row[8] == cc.clean_launch_bytes(part[0], part[1], part[2], K, limits != (0, 0)) <= budget
            ends[limits] = want
        assert ends[0, 0] == ac.plan(lengths, K, budget)                # without cleaning: the plan of today
        assert ends[K, 2 * K] == ends[0, 5] and len(ends[K, 2 * K]) >= len(ends[0, 0])
        cut_differs += ends[K, 2 * K] != ends[0, 0]
        # one byte under what the largest partition needs with cleaning: refused
        assert harness_plan(lib, lengths, K, alone - 1, K, 2 * K)[0] == KV_ERR_CAPACITY and cc.clean_plan(lengths, K, alone - 1, K, 2 * K) is None
    assert cut_differs > 10


# ---- the parsers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('module', ['assemble', 'alac'])
def test_clean_flags_of_the_two_parsers(module):
    import importlib
    mod = importlib.import_module('kevlar_amd.' + module)
    from kevlar_amd.assemble import clean_limits, clean_settings
    tail = ['reads.afq'] if module == 'assemble' else ['reads.afq', 'refr.fa']
    parse = lambda *flags: clean_settings(mod.parser().parse_args(list(flags) + tail))      # noqa: E731
    assert parse() == (0, 0, 8)
    assert parse('--clean') == (31, 62, 8) == clean_limits(31) + (8,)
    assert parse('--clean', '--asm-k', '25') == (25, 50, 8)
    assert parse('--tip-nodes', '20') == (20, 0, 8) and parse('--bubble-nodes', '40') == (0, 40, 8)
    assert parse('--clean', '--tip-nodes', '20', '--clean-rounds', '3') == (20, 62, 3)
    assert parse('--clean', '--bubble-nodes', '0') == (31, 0, 8)


def test_the_binding_and_the_header_know_the_new_entries():
    from kevlar_amd import _lib
    from kevlar_amd import assemble as asm
    names = {'kv_assemble_clean_batch', 'kv_assemble_clean_stats', 'kv_assemble_clean_plan'}
    assert names <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, 'include', 'kvsketch.h')).read()
    assert all('int {}('.format(name) in header for name in names) and '#define KV_ASSEMBLE_NCLEAN 5' in header
    assert '#define KV_ASSEMBLE_NSTATS 7' in header and len(asm.STAT_NAMES) == 7
    assert asm.CLEAN_NAMES == cc.CLEAN_NAMES and asm.DEFAULT_CLEAN_ROUNDS == 8 and asm.clean_limits(31) == cc.clean_limits(31) == (31, 62)
