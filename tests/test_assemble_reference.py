"""The assembly rule without a GPU: the plain-Python restatement of tests/assemble_common.py against what the reference's own
tests state about fermi-lite's contigs (tests/golden/assemble/recorded.json, read out of kevlar/tests/test_assemble.py), the
restatement held to change and, on repeats, hairpins and rings, to the rule itself (ac.check_unitigs), the planner of
kevlar_amd/csrc/kv_asm_plan.h at its edges (the header compiles for the host; tests/harness/asm_plan_host.cpp wraps it in a C
ABI), and the command line's four new entries.

The two assemblers differ by a few bases at contig ends and on repeats; the figures measured when the module was written stand
beside each assertion."""
import ctypes
import os
import random
import subprocess

import pytest

import assemble_common as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kevlar_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'harness', 'asm_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libasm_plan_host.so')
HEADERS = [os.path.join(CSRC, name) for name in ('kv_require.h', 'kv_asm_plan.h')]
KV_OK, KV_ERR_ARG, KV_ERR_CAPACITY = 0, -1, -6
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
END_SLACK = 7       # bases of the shorter contig that the longest common substring may miss


@pytest.fixture(scope='module')
def rec():
    return ac.recorded()


# ---- the restatement against the reference's statements ------------------------------------------------------------------------
def test_the_six_fixtures_without_a_contig(rec):
    assert len(rec['no_contig']) == 6
    for name in rec['no_contig']:
        assert ac.contigs(ac.all_reads(name)) == [], name


# fixture: (the rule's contig, the reference's, their longest common substring), as measured
MEASURED = {
    'reads2chain.fq.gz': (257, 246, 243),
    'fml/cc110.afq.gz': (242, 240, 233),
    'fml/cc206.afq.gz': (280, 285, 280),
    'fml/cc322.afq.gz': (230, 260, 230),
    'fml/cc58.afq.gz': (259, 281, 259),
    'var1.reads.augfastq': (145, 122, 119),
}


@pytest.mark.parametrize('name', sorted(MEASURED))
def test_one_contig_close_to_the_reference(rec, name):
    stated = rec['one_contig'][name]
    found = ac.contigs(ac.all_reads(name))
    assert len(found) == 1
    common = ac.common_either_strand(found[0], stated)
    assert common >= min(len(found[0]), len(stated)) - END_SLACK
    assert (len(found[0]), len(stated), common) == MEASURED[name]


def test_fiveparts(rec):
    parts = ac.read_partitions('fiveparts.augfastq.gz')
    assert [pid for pid, _ in parts] == ['1', '2', '3', '4', '5']
    found = [ac.contigs(reads) for _, reads in parts]
    assert [[len(c) for c in contigs] for contigs in found] == [[481], [192], [190], [146], [166]]
    stated = rec['fiveparts_partition_4']          # the seventh row of the table: 146, 123, 123
    common = ac.common_either_strand(found[3][0], stated)
    assert (len(stated), common) == (123, 123) and common >= min(len(stated), len(found[3][0])) - END_SLACK


def test_cc231_is_the_known_departure(rec):
    # The reference states one contig of 216 bases here.  It is built of near-copies of one stretch (...ACATAAAATATCAAAGTACCCAAAATGTGTATTA...
    # comes round again and again with substitutions), copies of 24 bases and more that a graph of 31-mers cannot thread: every
    # unitig ends at the next fork and none is longer than a read.  The rule has no repeat resolution (fermi-lite's string graph
    # has).  No contig: the one recorded departure.
    assert len(rec['one_contig']['fml/cc231.afq.gz']) == 216
    reads = ac.all_reads('fml/cc231.afq.gz')
    unitigs, stats = ac.unitigs(reads)
    assert ac.contigs(reads) == [] and len(unitigs) > 1 and max(len(u) for u in unitigs) <= max(len(r) for r in reads)


def test_pico_fixtures():
    lengths = {}
    for cc in (2, 3, 5, 6, 7, 8, 9, 10):
        lengths[cc] = [len(c) for c in ac.contigs(ac.all_reads('pico-var/cc{}.afq.gz'.format(cc)))]
    assert all(len(found) == 1 for cc, found in lengths.items() if cc != 2)
    assert len(lengths[2]) == 2                     # a 160-base insertion: the graph forks inside it
    assert len(ac.contigs(ac.all_reads('pico-4.augfastq.gz'))) == 1


# ---- held to change: the restatement's answer depends on what it should depend on ------------------------------------------------
def test_restatement_changes_with_a_read_and_with_min_count():
    reads = ac.all_reads('fml/cc110.afq.gz')
    whole, stats = ac.unitigs(reads)
    changed = 0
    for leave in range(len(reads)):
        fewer, fewer_stats = ac.unitigs(reads[:leave] + reads[leave + 1:])
        assert fewer_stats['windows'] < stats['windows']
        changed += fewer != whole
    assert changed > 0                              # (a read whose every window is still seen twice changes nothing)
    answers = [ac.unitigs(reads, 31, m) for m in (1, 2, 3)]
    assert answers[0][0] != answers[1][0] != answers[2][0]
    assert answers[0][1]['solid'] > answers[1][1]['solid'] > answers[2][1]['solid']
    assert answers[0][1]['solid'] == answers[0][1]['distinct']
    # (another K can give the same strings where the graph is one clean path; the windows behind them differ)
    assert ac.unitigs(reads, 29, 2)[1]['windows'] > stats['windows'] > ac.unitigs(reads, 33, 2)[1]['windows']


def test_restatement_on_hand_made_graphs():
    rng = random.Random(3)
    seq = ac.random_dna(rng, 100)
    once, stats = ac.unitigs([seq, seq], 31)
    assert once == [min(seq, ac.rc(seq))] and stats == dict(windows=140, distinct=70, solid=70, heads=2, unitigs=1, cycle_keys=0)
    assert ac.unitigs([seq, ac.rc(seq)], 31) == (once, stats)          # the strand of a read says nothing
    assert ac.unitigs([seq], 31)[0] == [] and ac.contigs([seq, seq]) == []
    assert ac.contigs([seq[:60], seq[:60], seq[20:], seq[20:]]) == once
    ring = ac.random_dna(rng, 90)
    found, stats = ac.unitigs([ring + ring[:60]] * 2, 31)
    assert found == [] and stats['cycle_keys'] == stats['solid'] == 90 and stats['heads'] == 0
    half = ac.random_dna(rng, 40)
    own = half + ac.rc(half)
    found, stats = ac.unitigs([own, own], 31)
    assert found == [own] and stats['heads'] == 1 and stats['solid'] == 25


# ---- the restatement against the rule itself: ac.check_unitigs needs no walk -------------------------------------------------------
@pytest.mark.parametrize('third', [0, 1, 2])
@pytest.mark.parametrize('min_count', [1, 2, 3])
@pytest.mark.parametrize('K', [13, 15, 31, 33, 63])
def test_restatement_keeps_the_rule_on_structured_partitions(K, min_count, third):
    seeds = ac.FUZZ_SEEDS[200 * third:200 * third + 200]
    assert len(seeds) == 200 and len(ac.FUZZ_SEEDS) == 600
    for kind, reads, found, stats in ac.structured_answers(K, min_count, seeds):
        ac.check_unitigs(reads, K, min_count, found, stats)


def test_restatement_keeps_the_rule_on_seeded_partitions_and_fixtures():
    for K in (13, 31, 33, 63):                      # the inputs of tests/test_gpu_assemble.py
        for i in range(4):
            reads = ac.seeded_partition(100 * K + i, n_reads=14, read_len=90 + 7 * i, hap_len=230)
            ac.check_unitigs(reads, K, 2, *ac.unitigs(reads, K, 2))
    for seed in (5, 77, 78):
        reads = ac.seeded_partition(seed, 12, 80, 200)
        ac.check_unitigs(reads, 31, 2, *ac.unitigs(reads, 31, 2))
    names = [name for name in ac.recorded()['files'] if name.startswith(('fml/', 'pico-var/'))]
    assert len(names) >= 13
    for name in names:
        for partid, reads in ac.read_partitions(name):
            found, stats = ac.unitigs(reads, 31, 2)
            ac.check_unitigs(reads, 31, 2, found, stats)
            assert stats['solid'] > 0, name


def test_structured_partitions_are_what_they_say():
    assert [ac.structured_partition(seed)[0] for seed in range(12)] == list(ac.KINDS) * 2
    assert ac.structured_partition(41) == ac.structured_partition(41)
    for seed in ac.FUZZ_SEEDS:
        kind, reads = ac.structured_partition(seed)
        assert 4 <= len(reads) <= 29 and len(set(len(r) for r in reads)) == 1 and 20 <= len(reads[0]) <= 69
        assert not ''.join(reads).strip('ACGTN')
        if kind in ('alpha2', 'alpha2rc'):          # (on either strand; a replaced byte may be any letter: at most one per read)
            alphabet = 'AC' if kind == 'alpha2' else 'AT'
            assert all(min(len(r.replace(alphabet[0], '').replace(alphabet[1], '')) for r in (read, ac.rc(read))) <= 1 for read in reads)
    rng = random.Random(1)
    for _ in range(200):
        for kind in ac.KINDS:
            assert 60 <= len(ac.structured_haplotype(rng, kind)) <= 260


# The census of the fuzz, as conditions on the inputs: what the device test of tests/test_gpu_assemble_shapes.py is certain to meet.
# Counted by the restatement alone over the same seeds in four of that test's fifteen cases, the cheapest that clear every floor
# (each further case only adds).  Figures when written: 116 cases with cycle keys, 20 of them with heads too, 276 unitigs that are
# their own reverse complement, 1184 cases of three unitigs or more; over K in {13, 15, 31} and min_count in {1, 2}: 57, 20, 469, 2659.
def test_census_of_the_structured_fuzz():
    cycles = cycles_and_heads = own = three = 0
    answered = dict.fromkeys(ac.KINDS, 0)
    for K in (13, 31):
        for min_count in (2, 3):
            for kind, reads, found, stats in ac.structured_answers(K, min_count):
                cycles += stats['cycle_keys'] > 0
                cycles_and_heads += stats['cycle_keys'] > 0 and stats['heads'] > 0
                own += sum(1 for u in found if u == ac.rc(u))
                three += len(found) >= 3
                answered[kind] += len(found) > 0
    assert cycles_and_heads >= 10
    assert cycles >= 40
    assert own >= 100
    assert three >= 1000
    assert all(n >= 1 for n in answered.values()), answered
    # the two-word keys meet hairpins and their own reverse complements too (K = 33; a read of the fuzz is too short for one at 63)
    assert sum(1 for m in (2, 3) for _, _, found, _ in ac.structured_answers(33, m) for u in found if u == ac.rc(u)) >= 10


def test_the_checker_rejects_three_wrong_answers():
    K, min_count = 15, 2
    cases = ac.structured_answers(K, min_count)
    # a unitig reported as the larger strand
    kind, reads, found, stats = next(c for c in cases if any(u != ac.rc(u) for u in c[2]))
    ac.check_unitigs(reads, K, min_count, found, stats)
    at = next(i for i, u in enumerate(found) if u != ac.rc(u))
    with pytest.raises(AssertionError, match='larger strand'):
        ac.check_unitigs(reads, K, min_count, found[:at] + [ac.rc(found[at])] + found[at + 1:], stats)
    # a unitig cut in two at a simple edge, each piece as its smaller strand
    kind, reads, found, stats = next(c for c in cases if any(len(u) >= K + 4 and u != ac.rc(u) for u in c[2]))
    at = next(i for i, u in enumerate(found) if len(u) >= K + 4 and u != ac.rc(u))
    cut = (len(found[at]) - K) // 2
    pieces = [min(piece, ac.rc(piece)) for piece in (found[at][:cut + K], found[at][cut + 1:])]
    assert len(pieces[0]) + len(pieces[1]) == len(found[at]) + K - 1
    with pytest.raises(AssertionError, match='goes on'):
        ac.check_unitigs(reads, K, min_count, sorted(found[:at] + pieces + found[at + 1:]), dict(stats, unitigs=stats['unitigs'] + 1))
    # a unitig that is its own reverse complement dropped, its keys counted as a cycle's
    kind, reads, found, stats = next(c for c in cases if any(u == ac.rc(u) for u in c[2]))
    ac.check_unitigs(reads, K, min_count, found, stats)
    at = next(i for i, u in enumerate(found) if u == ac.rc(u))
    fewer = dict(stats, unitigs=stats['unitigs'] - 1, heads=stats['heads'] - 1, cycle_keys=stats['cycle_keys'] + (len(found[at]) - K + 1) // 2)
    with pytest.raises(AssertionError, match='on no unitig and not on a cycle'):
        ac.check_unitigs(reads, K, min_count, found[:at] + found[at + 1:], fewer)
    # and a wrong count alone
    for name in ac.STAT_NAMES:
        with pytest.raises(AssertionError):
            ac.check_unitigs(reads, K, min_count, found, dict(stats, **{name: stats[name] + 1}))


# ---- the planner -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_last_error.restype = ctypes.c_char_p
    for name, args in (('h_table_cap', [U64]), ('h_grid', [U64]), ('h_launch_bytes', [U64, U64, U64, ctypes.c_int]),
                       ('h_read_windows', [U64, ctypes.c_int]), ('h_read_runs', [U64, ctypes.c_int])):
        getattr(L, name).restype = U64
        getattr(L, name).argtypes = args
    L.h_constants.argtypes = [ctypes.c_void_p]
    L.h_check_args.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_int, U32]
    L.h_plan.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_int, U64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def arrays(partition_read_lengths):
    read_off, part_first = [0], [0]
    for lengths in partition_read_lengths:
        for n in lengths:
            read_off.append(read_off[-1] + n)
        part_first.append(len(read_off) - 1)
    return (U64 * len(read_off))(*read_off), len(read_off) - 1, (U64 * len(part_first))(*part_first), len(part_first) - 1


def host_plan(lib, partition_read_lengths, K, budget):
    """(return code, rows of (part0, part1, read0, read1, bases, windows, runs, table slots, bytes))"""
    read_off, n_reads, part_first, n_parts = arrays(partition_read_lengths)
    rows = (U64 * (9 * max(n_parts, 1)))()
    n = U64(0)
    rc = lib.h_plan(read_off, n_reads, part_first, n_parts, K, budget, rows, ctypes.byref(n))
    return rc, [tuple(int(v) for v in rows[9 * l:9 * l + 9]) for l in range(n.value)]


def test_harness_and_test_share_their_constants(lib):
    out = (U64 * 8)()
    lib.h_constants(out)
    assert [int(v) for v in out] == [13, 63, 256, ac.RUN, 4096, 1024, ac.MAX_WINDOWS, 72]


def test_sizes_at_their_edges(lib):
    for n in (0, 1, 503, 504, 505, 1 << 20, (1 << 20) - 8, (1 << 20) - 7, ac.MAX_WINDOWS):
        cap = lib.h_table_cap(n)
        assert cap == ac.table_cap(n) and cap >= 2 * n + 16 and cap & (cap - 1) == 0 and (cap == 1024 or cap // 2 < 2 * n + 16)
    assert [lib.h_grid(n) for n in (0, 1, 256, 257, 4096 * 256, 4096 * 256 + 1, 1 << 40)] == [1, 1, 1, 2, 4096, 4096, 4096]
    for K in (13, 31, 33, 63):
        assert [lib.h_read_windows(n, K) for n in (0, K - 1, K, K + 1, K + 31, K + 32)] == [0, 0, 1, 2, 32, 33]
        assert [lib.h_read_runs(n, K) for n in (0, K - 1, K, K + 31, K + 32, K + 63, K + 64)] == [0, 0, 1, 1, 2, 2, 3]
        for size in ((0, 0, 0), (1, K, 1), (1000, 5000, 30), (1 << 22, 1 << 23, 1 << 15)):
            assert lib.h_launch_bytes(size[0], size[1], size[2], K) == ac.launch_bytes(size[0], size[1], size[2], K)
    assert ac.launch_bytes(100, 0, 0, 33) - ac.launch_bytes(100, 0, 0, 31) == 800        # the second key word


def test_plan_cuts_where_the_restatement_does(lib):
    rng = random.Random(11)
    for round_ in range(60):
        K = rng.choice((13, 31, 33, 63))
        parts = [[rng.choice((0, K - 1, K, 100, 150, 400)) for _ in range(rng.randrange(0, 12))] for _ in range(rng.randrange(1, 25))]
        alone = [ac.launch_bytes(*ac.partition_size(lengths, K), K) for lengths in parts]
        everything = ac.launch_bytes(*[sum(v) for v in zip(*[ac.partition_size(lengths, K) for lengths in parts])], K)
        for budget in (everything, everything - 1, max(alone), max(alone) + rng.randrange(0, everything), 1 << 40):
            want = ac.plan(parts, K, budget)
            rc, rows = host_plan(lib, parts, K, budget)
            if want is None:                        # (every other partition is empty: one byte less than everything refuses the one)
                assert rc == KV_ERR_CAPACITY and budget == max(alone) - 1 == everything - 1
                continue
            assert rc == KV_OK and [row[1] for row in rows] == want
            at = 0
            for part0, part1, read0, read1, bases, windows, runs, slots, nbytes in rows:
                inside = parts[part0:part1]
                size = [sum(v) for v in zip(*[ac.partition_size(lengths, K) for lengths in inside])]
                assert part0 == at and (windows, bases, read1 - read0) == tuple(size) and read0 == sum(len(p) for p in parts[:part0])
                assert nbytes == ac.launch_bytes(windows, bases, read1 - read0, K) <= budget and slots == ac.table_cap(windows)
                assert runs == sum((max(n - K + 1, 0) + ac.RUN - 1) // ac.RUN for lengths in inside for n in lengths)
                at = part1
            assert at == len(parts)
        assert host_plan(lib, parts, K, everything)[1][-1][1] == len(parts) and len(host_plan(lib, parts, K, everything)[1]) == 1
        rc, rows = host_plan(lib, parts, K, max(alone) - 1)
        assert rc == KV_ERR_CAPACITY and ac.plan(parts, K, max(alone) - 1) is None
        assert b'partition' in lib.h_last_error() and b'budget' in lib.h_last_error()


def test_plan_of_nothing_and_of_empty_partitions(lib):
    assert host_plan(lib, [], 31, 1 << 30) == (KV_OK, [])
    rc, rows = host_plan(lib, [[], [], [10, 20]], 31, 1 << 30)
    assert rc == KV_OK and [row[:7] for row in rows] == [(0, 3, 0, 2, 30, 0, 0)]


def test_argument_rules(lib):
    good_off, good_first = [0, 60, 120], [0, 1, 2]

    def check(ksize=31, min_count=2, off=good_off, first=good_first, n_reads=2, n_parts=2):
        return lib.h_check_args((U64 * len(off))(*off), n_reads, (U64 * len(first))(*first), n_parts, ksize, min_count)

    assert check() == KV_OK
    assert [check(ksize=k) for k in (13, 15, 31, 33, 61, 63)] == [KV_OK] * 6
    assert [check(ksize=k) for k in (-1, 0, 11, 12, 14, 30, 32, 62, 64, 65)] == [KV_ERR_ARG] * 10
    assert b'odd' in lib.h_last_error()
    assert check(min_count=0) == KV_ERR_ARG and check(min_count=1) == KV_OK
    assert check(off=[0, 130, 120]) == KV_ERR_ARG and check(off=[0, 0, 0]) == KV_OK
    assert [check(first=f) for f in ([0, 2, 1], [1, 1, 2], [0, 1, 1], [0, 0, 3])] == [KV_ERR_ARG] * 4
    assert check(first=[0, 0, 2]) == KV_OK and check(first=[0, 2, 2]) == KV_OK
    assert lib.h_check_args(None, 0, None, 0, 31, 2) == KV_ERR_ARG


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_cli_knows_the_four_new_entries():
    import kevlar_amd
    cli = kevlar_amd.cli
    assert set(cli.calling_mains) == {'assemble', 'alac', 'call', 'simlike'}
    assert set(cli.mains) == {'count', 'novel', 'filter', 'partition', 'unband', 'dist', 'split', 'augment', 'gentrio'}
    assert cli.downstream_mains == {'localize': kevlar_amd.localize.main}
    args = cli.parser().parse_args(['assemble', 'reads.augfastq'])
    assert (args.cmd, args.augfastq, args.part_id, args.max_reads, args.out, args.asm_k, args.min_count) == (
        'assemble', 'reads.augfastq', None, 10000, None, 31, 2)
    args = cli.parser().parse_args(['assemble', '-p', '7', '--max-reads', '50', '-o', 'c.augfasta', '--asm-k', '25', '--min-count', '3', 'r.fq'])
    assert (args.part_id, args.max_reads, args.out, args.asm_k, args.min_count) == ('7', 50, 'c.augfasta', 25, 3)
    args = cli.parser().parse_args(['alac', 'reads.augfastq', 'refr.fa'])
    assert (args.cmd, args.infile, args.refr, args.part_id, args.max_reads, args.seed_size, args.delta, args.max_diff) == (
        'alac', 'reads.augfastq', 'refr.fa', None, 10000, 51, 50, None)
    assert (args.include, args.exclude, args.max_target_length, args.match, args.mismatch, args.open, args.extend) == (None, None, 10000, 1, 2, 5, 0)
    assert (args.gen_mask, args.mask_mem, args.mask_max_fpr, args.out, args.min_ikmers, args.ksize, args.threads) == (None, 1e6, 0.01, None, None, 31, 1)
    assert (args.asm_k, args.min_count, args.max_occ) == (31, 2, 5000)
    args = cli.parser().parse_args(['alac', '-p', '2', '-z', '31', '-d', '25', '-x', '0', '--include', 'chr', '--exclude', 'Un', '-A', '2', '-B', '3',
                                    '-O', '6', '-E', '1', '--gen-mask', 'm.nt', '--mask-mem', '1M', '--mask-max-fpr', '0.1', '-i', '3', '-k', '25',
                                    '-t', '4', '--max-target-length', '500', '--max-occ', '9', '-o', 'o.vcf', 'a', 'b'])
    assert (args.part_id, args.seed_size, args.delta, args.max_diff, args.include, args.exclude, args.match, args.mismatch, args.open,
            args.extend, args.gen_mask, args.mask_mem, args.mask_max_fpr, args.min_ikmers, args.ksize, args.threads,
            args.max_target_length, args.max_occ, args.out) == ('2', 31, 25, 0, 'chr', 'Un', 2, 3, 6, 1, 'm.nt', 1e6, 0.1, 3, 25, 4, 500, 9, 'o.vcf')
    # `call` and `simlike` take the definitions of their modules' own parsers
    import kevlar_amd.call
    import kevlar_amd.simlike
    for name, module, argv in (('call', kevlar_amd.call, ['contigs.augfasta', 'targets.fa']),
                               ('simlike', kevlar_amd.simlike, ['--case', 'kid.ct', '--controls', 'mom.ct', 'dad.ct', '--refr', 'r.sct', 'calls.vcf'])):
        own = vars(module.parser().parse_args(argv))
        through = vars(cli.parser().parse_args([name] + argv))
        assert through.pop('cmd') == name and through.pop('logfile') is None and through.pop('tee') is False
        assert through == own
        assert cli.calling_mains[name].__name__ == name + '_main'
    helptext = cli.parser().format_help()
    assert all(name in helptext for name in ('assemble', 'alac', 'call', 'simlike', 'localize', 'novel'))
