"""`kevlar assemble` on the device: every case compares the FULL unitig set of every partition and the stats of the call
(kevlar_amd/csrc/kv_assemble.hip through kevlar_amd.assemble.unitigs_batch) with the plain-Python restatement of the rule in
tests/assemble_common.py -- never with itself -- and the command line with what the reference's own tests state."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd import assemble as asm

import assemble_common as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


agree, device_plan = ac.agree, ac.device_plan       # (shared with tests/test_gpu_assemble_shapes.py)


@pytest.fixture(scope='module')
def rng():
    return random.Random(20261021)


# ---- 1. K on both sides of the word switch ------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [13, 31, 33, 63])
def test_seeded_partitions_at_k(hk, K):
    parts = [ac.seeded_partition(100 * K + i, n_reads=14, read_len=90 + 7 * i, hap_len=230) for i in range(4)]
    found, stats = agree(parts, K)
    assert stats['unitigs'] > 0 and stats['solid'] < stats['distinct']


# ---- 2. reads at the edges ----------------------------------------------------------------------------------------------------
def test_short_reads_single_read_empty_partition_n_runs_lower_case(hk, rng):
    hap = ac.random_dna(rng, 150)
    with_n = hap[:60] + 'NNNN' + hap[64:110] + 'N' + hap[111:]
    parts = [
        [hap[:30], hap[:31], hap[5:20], ''],                # shorter than K, exactly K, and an empty read
        [hap],                                              # one read: nothing is seen twice
        [],                                                 # no read at all
        [with_n, with_n, hap[40:120]],                      # runs of N cut the windows
        [hap.lower(), hap, hap[:80].lower() + hap[80:]],    # either case counts
        ['N' * 50, 'n' * 40, 'ACGTRYKM' * 6],               # nothing valid
    ]
    found, stats = agree(parts, 31)
    assert found[1] == [] and found[2] == [] and found[5] == []
    assert len(found[4]) == 1 and len(found[4][0]) == 150
    agree(parts, 31, min_count=1)
    agree(parts, 13, min_count=2)


@pytest.mark.parametrize('min_count', [1, 2, 3, 4])
def test_counts_on_either_side_of_min_count(hk, rng, min_count):
    hap = ac.random_dna(rng, 120)
    # the windows of the left read are seen min_count times, those of the right one min_count - 1 times; they share none
    reads = [hap[:75]] * min_count + [hap[60:]] * (min_count - 1)
    found, stats = agree([reads], 31, min_count)
    counts, _ = ac.key_counts(reads, 31)
    assert min_count in counts.values() and (min_count == 1 or min_count - 1 in counts.values())
    assert stats['solid'] == sum(1 for c in counts.values() if c >= min_count)


# ---- 3. shapes of the graph -----------------------------------------------------------------------------------------------------
def test_snp_bubble_gives_four_unitigs(hk, rng):
    hap = ac.random_dna(rng, 161)
    alt = hap[:80] + ('A' if hap[80] != 'A' else 'C') + hap[81:]
    reads = ac.tiled_reads(hap, 70, 7, copies=2) + ac.tiled_reads(alt, 70, 7, copies=2)
    found, stats = agree([reads], 31)
    assert len(found[0]) == 4 and sorted(len(u) for u in found[0]) == [61, 61, 80, 80]


def test_fork_and_tip(hk, rng):
    trunk, left, right = ac.random_dna(rng, 100), ac.random_dna(rng, 70), ac.random_dna(rng, 70)
    fork = ac.tiled_reads(trunk + left, 60, 5, copies=2) + ac.tiled_reads(trunk + right, 60, 5, copies=2)
    found, _ = agree([fork], 31)
    assert len(found[0]) == 3
    # a tip: a short dead end hanging off the middle of a path
    path = ac.random_dna(rng, 160)
    spur = path[40:80] + ac.random_dna(rng, 12)
    tip = ac.tiled_reads(path, 60, 5, copies=2) + [spur, spur]
    found, _ = agree([tip], 31)
    assert len(found[0]) == 3
    agree([fork, tip, fork + tip], 33)


def test_unitig_equal_to_its_own_reverse_complement(hk, rng):
    half = ac.random_dna(rng, 60)
    own = half + ac.rc(half)
    assert own == ac.rc(own)
    found, stats = agree([[own, own]], 31)
    assert found[0] == [own] and stats['heads'] == 1 and stats['solid'] == (len(own) - 31 + 1) // 2
    agree([[own, own]], 33)
    agree([[own, own, own[:70]]], 13)


def test_hairpin_inside_a_longer_sequence(hk, rng):
    # the node in the middle of stem + rc(stem) has its own reverse complement as its successor
    stem = ac.random_dna(rng, 45)
    seq = ac.random_dna(rng, 50) + stem + ac.rc(stem) + ac.random_dna(rng, 50)
    for K in (31, 33, 13):
        w = (stem + ac.rc(stem))[(90 - K - 1) // 2:][:K]
        assert w[1:] + ac.rc(w)[-1] == ac.rc(w)
        agree([ac.tiled_reads(seq, 80, 4, copies=2)], K)


def test_pure_cycle_gives_nothing_and_is_counted(hk, rng):
    ring = ac.random_dna(rng, 200)
    reads = [(ring + ring)[s:s + 80] for s in range(0, 200, 10) for _ in range(2)]
    found, stats = agree([reads], 31)
    assert found[0] == [] and stats['heads'] == 0 and stats['cycle_keys'] == stats['solid'] == 200
    # the same ring beside an ordinary partition, and with a tail that gives the ring a way in
    tail = ac.random_dna(rng, 60) + ring[:40]
    agree([reads, ac.seeded_partition(5, 12, 80, 200), reads + [tail, tail]], 31)


# ---- 4. partitions keep to themselves -----------------------------------------------------------------------------------------
def test_identical_partitions_give_identical_unitigs(hk):
    reads = ac.seeded_partition(77, n_reads=20, read_len=100, hap_len=260)
    found, _ = agree([reads, list(reads), ac.seeded_partition(78, 10, 80, 200), list(reads)], 31)
    assert found[0] == found[1] == found[3] and found[0]


def test_a_key_seen_once_in_each_of_two_partitions_is_solid_in_neither(hk, rng):
    read = ac.random_dna(rng, 100)
    found, stats = agree([[read], [read]], 31, min_count=2)
    assert found == [[], []] and stats['solid'] == 0 and stats['distinct'] == 2 * 70
    found, _ = agree([[read], [ac.rc(read)], [read, read]], 31, min_count=2)
    assert found == [[], [], [min(read, ac.rc(read))]]


# ---- 5. sizes -------------------------------------------------------------------------------------------------------------------
def test_a_unitig_of_20000_bases(hk, rng):
    seq = ac.random_dna(rng, 20000)
    found, stats = agree([ac.tiled_reads(seq, 250, 125, copies=2)], 31)
    assert found[0] == [min(seq, ac.rc(seq))]


def test_one_partition_of_10000_reads(hk, rng):
    hap = ac.random_dna(rng, 3000)
    reads = [hap[s:s + 42] for s in (rng.randrange(0, 3000 - 42) for _ in range(10000))]
    found, stats = agree([reads], 31)
    assert stats['windows'] == 10000 * 12


def test_300_partitions_at_once_in_sevens_and_one_at_a_time(hk):
    parts = [ac.seeded_partition(9000 + i, n_reads=6 + i % 5, read_len=50 + i % 23, hap_len=110 + i % 40, error=0.02) for i in range(300)]
    want = [ac.unitigs(reads, 31, 2) for reads in parts]
    total = ac.add_stats([s for _, s in want])
    got, stats = asm.unitigs_batch(parts, 31, 2)
    assert [sorted(u) for u in got] == [u for u, _ in want]
    assert {name: stats[name] for name in ac.STAT_NAMES} == total and stats['launches'] == 1
    sevens, summed = [], []
    for at in range(0, 300, 7):
        some, s = asm.unitigs_batch(parts[at:at + 7], 31, 2)
        sevens.extend(some)
        summed.append(s)
    assert [sorted(u) for u in sevens] == [u for u, _ in want] and ac.add_stats(summed) == total
    singles = [asm.unitigs_batch([reads], 31, 2)[0][0] for reads in parts]
    assert [sorted(u) for u in singles] == [u for u, _ in want]


# ---- 6. the planner's edges through the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [31, 33])
def test_launch_split_and_capacity_edges(hk, K):
    parts = [ac.seeded_partition(400 + i, n_reads=5 + 3 * (i % 4), read_len=70 + i, hap_len=180) for i in range(12)]
    lengths = [[len(r) for r in reads] for reads in parts]
    sizes = [ac.partition_size(ls, K) for ls in lengths]
    alone = [ac.launch_bytes(w, b, r, K) for w, b, r in sizes]
    everything = ac.launch_bytes(sum(s[0] for s in sizes), sum(s[1] for s in sizes), sum(s[2] for s in sizes), K)
    whole, _ = agree(parts, K, launches=1)
    for budget in (everything, everything - 1, max(alone), max(alone) + 1, 2 * max(alone), 3 * max(alone) + 17):
        ends = ac.plan(lengths, K, budget)
        assert device_plan(parts, K, budget) == (_lib.KV_OK, ends)
        split, _ = agree(parts, K, mem_budget=budget, launches=len(ends))
        assert split == whole
    assert ac.plan(lengths, K, everything) == [12] and len(ac.plan(lengths, K, everything - 1)) == 2
    assert len(ac.plan(lengths, K, max(alone))) > 2
    # one byte less than the largest partition needs alone: refused, by the plan and by the call
    assert ac.plan(lengths, K, max(alone) - 1) is None
    assert device_plan(parts, K, max(alone) - 1)[0] == _lib.KV_ERR_CAPACITY
    with pytest.raises(_lib.KvCapacityError):
        asm.unitigs_batch(parts, K, 2, mem_budget=max(alone) - 1)


# ---- 7. argument errors leave the outputs alone ------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(hk):
    lib = _lib.load()
    _lib.require_device()
    bases = np.frombuffer(b'ACGT' * 30, dtype=np.uint8)
    good_off, good_first = [0, 60, 120], [0, 1, 2]

    def call(ksize=31, min_count=2, off=good_off, first=good_first, n_reads=2, n_parts=2, null=None):
        off, first = np.array(off, dtype=np.uint64), np.array(first, dtype=np.uint64)
        n_unitigs, n_bases, handle = ctypes.c_uint64(12345), ctypes.c_uint64(54321), ctypes.c_void_p(0xDEAD)
        args = [bases.ctypes.data, off.ctypes.data, n_reads, first.ctypes.data, n_parts, ksize, min_count, 0, ctypes.byref(n_unitigs),
                ctypes.byref(n_bases), ctypes.byref(handle)]
        if null is not None:
            args[null] = None
        rc = lib.kv_assemble_batch(*args)
        return rc, (n_unitigs.value, n_bases.value, handle.value)

    untouched = (12345, 54321, 0xDEAD)
    for bad in (dict(ksize=32), dict(ksize=11), dict(ksize=65), dict(ksize=12), dict(ksize=0), dict(min_count=0), dict(off=[0, 130, 120]),
                dict(first=[0, 2, 1]), dict(first=[1, 1, 2]), dict(first=[0, 1, 1]), dict(null=0), dict(null=1), dict(null=3), dict(null=8),
                dict(null=9), dict(null=10)):
        rc, outputs = call(**bad)
        assert rc == _lib.KV_ERR_ARG and outputs == untouched, bad
        assert _lib.last_error()
    rc, (n_unitigs, n_bases, handle) = call()
    assert rc == _lib.KV_OK and handle not in (None, 0xDEAD)
    lib.kv_assemble_destroy(ctypes.c_void_p(handle))
    with pytest.raises(_lib.KvArgError):
        asm.unitigs_batch([['ACGT' * 20] * 2], 30)


# ---- 8. the reference's fixtures through the command line ------------------------------------------------------------------------
def parse_contigs(text):
    """[(name, sequence)] of augmented FASTA output"""
    lines = text.split('\n')
    return [(ln[1:], lines[i + 1]) for i, ln in enumerate(lines) if ln.startswith('>')]


def test_fixtures_through_the_command_line(hk, capsys, kevlar_log):
    rec = ac.recorded()
    for name in rec['no_contig'] + ['fml/cc231.afq.gz']:
        kevlar_amd.cli.run(['assemble', ac.fixture_path(name)])
        out, err = capsys.readouterr()
        assert out == '', name
    for name, stated in sorted(rec['one_contig'].items()):
        if name == 'fml/cc231.afq.gz':
            continue
        kevlar_amd.cli.run(['assemble', ac.fixture_path(name)])
        out, err = capsys.readouterr()
        contigs = parse_contigs(out)
        assert [seq for _, seq in contigs] == ac.contigs(ac.all_reads(name)), name
        assert len(contigs) == 1 and contigs[0][0].startswith('contig1')
        assert ac.common_either_strand(contigs[0][1], stated) >= min(len(stated), len(contigs[0][1])) - 7


def test_fiveparts_through_the_command_line(hk, capsys, tmp_path, kevlar_log):
    five = ac.fixture_path('fiveparts.augfastq.gz')
    parts = ac.read_partitions('fiveparts.augfastq.gz')
    out_file = str(tmp_path / 'contigs.augfasta')
    kevlar_amd.cli.run(['assemble', '-o', out_file, five])
    contigs = parse_contigs(open(out_file).read())
    assert [name for name, _ in contigs] == ['contig{} kvcc={}'.format(n, pid) for n, (pid, _) in enumerate(parts, 1)]
    assert [[seq] for _, seq in contigs] == [ac.contigs(reads) for _, reads in parts]
    out, err = capsys.readouterr()          # (run() sends the log to stderr)
    assert out == '' and 'processed 5 partitions and assembled 5 contigs' in err
    # annotated with the partition's interesting k-mers
    assert sum(1 for ln in open(out_file) if ln.endswith('#\n')) > 5
    kevlar_amd.cli.run(['assemble', '--part-id', '4', five])
    out, err = capsys.readouterr()
    only = parse_contigs(out)
    assert [name for name, _ in only] == ['contig1 kvcc=4']
    assert ac.common_either_strand(only[0][1], ac.recorded()['fiveparts_partition_4']) == 123
    # the parameters of the rule, and the limit on reads
    kevlar_amd.cli.run(['assemble', '--asm-k', '25', '--min-count', '3', '--part-id', '4', five])
    out, err = capsys.readouterr()
    assert [seq for _, seq in parse_contigs(out)] == ac.contigs(dict(parts)['4'], 25, 3)
    kevlar_amd.cli.run(['assemble', '--max-reads', '20', five])
    out, err = capsys.readouterr()
    assert [name for name, _ in parse_contigs(out)] == ['contig1 kvcc=3', 'contig2 kvcc=4', 'contig3 kvcc=5']
    assert 'WARNING: skipping partition with 67 reads' in err and 'WARNING: skipping partition with 23 reads' in err


def test_the_module_is_a_command(hk, tmp_path):
    out_file = str(tmp_path / 'contigs.augfasta')
    for command in (['-m', 'kevlar_amd', 'assemble'], ['-m', 'kevlar_amd.assemble']):
        done = subprocess.run([sys.executable] + command + ['-o', out_file, ac.fixture_path('var1.reads.augfastq')], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert done.returncode == 0, done.stderr
        assert [seq for _, seq in parse_contigs(open(out_file).read())] == ac.contigs(ac.all_reads('var1.reads.augfastq'))
        assert 'RuntimeWarning' not in done.stderr
