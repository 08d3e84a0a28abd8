"""`kevlar assemble --clean` on the device (kv_assemble.hip: k_asm_measure, k_asm_decide, k_asm_kill and the round loop in front
of the walk): every case compares the FULL unitig set of every partition, the seven stats and the five clean stats of the call
with the plain-Python restatement in tests/asmclean_common.py (cc.agree_clean) -- strings and integers, equal or not.  The
restatement itself is held by tests/test_asmclean_reference.py, which also states the census of the planted inputs."""
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
from kevlar_amd.alac import alac

import assemble_common as ac
import asmclean_common as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_GRID = 4096 * ac.THREADS                        # ASM_MAX_GRID workgroups of ASM_THREADS: 1 048 576
PICO_REFR = ac.fixture_path('human-random-pico.fa.gz')
CC2 = 'pico-var/cc2.afq.gz'


def rows_of(K, min_count, seeds, **limits):
    rows = cc.planted_answers(K, min_count, seeds, **limits)
    return [row[1] for row in rows], [row[2:] for row in rows]


def raw_call(parts, K, min_count, budget=0, clean=None):
    """kv_assemble_batch (clean None) or kv_assemble_clean_batch(tip_nodes, bubble_nodes, clean_rounds) through ctypes: the bytes
    of everything it returns, the unitigs of each partition put in order first.  include/kvsketch.h promises none inside a
    partition: unitigs come in the order of their heads' windows, and which of a key's windows owns it is whichever reached the
    table first.  So what two calls must share is every byte of this serialisation: bases, offsets, partitions, counts per
    partition, stats and clean stats."""
    lib = _lib.load()
    _lib.require_device()
    reads = [seq for part in parts for seq in part]
    read_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    read_off[1:] = np.cumsum(np.array([len(seq) for seq in reads], dtype=np.uint64))
    part_first = np.zeros(len(parts) + 1, dtype=np.uint64)
    part_first[1:] = np.cumsum(np.array([len(part) for part in parts], dtype=np.uint64))
    bases = np.frombuffer(''.join(reads).encode('latin-1'), dtype=np.uint8)
    n_unitigs, n_bases, handle = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_void_p()
    head = [bases.ctypes.data, read_off.ctypes.data, len(reads), part_first.ctypes.data, len(parts), K, min_count, budget]
    tail = [ctypes.byref(n_unitigs), ctypes.byref(n_bases), ctypes.byref(handle)]
    if clean is None:
        _lib.check(lib.kv_assemble_batch(*(head + tail)))
    else:
        _lib.check(lib.kv_assemble_clean_batch(*(head + list(clean) + tail)))
    try:
        text = np.zeros(max(n_bases.value, 1), dtype=np.uint8)
        offsets = np.zeros(n_unitigs.value + 1, dtype=np.uint64)
        part_of = np.zeros(max(n_unitigs.value, 1), dtype=np.uint32)
        counts = np.zeros(max(len(parts), 1), dtype=np.uint32)
        _lib.check(lib.kv_assemble_fetch(handle, text.ctypes.data, offsets.ctypes.data, part_of.ctypes.data, counts.ctypes.data))
        stats = np.zeros(7, dtype=np.uint64)
        _lib.check(lib.kv_assemble_stats(handle, stats.ctypes.data))
        cleaned = np.zeros(5, dtype=np.uint64)
        _lib.check(lib.kv_assemble_clean_stats(handle, cleaned.ctypes.data))
    finally:
        lib.kv_assemble_destroy(handle)
    whole, bounds, where = text[:n_bases.value].tobytes(), offsets.tolist(), part_of[:n_unitigs.value].tolist()
    assert where == sorted(where) and bounds[0] == 0 and bounds[-1] == n_bases.value       # partition after partition
    ordered = sorted((p, whole[bounds[u]:bounds[u + 1]]) for u, p in enumerate(where))
    lengths = np.array([0] + [len(seq) for _, seq in ordered], dtype=np.uint64)
    return (n_unitigs.value, n_bases.value, b''.join(seq for _, seq in ordered), np.cumsum(lengths).astype(np.uint64).tobytes(),
            part_of.tobytes(), counts.tobytes(), stats.tobytes(), cleaned.tobytes())


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [13, 31, 33, 63])
def test_hand_built_cases(hk, K):
    cases = cc.hand_cases(K)
    parts = [reads for reads, _, _ in cases.values()]
    found, stats, clean = cc.agree_clean(parts, K, 2, launches=1)
    for (name, (reads, want, numbers)), mine in zip(cases.items(), found):
        if want is not None:
            assert mine == sorted(want), name       # the answer as it is written out
    assert tuple(clean[n] for n in cc.CLEAN_NAMES[:4]) == tuple(sum(numbers[i] for _, _, numbers in cases.values()) for i in range(4))
    assert clean['rounds'] == 2                     # the tip on an arm takes two, nothing takes more
    # each alone: its own five numbers
    for name, (reads, want, numbers) in cases.items():
        _, _, alone = cc.agree_clean([reads], K, 2)
        assert tuple(alone[n] for n in cc.CLEAN_NAMES) == numbers, name


@pytest.mark.parametrize('min_count', [1, 2])
@pytest.mark.parametrize('K', [13, 31, 33, 63])
def test_300_planted_partitions(hk, K, min_count):
    parts, want = rows_of(K, min_count, range(300))
    found, stats, clean = cc.agree_clean(parts, K, min_count, launches=1, want=want)
    assert clean['tips'] > 40 and clean['arms'] > 100 and clean['rounds'] >= 2 and stats['unitigs'] > 300


def test_in_sevens_and_one_at_a_time(hk):
    parts, want = rows_of(31, 2, range(42))
    for at in range(0, 42, 7):
        cc.agree_clean(parts[at:at + 7], 31, 2, launches=1, want=want[at:at + 7])
    for p in range(0, 42, 3):
        cc.agree_clean(parts[p:p + 1], 31, 2, launches=1, want=want[p:p + 1])


@pytest.mark.parametrize('K', [31, 33])
def test_a_budget_cuts_the_call_and_the_rounds_follow_the_cut(hk, K):
    parts, want = rows_of(K, 2, range(96))
    lengths = [[len(r) for r in reads] for reads in parts]
    sizes = [ac.partition_size(ls, K) for ls in lengths]
    alone = max(cc.clean_launch_bytes(w, b, r, K, True) for w, b, r in sizes)
    seen = set()
    for budget in (alone, 3 * alone, 7 * alone):
        ends = cc.clean_plan(lengths, K, budget, K, 2 * K)
        assert len(ends) > 1
        # the library's own plan entry cuts where the mirror does, and today's entry cuts later
        lib = _lib.load()
        off = np.zeros(sum(len(ls) for ls in lengths) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.array([n for ls in lengths for n in ls], dtype=np.uint64))
        first = np.zeros(len(parts) + 1, dtype=np.uint64)
        first[1:] = np.cumsum(np.array([len(ls) for ls in lengths], dtype=np.uint64))
        got, n = np.zeros(len(parts), dtype=np.uint64), ctypes.c_uint64(0)
        assert lib.kv_assemble_clean_plan(off.ctypes.data, len(off) - 1, first.ctypes.data, len(parts), K, budget, K, 2 * K, 8,
                                          got.ctypes.data, ctypes.byref(n)) == 0
        assert got[:n.value].tolist() == ends
        assert ac.device_plan(parts, K, budget) == (0, ac.plan(lengths, K, budget)) and len(ac.plan(lengths, K, budget)) <= len(ends)
        found, stats, clean = cc.agree_clean(parts, K, 2, mem_budget=budget, launches=len(ends), want=want, launch_ends=ends)
        seen.add(clean['rounds'])
        assert clean['rounds'] == sum(max(w[2]['rounds'] for w in want[a:b]) for a, b in zip([0] + ends, ends))
    assert len(seen) == 3                           # the number follows the cut


def test_no_limits_is_kv_assemble_batch_byte_for_byte(hk):
    for K, min_count, seeds in ((31, 2, range(60)), (33, 1, range(60, 90))):
        parts = [cc.planted_partition(seed, K)[1] for seed in seeds]
        lengths = [[len(r) for r in reads] for reads in parts]
        budget = 4 * max(ac.launch_bytes(*ac.partition_size(ls, K), K) for ls in lengths)
        for b in (0, budget):
            today = raw_call(parts, K, min_count, b)
            assert raw_call(parts, K, min_count, b, clean=(0, 0, 8)) == today
            assert raw_call(parts, K, min_count, b, clean=(0, 0, 0)) == today       # without a limit the rounds say nothing
            assert np.frombuffer(today[7], dtype=np.uint64).tolist() == [0, 0, 0, 0, 0]
            launches = int(np.frombuffer(today[6], dtype=np.uint64)[6])
            assert launches == (1 if b == 0 else len(ac.plan(lengths, K, budget))) and (b == 0 or launches > 1)
        assert raw_call(parts, K, min_count, 0, clean=(K, 2 * K, 8)) != today


@pytest.mark.parametrize('K', [13, 33])
@pytest.mark.parametrize('rounds', [1, 2, 8])
def test_clean_rounds_1_2_and_8(hk, K, rounds):
    parts, want = rows_of(K, 2, range(120), clean_rounds=rounds)
    found, stats, clean = cc.agree_clean(parts, K, 2, clean_rounds=rounds, launches=1, want=want)
    assert clean['rounds'] == max(w[2]['rounds'] for w in want) and (clean['rounds'] == 1) == (rounds == 1)
    eight = rows_of(K, 2, range(120))[1]
    assert ([w[0] for w in want] != [w[0] for w in eight]) == (rounds == 1)


def test_other_limits_than_the_defaults(hk):
    for tip_nodes, bubble_nodes in ((31, 0), (0, 62), (5, 30), (30, 61), (1, 1), (1000, 1000)):
        parts, want = rows_of(31, 2, range(60), tip_nodes=tip_nodes, bubble_nodes=bubble_nodes)
        cc.agree_clean(parts, 31, 2, tip_nodes=tip_nodes, bubble_nodes=bubble_nodes, want=want)


def test_the_same_call_twice_gives_identical_bytes(hk):
    parts = [cc.planted_partition(seed, 33)[1] for seed in range(200)]
    first = raw_call(parts, 33, 2, 0, clean=(33, 66, 8))
    assert first[0] > 200 and np.frombuffer(first[7], dtype=np.uint64)[4] >= 2
    assert raw_call(parts, 33, 2, 0, clean=(33, 66, 8)) == first
    assert raw_call(parts[::-1], 33, 2, 0, clean=(33, 66, 8))[:3] != first[:3]      # (another call: other bytes)


def test_argument_errors(hk):
    parts = [cc.planted_partition(0, 31)[1]]
    for limits in ((31, 62, 0), (1, 0, 0), (0, 1, 0)):
        with pytest.raises(_lib.KvArgError):
            raw_call(parts, 31, 2, 0, clean=limits)
    with pytest.raises(_lib.KvArgError):
        asm.unitigs_batch(parts, 31, 2, tip_nodes=-1)
    lib = _lib.load()
    assert lib.kv_assemble_clean_stats(None, None) != 0


# ---- 2. more heads than one grid covers, and the edges of a wave and of a chunk ---------------------------------------------------
def fork_field(rng, K, components):
    """one partition of many small graphs: a stem of K + 2 bases seen five times, three of them going on with one pair of bases
    and two with another -- 2 nodes a branch, 6 heads, and the weaker branch is a tip"""
    reads = []
    for _ in range(components):
        stem = ac.random_dna(rng, K + 2)
        strong = ac.random_dna(rng, 2)
        weak = cc.other_base(rng, strong[0]) + rng.choice('ACGT')
        reads += [stem + strong] * 3 + [stem + weak] * 2
    return reads


def test_more_heads_than_one_grid(hk):
    K, min_count, repeats = 13, 2, 60
    rng = random.Random(4097)
    distinct = [cc.planted_partition(seed, K)[1] for seed in range(20)] + [fork_field(rng, K, 300) for _ in range(10)]
    answers = [cc.clean_unitigs(reads, K, min_count, K, 2 * K) for reads in distinct]
    assert all(clean['tips'] >= 290 for _, _, clean in answers[20:])
    order = list(range(len(distinct))) * repeats
    rng.shuffle(order)
    parts, want = [distinct[i] for i in order], [answers[i] for i in order]
    # the first round has the heads of the graph before cleaning: measure, decide and kill go round their loops twice
    before = sum(ac.unitigs(distinct[i], K, min_count)[1]['heads'] for i in range(len(distinct))) * repeats
    assert before > ONE_GRID and ac.add_stats([w[1] for w in want])['windows'] > ONE_GRID
    found, stats, clean = cc.agree_clean(parts, K, min_count, launches=1, want=want)
    assert clean['tips'] > 170000 and clean['arms'] > 0


@pytest.mark.parametrize('K', [31, 33])
def test_a_tip_on_the_last_lane_of_a_wave_and_of_a_chunk(hk, K):
    # min_count 1 and a tip seen once: the window that owns the tip's first key is the one window that holds it.  The tip read is
    # K + 1 bases of the haplotype, an error and 3 more: windows 0 and 1 are the haplotype's, window 2 is the tip's head
    rng = random.Random(7 * K)
    parts, at_window = [], []
    windows = 0
    for edge in (63, 255, 511):
        fill = edge - 2 - windows
        assert fill > 0
        parts.append([ac.random_dna(rng, fill + K - 1)])
        hap = ac.random_dna(rng, 3 * K)
        at = 2 * K
        tip = hap[at - K - 1:at] + cc.other_base(rng, hap[at]) + ac.random_dna(rng, 3)
        parts.append([tip, hap, hap])
        at_window.append(windows + fill + 2)
        windows += fill + sum(len(r) - K + 1 for r in parts[-1])
    assert at_window == [63, 255, 511]
    found, stats, clean = cc.agree_clean(parts, K, 1, launches=1)
    assert (clean['tips'], clean['tip_keys'], clean['arms'], clean['rounds']) == (3, 12, 0, 1)
    assert [len(found[p]) for p in (1, 3, 5)] == [1, 1, 1]


# ---- 3. the command line and alac ---------------------------------------------------------------------------------------------------
def stream(path):
    return kevlar_amd.parse_partitioned_reads(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(path, 'r')))


def contig_seqs(text):
    """the sequence lines of augmented Fasta: the line behind every name"""
    lines = text.split('\n')
    return [lines[i + 1] for i, ln in enumerate(lines) if ln.startswith('>')]


def cc2_contig():
    reads = ac.all_reads(CC2)
    found = ac.contigs_of(cc.clean_unitigs(reads, 31, 2, 31, 62)[0], reads)
    assert [len(c) for c in found] == [337]
    return found[0]


def test_assemble_clean_through_the_command_line(hk, tmp_path):
    out_file = str(tmp_path / 'contigs.augfasta')
    done = subprocess.run([sys.executable, '-m', 'kevlar_amd', 'assemble', '--clean', '-o', out_file, ac.fixture_path(CC2)], cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr
    assert contig_seqs(open(out_file).read()) == [cc2_contig()]
    assert 'assembled 1 contigs; cleaning removed 3 tips (34 k-mers) and 0 bubble arms (0 k-mers)' in done.stderr


def test_assemble_flags_reach_the_device(hk, capsys, kevlar_log):
    path = ac.fixture_path(CC2)
    for flags, lengths in (([], [165, 162]), (['--clean'], [337]), (['--tip-nodes', '15'], [202, 165]), (['--tip-nodes', '31'], [337]),
                           (['--clean', '--tip-nodes', '0'], [165, 162]), (['--bubble-nodes', '62'], [165, 162])):
        kevlar_amd.cli.run(['assemble'] + flags + [path])
        out, err = capsys.readouterr()
        assert [len(seq) for seq in contig_seqs(out)] == lengths, flags
        assert ('cleaning removed' in kevlar_log.getvalue() + err) == bool(flags)
        kevlar_log.truncate(0)
        kevlar_log.seek(0)
    found = [contig.sequence for _, contig in asm.assemble(stream(path), tip_nodes=31, bubble_nodes=62)]
    assert found == [cc2_contig()]
    triples = list(asm.assemble_partitions(stream(path), tip_nodes=31, bubble_nodes=62, clean_rounds=1))
    assert [t[2] for t in triples] == [[cc2_contig()]]


def test_alac_on_cc2_with_cleaning(hk):
    # what is observed, see DESIGN.md section 13
    row = [r for r in ac.recorded()['pico_calls'] if r['cc'] == 2][0]
    calls = list(alac(stream(ac.fixture_path(CC2)), PICO_REFR, ksize=25, delta=50, tip_nodes=31, bubble_nodes=62))
    assert [(c.seqid, c._pos, c._refr, c._alt) for c in calls] == [('seq1', row['pos'], row['ref'], row['alt'])]
    # and off, as before
    calls = list(alac(stream(ac.fixture_path(CC2)), PICO_REFR, ksize=25, delta=50))
    assert [(c._pos, c.filterstr) for c in calls] == [(834515, 'InscrutableCigar')]
