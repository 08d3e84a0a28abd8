"""The rate of the batched assembly of `kevlar assemble` (kevlar_amd/csrc/kv_assemble.hip): seeded synthetic partitions -- 30 reads
of 150 bases tiled at random over a 400-base haplotype, either strand, 1 % substitutions -- 20 000 of them in one call.  The
contigs of a sample of the partitions are checked against the plain-Python restatement first (tests/assemble_common.py), then one
warm-up call and five timed ones: every kernel by the library's events (kv_prof), the whole call -- uploads, the three read-backs
and the copy of the unitigs included -- by the host clock, the card's clock and power sampled beside them.  Then the same with
--clean's limits (tips of at most K nodes, arms of at most 2K, 8 rounds) in the same process: the unitigs of the sample against
tests/asmclean_common.py, one warm-up call and five timed ones, the rounds run and the keys removed beside the times.  DESIGN.md
section 13.  `python scratch/assemble_rate.py [partitions] [sample]`"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
torch.cuda.init()
from kevlar_amd import _lib
from kevlar_amd import assemble as asm
from bench import ClockWatch
import assemble_common as ac
import asmclean_common as cc
lib = _lib.load(); _lib.require_device()
K, MIN_COUNT, READS, READ_LEN, HAP_LEN, ERROR = 31, 2, 30, 150, 400, 0.01
PARTS = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
SAMPLE = int(sys.argv[2]) if len(sys.argv) > 2 else 50
KERNELS = ('k_asm_keys', 'k_asm_group', 'k_asm_degree', 'k_asm_heads', 'k_asm_scan', 'k_asm_walk_len', 'k_asm_walk_write')
CLEAN_KERNELS = ('k_asm_measure', 'k_asm_decide', 'k_asm_kill')
rng = np.random.default_rng(13)
letters = np.frombuffer(b'ACGT', dtype=np.uint8)
comp = np.zeros(256, dtype=np.uint8); comp[list(b'ACGT')] = list(b'TGCA')
# all partitions at once: haplotypes, read starts, substitutions (a substituted base always changes), strands
haps = letters[rng.integers(0, 4, size=(PARTS, HAP_LEN), dtype=np.uint8)]
starts = rng.integers(0, HAP_LEN - READ_LEN + 1, size=(PARTS, READS))
reads = haps[np.arange(PARTS)[:, None, None], starts[:, :, None] + np.arange(READ_LEN)[None, None, :]]
hit = rng.random(reads.shape) < ERROR
codes = np.searchsorted(letters, reads)
reads = np.where(hit, letters[(codes + rng.integers(1, 4, size=reads.shape)) % 4], reads)
flip = rng.random((PARTS, READS)) < 0.5
reads = np.where(flip[:, :, None], comp[reads[:, :, ::-1]], reads).astype(np.uint8)
flat = reads.reshape(PARTS * READS, READ_LEN)
partitions = [[row.tobytes().decode() for row in flat[p * READS:(p + 1) * READS]] for p in range(PARTS)]

def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value, cnt.value

found, stats = asm.unitigs_batch(partitions, K, MIN_COUNT)
for p in range(0, PARTS, max(PARTS // SAMPLE, 1)):      # the contigs of a sample against the restatement
    want, _ = ac.unitigs(partitions[p], K, MIN_COUNT)
    assert sorted(found[p]) == want, p
    assert asm.contigs_of(found[p], partitions[p]) == ac.contigs_of(want, partitions[p]), p
contigs = sum(len(asm.contigs_of(found[p], partitions[p])) for p in range(PARTS))
print('stats {}, contigs {}'.format(stats, contigs), flush=True)
lib.kv_prof_enable(1)
# the device call alone, on arrays built once: what the wrapper adds (joining and slicing Python strings) is reported beside it
seqs = [seq for part in partitions for seq in part]
read_off = np.arange(len(seqs) + 1, dtype=np.uint64) * READ_LEN
part_first = np.arange(PARTS + 1, dtype=np.uint64) * READS
bases = np.frombuffer(''.join(seqs).encode('latin-1'), dtype=np.uint8)


def measure(kernels, limits):
    """(per kernel: the five readings, the five calls by the host clock, unitig bases, clean stats, clock) of kv_assemble_clean_batch"""
    kernel_ms, call_ms, watch = {name: [] for name in kernels}, [], None
    for rep in range(6):            # the first is a warm-up with the profiler's events on
        if rep == 1:
            watch = ClockWatch(0)
        lib.kv_prof_reset()
        n_unitigs, n_bases, handle = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.kv_assemble_clean_batch(bases.ctypes.data, read_off.ctypes.data, len(seqs), part_first.ctypes.data, PARTS, K, MIN_COUNT,
                                               0, limits[0], limits[1], 8, ctypes.byref(n_unitigs), ctypes.byref(n_bases), ctypes.byref(handle)))
        t1 = time.perf_counter()
        removed = np.zeros(5, dtype=np.uint64)
        lib.kv_assemble_clean_stats(handle, removed.ctypes.data)
        lib.kv_assemble_destroy(handle)
        if rep:
            call_ms.append(round((t1 - t0) * 1e3, 3))
            for name in kernels:
                kernel_ms[name].append(round(prof(name)[0], 3))
    return kernel_ms, call_ms, n_bases.value, dict(zip(asm.CLEAN_NAMES, removed.tolist())), watch.stop()


kernel_ms, call_ms, unitig_bases, _, clock = measure(KERNELS, (0, 0))
t0 = time.perf_counter(); asm.unitigs_batch(partitions, K, MIN_COUNT); wrapper = (time.perf_counter() - t0) * 1e3
median = {name: float(np.median(ms)) for name, ms in kernel_ms.items()}
total = sum(median.values())
windows = stats['windows']
print(json.dumps({'partitions': PARTS, 'reads_per_partition': READS, 'read_len': READ_LEN, 'ksize': K, 'min_count': MIN_COUNT,
                  'stats': stats, 'contigs': contigs, 'unitig_bases': unitig_bases, 'kernel_ms': kernel_ms, 'kernel_ms_median': median,
                  'kernels_ms_total': total, 'call_ms': call_ms, 'call_ms_median': float(np.median(call_ms)),
                  'wrapper_call_ms': round(wrapper, 1),
                  'partitions_per_s': {'kernels': PARTS / (total * 1e-3), 'call': PARTS / (float(np.median(call_ms)) * 1e-3)},
                  'windows_per_s': dict({name: windows / (ms * 1e-3) for name, ms in median.items() if ms > 0},
                                        kernels=windows / (total * 1e-3), call=windows / (float(np.median(call_ms)) * 1e-3)),
                  'clock': clock}), flush=True)

# ---- the same with --clean's limits ----------------------------------------------------------------------------------------------
limits = asm.clean_limits(K)
found, stats = asm.unitigs_batch(partitions, K, MIN_COUNT, tip_nodes=limits[0], bubble_nodes=limits[1])
for p in range(0, PARTS, max(PARTS // SAMPLE, 1)):
    want, _, _ = cc.clean_unitigs(partitions[p], K, MIN_COUNT, limits[0], limits[1])
    assert sorted(found[p]) == want, p
contigs = sum(len(asm.contigs_of(found[p], partitions[p])) for p in range(PARTS))
kernel_ms, call_ms, unitig_bases, removed, clock = measure(KERNELS + CLEAN_KERNELS, limits)
median = {name: float(np.median(ms)) for name, ms in kernel_ms.items()}
total = sum(median.values())
print(json.dumps({'clean': {'tip_nodes': limits[0], 'bubble_nodes': limits[1], 'clean_rounds': 8}, 'stats': stats, 'removed': removed,
                  'contigs': contigs, 'unitig_bases': unitig_bases, 'kernel_ms': kernel_ms, 'kernel_ms_median': median,
                  'kernels_ms_total': total, 'call_ms': call_ms, 'call_ms_median': float(np.median(call_ms)),
                  'partitions_per_s': {'kernels': PARTS / (total * 1e-3), 'call': PARTS / (float(np.median(call_ms)) * 1e-3)},
                  'clock': clock}), flush=True)
