"""The rate of contig-to-cutout alignment (k_align, kevlar_amd/csrc/kv_align.hip) on a batch shaped like one `kevlar call` run:
1 000 seeded pairs on both strands = 2 000 jobs, targets of 300 to 10 000 bases, queries of 200 to 3 000 cut from their target
with 1 % substitutions and a 30-base deletion.  A few jobs are checked first (scores symmetric in the obvious way, CIGAR lengths
add up), then one warm-up batch and five timed ones: the kernels by the library's events (kv_prof, summed over the launches of a
batch), the whole call -- uploads, CIGAR strings -- by the host clock, the card's clock sampled beside them; then the single
10 000 x 3 000 job alone, the latency of one wave.  The share of the traceback is the share of the waves' own time (the device's
100 MHz counter, summed over the jobs) spent after the fill.  DESIGN.md section 10.

`python scratch/align_rate.py [pairs]` on the GPU; `python scratch/align_rate.py --reference [pairs]` times the reference's own
align() on one host core over the same batch (build machine only: compiles it as tests/golden/make_golden_align.py does)."""
import json, os, re, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith('--')]
PAIRS = int(args[0]) if args else 1000
rng = np.random.default_rng(2024)
letters = np.frombuffer(b'ACGT', dtype=np.uint8)
targets, queries = [], []
for _ in range(PAIRS):
    tlen, qlen = int(rng.integers(300, 10001)), int(rng.integers(200, 3001))
    t = letters[rng.integers(0, 4, size=tlen, dtype=np.uint8)]
    start = int(rng.integers(0, max(tlen - qlen - 30, 0) + 1))
    q = np.resize(t[start:start + qlen + 30], qlen + 30).copy()
    hit = rng.random(qlen + 30) < 0.01
    q[hit] = letters[rng.integers(0, 4, size=int(hit.sum()), dtype=np.uint8)]
    q = np.concatenate([q[:qlen // 2], q[qlen // 2 + 30:]])
    targets.append(t.tobytes().decode()); queries.append(q.tobytes().decode())
cells = 2 * sum(len(t) * len(q) for t, q in zip(targets, queries))
pairs = [(k, k) for k in range(PAIRS)]
big_t = letters[rng.integers(0, 4, size=10000, dtype=np.uint8)].tobytes().decode()
big_q = big_t[3500:5000] + big_t[5030:6530]


def cigar_spans(cigar):
    runs = [(int(n), op) for n, op in re.findall(r'(\d+)([MID])', cigar)]
    return sum(n for n, op in runs if op in 'MD'), sum(n for n, op in runs if op in 'MI')


if '--reference' in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import tempfile
    import make_golden_align
    align = make_golden_align.compile_reference(tempfile.mkdtemp(prefix='kevlar-align-'))
    comp = str.maketrans('ACGT', 'TGCA')
    t0 = time.perf_counter(); align(big_t, big_q); t1 = time.perf_counter()
    print(json.dumps({'host_one_job_s': t1 - t0, 'host_one_job_cells_per_s': len(big_t) * len(big_q) / (t1 - t0)}), flush=True)
    t0 = time.perf_counter()
    for t, q in zip(targets, queries):
        align(t, q); align(t, q.translate(comp)[::-1])
    t1 = time.perf_counter()
    print(json.dumps({'pairs': PAIRS, 'jobs': 2 * PAIRS, 'cells': cells, 'host_s': t1 - t0, 'host_cells_per_s': cells / (t1 - t0)}), flush=True)
    sys.exit(0)

import ctypes
import torch
torch.cuda.init()
from kevlar_amd import _lib, alignment
from bench import ClockWatch
lib = _lib.load(); _lib.require_device()


def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value, cnt.value


def timed(run, reps=6):
    """the first repetition is a warm-up with the profiler's events on"""
    kernel_ms, call_ms, stats = [], [], None
    for rep in range(reps):
        lib.kv_prof_reset()
        t0 = time.perf_counter(); run(); t1 = time.perf_counter()
        ms, _ = prof('k_align')
        stats = alignment.last_stats()
        if rep:
            kernel_ms.append(round(ms, 3)); call_ms.append(round((t1 - t0) * 1e3, 3))
    return kernel_ms, call_ms, stats


found = alignment.align_batch(targets, queries, pairs)
for (score, cigar, strand), t, q in zip(found, targets, queries):
    assert cigar_spans(cigar) == (len(t), len(q)), 'a CIGAR does not span its sequences'
    assert len(t) < len(q) + 30 or (strand == 1 and score > len(q) // 2), 'a query cut from its target should align forward'
lib.kv_prof_enable(1)
watch = ClockWatch(0)
kernel_ms, call_ms, stats = timed(lambda: alignment.align_batch(targets, queries, pairs))
one_kernel_ms, one_call_ms, one_stats = timed(lambda: alignment.align_batch([big_t], [big_q], [(0, 0)], both_strands=False))
clock = watch.stop()
k, k1 = float(np.median(kernel_ms)), float(np.median(one_kernel_ms))
print(json.dumps({'pairs': PAIRS, 'jobs': 2 * PAIRS, 'cells': cells, 'launches': stats[0], 'z_budget': alignment.DEFAULT_Z_BUDGET,
                  'kernel_ms': kernel_ms, 'kernel_ms_median': k, 'call_ms': call_ms, 'call_ms_median': float(np.median(call_ms)),
                  'cells_per_s_kernels': cells / (k * 1e-3), 'cells_per_s_call': cells / (float(np.median(call_ms)) * 1e-3),
                  'traceback_share_of_wave_time': stats[2] / (stats[1] + stats[2]),
                  'mean_wave_ms': (stats[1] + stats[2]) / 1e5 / (2 * PAIRS),
                  'one_job_cells': len(big_t) * len(big_q), 'one_job_kernel_ms': one_kernel_ms, 'one_job_kernel_ms_median': k1,
                  'one_job_call_ms_median': float(np.median(one_call_ms)), 'one_job_cells_per_s': len(big_t) * len(big_q) / (k1 * 1e-3),
                  'one_job_traceback_share': one_stats[2] / (one_stats[1] + one_stats[2]), 'clock': clock}), flush=True)
