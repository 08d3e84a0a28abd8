"""The rate of the seed scan of `kevlar localize` (k_loc_scan, kevlar_amd/csrc/kv_localize.hip): 256 Mb of random A/C/G/T against
1 M seeds of length 51, 10 % of them cut from the text (every other one reverse-complemented), seeded.  The matches are checked
first (every planted seed is found where it was cut), then one warm-up scan and five timed ones: the kernel by the library's
events (kv_prof, summed over the chunks of a scan), the whole call -- uploads included -- by the host clock, the card's clock
sampled beside them.  DESIGN.md section 9.  `python scratch/localize_scan_rate.py [megabases] [seeds]`"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()
from kevlar_amd import _lib
from kevlar_amd.localize import SeedSet, DEFAULT_CHUNK_BYTES
from bench import ClockWatch
lib = _lib.load(); _lib.require_device()
Z = 51
N = (int(sys.argv[1]) if len(sys.argv) > 1 else 256) * 1000000
SEEDS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
PLANTED = SEEDS // 10
rng = np.random.default_rng(51)
letters = np.frombuffer(b'ACGT', dtype=np.uint8)
comp = np.zeros(256, dtype=np.uint8); comp[list(b'ACGT')] = list(b'TGCA')
text = letters[rng.integers(0, 4, size=N, dtype=np.uint8)]
starts = np.sort(rng.choice(N - Z, size=PLANTED, replace=False))
planted = text[starts[:, None] + np.arange(Z)[None, :]]
planted[1::2] = comp[planted[1::2, ::-1]]
rows = np.concatenate([planted, letters[rng.integers(0, 4, size=(SEEDS - PLANTED, Z), dtype=np.uint8)]])
seeds = [row.tobytes().decode() for row in rows]

def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value, cnt.value

with SeedSet(seeds, Z) as seedset:
    before = seedset.stats()
    ids, pos = seedset.scan(text)
    after = seedset.stats()
    # every planted seed is reported at the position it was cut from, by the id of its own window (or of an equal seed's)
    found = set(zip(seedset.seed_of_window[ids].tolist(), pos.tolist()))
    assert len(found) == len(ids), 'a match was reported twice'
    missing = [int(s) for n, s in enumerate(starts.tolist()) if (int(seedset.seed_of_window[n]), s) not in found]
    assert not missing, missing[:5]
    valid, passed, matched = (after[i] - before[i] for i in range(3))
    print('matches {} (planted {}), windows {}, past the prefilter {}'.format(len(ids), PLANTED, valid, passed), flush=True)
    lib.kv_prof_enable(1)
    kernel_ms, call_ms, launches = [], [], 0
    watch = None
    for rep in range(6):            # the first is a warm-up with the profiler's events on
        if rep == 1:
            watch = ClockWatch(0)
        lib.kv_prof_reset()
        t0 = time.perf_counter(); seedset.scan(text); t1 = time.perf_counter()
        ms, launches = prof('k_loc_scan')
        if rep:
            kernel_ms.append(round(ms, 3)); call_ms.append(round((t1 - t0) * 1e3, 3))
    clock = watch.stop()
k = float(np.median(kernel_ms))
print(json.dumps({'bases': N, 'seeds': SEEDS, 'distinct_seeds': after[3], 'seedsize': Z, 'chunk_bytes': DEFAULT_CHUNK_BYTES,
                  'launches_per_scan': launches, 'kernel_ms': kernel_ms, 'kernel_ms_median': k, 'call_ms': call_ms,
                  'call_ms_median': float(np.median(call_ms)), 'bases_per_s': N / (k * 1e-3), 'text_bytes_per_s': N / (k * 1e-3),
                  'prefilter_pass_share': passed / valid, 'match_share': matched / valid, 'matches': len(ids), 'clock': clock}), flush=True)
