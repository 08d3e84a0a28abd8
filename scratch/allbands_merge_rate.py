"""kv_hits_merge (merge by rank, full-width key) against kv_hits_from_tagged (rocPRIM radix sort of read << 16 | offset tags) for one
batch of cfg4-band's shape: 8 runs x 2.5 M hits, S = 3, seeded; outputs compared first, then five alternated repetitions, the kernels
timed by the library's events (kv_prof) and the whole call by the host clock.  DESIGN.md section 7.  `python scratch/allbands_merge_rate.py`"""
import ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()
from kevlar_amd import _lib, khmer as hk
lib = _lib.load(); _lib.require_device()
R, PER, S = 8, 2500000, 3
n = R * PER
rng = np.random.default_rng(2024)
keys = np.unique((rng.integers(0, 1 << 23, size=n + n // 8, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 70, size=n + n // 8, dtype=np.uint64))
keys = keys[rng.permutation(len(keys))[:n]]
owner = np.repeat(np.arange(R), PER)
order = np.lexsort((keys, owner)); keys = keys[order]
read = (keys >> np.uint64(32)).astype(np.uint32); offset = (keys & np.uint64(0xffffffff)).astype(np.uint32)
abund = rng.integers(0, 256, size=(n, S), dtype=np.uint8)
starts = (np.arange(R + 1) * PER).astype(np.uint64)
tags = (read.astype(np.int64) << 16) | offset.astype(np.int64)
d_read = torch.from_numpy(read.view(np.int32)).cuda(); d_off = torch.from_numpy(offset.view(np.int32)).cuda()
d_abund = torch.from_numpy(abund).cuda(); d_tags = torch.from_numpy(tags).cuda()
torch.cuda.synchronize()

def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value

def merge():
    return hk.hits_merge(d_read.data_ptr(), d_off.data_ptr(), d_abund.data_ptr(), starts, S)

def tagged():
    return hk.hits_from_tagged(d_tags.data_ptr(), d_abund.data_ptr(), n, n, S)

a = merge(); b = tagged()
want = np.lexsort((offset, read))
same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[0], read[want]) and np.array_equal(a[2], abund[want]))
print('outputs equal:', same, flush=True)
assert same
del a, b
lib.kv_prof_enable(1)
res = {'merge': {'device_ms': [], 'call_ms': []}, 'tagged': {'device_ms': [], 'call_ms': []}}
for rep in range(6):          # the first pair is a warm-up with the profiler's events on
    for name, fn, scope in (('merge', merge, 'merge_hits'), ('tagged', tagged, 'sort_hits')):
        lib.kv_prof_reset()
        t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
        del out
        if rep:
            res[name]['device_ms'].append(round(prof(scope), 3)); res[name]['call_ms'].append(round((t1 - t0) * 1e3, 3))
for name in res:
    for key in ('device_ms', 'call_ms'):
        v = res[name][key]
        res[name][key + '_median'] = float(np.median(v)); res[name][key + '_min_max'] = [min(v), max(v)]
print(json.dumps({'hits': n, 'runs': R, 'S': S, **res}), flush=True)
