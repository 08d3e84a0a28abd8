"""The rate of `kevlar varfilter` (k_vf_scan, kevlar_amd/csrc/kv_varfilter.hip): a seeded BED of 20 M lines over 24 chromosomes against
10 000 calls.  The flags are checked first against a numpy restatement of the join (sorted starts; no call is longer than 50 bases),
then one warm-up and seven timed scans of the text resident on the device and of the text in host memory: the kernel by the
library's events (kv_prof, summed over the chunks), the whole call by the host clock.  Beside it the command's wall time on the
same file, and the host generator parse_bed joined by bisect on it.  DESIGN.md section 14.
`python scratch/varfilter_rate.py [lines] [calls] [host_lines] [scan-only]` (host_lines: how many lines the Python baseline reads,
0 = all; scan-only: stop behind the scans, for A/B libraries under KV_LIB_PATH)"""
import bisect, ctypes, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()
import kevlar_amd
from kevlar_amd import _lib, varfilter
lib = _lib.load(); _lib.require_device()
LINES = int(sys.argv[1]) if len(sys.argv) > 1 else 20000000
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
HOST_LINES = int(sys.argv[3]) if len(sys.argv) > 3 else 0
CHUNK = varfilter.DEFAULT_CHUNK_BYTES
rng = np.random.default_rng(14)
names = ['chr{}'.format(i) for i in range(1, 23)] + ['chrX', 'chrY']
sizes = np.linspace(248e6, 50e6, len(names)).astype(np.int64)


def digits(values):
    return np.searchsorted(10 ** np.arange(1, 19, dtype=np.int64), values, side='right') + 1


def put_number(out, at, values, width):
    """the decimal digits of values[i] at out[at[i] ..], width[i] of them"""
    for k in range(int(width.max())):
        mask = width > k
        out[at[mask] + width[mask] - 1 - k] = 48 + (values[mask] // 10 ** k) % 10


def bed_text(chrom, start, end):
    name_bytes = np.zeros((len(names), 8), dtype=np.uint8)
    name_len = np.array([len(n) for n in names])
    for i, n in enumerate(names):
        name_bytes[i, :len(n)] = list(n.encode())
    nl, ds, de = name_len[chrom], digits(start), digits(end)
    at = np.concatenate([[0], np.cumsum(nl + ds + de + 3)])
    out = np.empty(at[-1], dtype=np.uint8)
    at = at[:-1]
    for k in range(int(name_len.max())):
        mask = nl > k
        out[at[mask] + k] = name_bytes[chrom[mask], k]
    out[at + nl] = 9
    put_number(out, at + nl + 1, start, ds)
    out[at + nl + 1 + ds] = 9
    put_number(out, at + nl + ds + 2, end, de)
    out[at + nl + ds + de + 2] = 10
    return out


t0 = time.perf_counter()
weights = sizes / sizes.sum()
call_chrom = rng.choice(len(names), size=CALLS, p=weights)
call_start = (rng.random(CALLS) * sizes[call_chrom]).astype(np.int64)
call_end = call_start + np.where(rng.random(CALLS) < 0.9, 1, rng.integers(2, 50, size=CALLS))
chrom = np.sort(rng.choice(len(names), size=LINES, p=weights))                       # a BED sorted by chromosome and start, as the tracks are
start = (rng.random(LINES) * sizes[chrom]).astype(np.int64)
order = np.lexsort((start, chrom))
chrom, start = chrom[order], start[order]
end = start + rng.integers(1, 3000, size=LINES)
text = bed_text(chrom, start, end)
print('generated {} lines, {} bytes ({:.1f} per line) in {:.1f} s'.format(LINES, len(text), len(text) / LINES, time.perf_counter() - t0), flush=True)

# the restatement: per chromosome, calls sorted by start; a region hits the calls in front of its end whose end lies behind its start
want = np.zeros(CALLS, dtype=bool)
n_overlaps = 0
for c in range(len(names)):
    calls_c = np.flatnonzero(call_chrom == c)
    calls_c = calls_c[np.argsort(call_start[calls_c], kind='stable')]
    a, b = call_start[calls_c], call_end[calls_c]
    rows = chrom == c
    s, e = start[rows], end[rows]
    hi = np.searchsorted(a, e, side='left')                 # calls with a < e
    lo = np.searchsorted(a, s - 50, side='left')            # no call is longer than 50: those in front of lo end at or before s
    for width in range(int((hi - lo).max()) if len(s) else 0):
        j = lo + width
        ok = j < hi
        hit = ok.copy()
        hit[ok] = b[j[ok]] > s[ok]
        n_overlaps += int(hit.sum())
        want[calls_c[j[hit]]] = True
print('restatement: {} overlaps, {} of {} calls flagged'.format(n_overlaps, int(want.sum()), CALLS), flush=True)

regions = [(names[c], int(a), int(b)) for c, a, b in zip(call_chrom, call_start, call_end)]


def pieces(array):
    cuts, at = [], 0
    while at < len(array):
        stop = min(at + CHUNK, len(array))
        while stop < len(array) and array[stop - 1] != 10:
            stop -= 1
        cuts.append((at, stop))
        at = stop
    return cuts


def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value, cnt.value


cuts = pieces(text)
resident = torch.from_numpy(text).cuda()
torch.cuda.synchronize()
result = {'lines': LINES, 'calls': CALLS, 'bytes': int(len(text)), 'chunks': len(cuts), 'lib': os.path.basename(_lib.LIBPATH)}
plan = (ctypes.c_uint64 * 5)()
lib.kv_varfilter_plan(cuts[0][1] - cuts[0][0], plan)
result['tile_bytes'] = int(plan[0])
with varfilter.CallIndex(regions) as index:
    handle = index._handle
    lib.kv_prof_enable(1)
    for where in ('device', 'host'):
        kernel_ms, call_ms = [], []
        for rep in range(8):                                # the first is a warm-up
            lib.kv_prof_reset()
            t0 = time.perf_counter()
            for at, stop in cuts:
                pointer = resident.data_ptr() + at if where == 'device' else text.ctypes.data + at
                _lib.check(lib.kv_varfilter_scan(handle, ctypes.c_void_p(pointer), stop - at, at))
            t1 = time.perf_counter()
            if rep:
                kernel_ms.append(round(prof('k_vf_scan')[0], 3)); call_ms.append(round((t1 - t0) * 1e3, 3))
        k, c = float(np.median(kernel_ms)), float(np.median(call_ms))
        result[where] = {'kernel_ms': kernel_ms, 'kernel_ms_median': k, 'call_ms': call_ms, 'call_ms_median': c,
                         'lines_per_s_kernel': round(LINES / (k * 1e-3)), 'lines_per_s_call': round(LINES / (c * 1e-3)),
                         'GB_per_s_kernel': round(len(text) / (k * 1e-3) / 1e9, 1)}
        print(where, json.dumps(result[where]), flush=True)
    stats = index.stats()
    flags = index.hits().astype(bool)
    assert np.array_equal(flags, want), 'flags differ from the restatement'
    assert stats['lines'] == stats['regions'] == stats['known'] == 16 * LINES and stats['overlaps'] == 16 * n_overlaps, stats
    result['overlaps'], result['flagged'] = n_overlaps, int(want.sum())
del resident
if sys.argv[4:5] == ['scan-only']:
    print(json.dumps(result))
    sys.exit(0)

# the command on the same file, and the host generator joined by bisect
with tempfile.TemporaryDirectory() as tmp:
    bed, vcf, out = os.path.join(tmp, 'mask.bed'), os.path.join(tmp, 'calls.vcf'), os.path.join(tmp, 'out.vcf')
    text.tofile(bed)
    with open(vcf, 'w') as stream:
        writer = kevlar_amd.vcf.VCFWriter(stream)
        writer.write_header()
        for name, a, b in regions:
            writer.write(kevlar_amd.vcf.Variant(name, a, 'A' * (b - a), 'C'))
    cli = []
    for rep in range(4):
        t0 = time.perf_counter()
        subprocess.check_call([sys.executable, '-m', 'kevlar_amd', 'varfilter', '-o', out, bed, vcf], cwd=ROOT, stderr=subprocess.DEVNULL)
        cli.append(round(time.perf_counter() - t0, 2))
    result['cli_wall_s'] = cli
    filtered = sum('\tUserFilter\t' in line for line in open(out))
    assert filtered == int(want.sum()), filtered
    t0 = time.perf_counter(); n = len(open(bed, 'rb').read()); result['file_read_s'] = round(time.perf_counter() - t0, 3)
    print('cli', cli, 'file read', result['file_read_s'], flush=True)

    by_chrom = {}
    for number, (name, a, b) in enumerate(regions):
        by_chrom.setdefault(name, []).append((a, b, number))
    tables = {name: (sorted(rows), [row[0] for row in sorted(rows)]) for name, rows in by_chrom.items()}
    host_flags = np.zeros(CALLS, dtype=bool)
    t0 = time.perf_counter()
    done = 0
    with open(bed, 'rb') as stream:
        for name, s, e, _ in kevlar_amd.parse_bed(stream):
            rows, starts = tables.get(name, ((), ()))
            j = bisect.bisect_left(starts, e)
            while j > 0 and starts[j - 1] > s - 50:
                j -= 1
                if rows[j][1] > s:
                    host_flags[rows[j][2]] = True
            done += 1
            if done == HOST_LINES:
                break
    host_s = time.perf_counter() - t0
    if done == LINES:
        assert np.array_equal(host_flags, want)
    result['host_parse_bed_bisect'] = {'lines': done, 'seconds': round(host_s, 2), 'lines_per_s': round(done / host_s)}
print(json.dumps(result))
