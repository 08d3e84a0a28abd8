"""What `kevlar call` costs behind the alignment (k_call_scan, kevlar_amd/csrc/kv_call.hip): the six partitions of
tests/golden/call/homopolymer/14153-6parts, copied (fresh records, fresh partition ids) until the run has about 20 000
(contig, cutout, strand) jobs to scan.

1. The jobs are aligned once (not timed here), then scanned: one warm-up batch and five timed ones, the kernel by the library's
   events (kv_prof), the whole scan_batch call -- runs parsed from the CIGAR strings, uploads, records back -- by the host clock
   around it (the call ends in a synchronise), the card's clock sampled beside them.  Every record of the first batch is compared
   with the restatement's.
2. The baseline: tests/call_common.py's plain-Python restatement of the same jobs on one host core.
3. The whole call_partitions, three times after a warm-up, split as kevlar_amd.call.last_timing splits it: alignment, scan,
   and the host's assembly of Variant objects, de-duplication and merging.

`python scratch/call_rate.py [jobs]` on the GPU.  DESIGN.md section 11."""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
torch.cuda.init()
import kevlar_amd
import kevlar_amd.call
from kevlar_amd import _lib, alignment, varmap
from kevlar_amd.sequence import Record
from kevlar_amd.reference import ReferenceCutout
from bench import ClockWatch
import call_common as cc

WANTED = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
KSIZE, MINDIST = 31, 5
lib = _lib.load(); _lib.require_device()
kevlar_amd.logstream = open(os.devnull, 'w')
parts = cc.load_partitions(cc.FIXTURE_BY_NAME['homopolymer-14153'], kevlar_amd)
per_copy = sum(len(cutouts) * len(contigs) for partid, cutouts, contigs in parts)
copies = max(1, round(WANTED / per_copy))
contigs_by_partition, cutouts_by_partition = {}, []
for n in range(copies):
    for partid, cutouts, contigs in parts:
        label = '{}c{}'.format(partid, n)
        contigs_by_partition[label] = [Record(r.name, r.sequence, annotations=list(r.annotations)) for r in contigs]
        cutouts_by_partition.append((label, [ReferenceCutout(c.defline, c.sequence) for c in cutouts]))


def prof(name):
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value


# ---- 1. the scan of one batch
rows = list(alignment.align_partitions(list(contigs_by_partition.items()), cutouts_by_partition))
targets, queries, notes, jobs, cigars, at = [], [], [], [], [], {}
for partid, contig, cutout, score, cigar, strand in rows:
    for item, pool in ((cutout, targets), (contig, queries)):
        if id(item) not in at:
            at[id(item)] = len(pool)
            pool.append(item.sequence)
            if pool is queries:
                notes.append(varmap.contig_annotations(contig))
    jobs.append((at[id(cutout)], at[id(contig)], int(strand == -1)))
    cigars.append(cigar)
aligned_bases = sum(int(n) for cigar in cigars for n, op in varmap.cigar_blocks(cigar) if op == 'M')
lib.kv_prof_enable(1)
watch = ClockWatch(0)
kernel_ms, call_ms = [], []
for rep in range(6):
    lib.kv_prof_reset()
    t0 = time.perf_counter(); got = varmap.scan_batch(targets, queries, jobs, cigars, notes, KSIZE, MINDIST); t1 = time.perf_counter()
    if rep:
        kernel_ms.append(round(prof('k_call_scan'), 3)); call_ms.append(round((t1 - t0) * 1e3, 3))
clock = watch.stop()
lib.kv_prof_enable(0)

# ---- 2. the same jobs through the restatement, one host core
t0 = time.perf_counter()
wanted = [cc.job_record(targets[t], queries[q], rev, cigar, notes[q], KSIZE, MINDIST) for (t, q, rev), cigar in zip(jobs, cigars)]
host_s = time.perf_counter() - t0
assert [record.astuple() for record in got] == wanted, 'the device scan differs from the restatement'
print(json.dumps({'jobs': len(jobs), 'copies': copies, 'targets': len(targets), 'queries': len(queries), 'aligned_bases': aligned_bases,
                  'annotations': int(sum(len(n) for n in notes)), 'calls_with_a_window': int(sum(1 for r in wanted for w in r[16:25] if w)),
                  'kernel_ms': kernel_ms, 'kernel_ms_median': float(np.median(kernel_ms)), 'scan_call_ms': call_ms,
                  'scan_call_ms_median': float(np.median(call_ms)), 'restatement_one_core_s': round(host_s, 3),
                  'restatement_over_kernel': host_s / (float(np.median(kernel_ms)) * 1e-3),
                  'restatement_over_scan_call': host_s / (float(np.median(call_ms)) * 1e-3), 'clock': clock}), flush=True)

# ---- 3. the whole of call_partitions
watch = ClockWatch(0)
splits = []
for rep in range(4):
    t0 = time.perf_counter()
    ncalls = sum(1 for _ in kevlar_amd.call.call_partitions(contigs_by_partition, cutouts_by_partition, ksize=KSIZE, mindist=MINDIST))
    total = time.perf_counter() - t0
    if rep:
        splits.append({'total_s': round(total, 3), 'calls': ncalls, **{k: round(v, 3) for k, v in kevlar_amd.call.last_timing.items()}})
print(json.dumps({'call_partitions': splits, 'clock': watch.stop()}), flush=True)
