"""Whole job on a FASTQ trio of config 2's size (7.5 M reads per sample, written once from kevlar_amd.synth): `kevlar novel --num-bands 4
--all-bands` in one process against the four `--band i` commands + `kevlar unband`; wall time of the processes, one warm-up round, five
alternated; the two outputs compared as sets of records first.  DESIGN.md section 7.  `python scratch/allbands_whole_job.py`
(WJ_GENOME / WJ_MEM: genome length and bytes per band sketch, for a smaller rehearsal.)"""
import json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from kevlar_amd import synth

GENOME, COV, L, K, NB, MEM = int(float(os.environ.get('WJ_GENOME', 25e6))), 30, 100, 31, 4, int(float(os.environ.get('WJ_MEM', 5e8)))
tmp = tempfile.mkdtemp(prefix='kvwhole_')
res = {'all_bands_s': [], 'per_band_plus_unband_s': [], 'per_band_parts_s': []}
try:
    t0 = time.time()
    packed = synth.trio_reads_packed(GENOME, COV, L, 42)
    names = ['proband', 'mother', 'father']
    rng = np.random.default_rng(12)
    for name in names:
        words = packed[name]; n = len(words)
        tag = '@{}_'.format(name).encode()
        rec = np.empty((n, len(tag) + 8 + 1 + L + 3 + L + 1), dtype=np.uint8)
        col = len(tag); rec[:, :col] = np.frombuffer(tag, dtype=np.uint8)
        digits = np.arange(n, dtype=np.int64)
        for d in range(8):
            rec[:, col + 7 - d] = 48 + digits % 10; digits //= 10
        col += 8; rec[:, col] = 10; col += 1
        for j in range(L):
            rec[:, col + j] = np.frombuffer(b'ACGT', dtype=np.uint8)[(words[:, j >> 4] >> np.uint32(2 * (j & 15))) & np.uint32(3)]
        col += L; rec[:, col:col + 3] = np.frombuffer(b'\n+\n', dtype=np.uint8); col += 3
        rec[:, col:col + L] = ord('F'); col += L; rec[:, col] = 10
        with open(os.path.join(tmp, name + '.fq'), 'wb') as fh:
            fh.write(rec.tobytes())
        del rec
    del packed
    os.sync()
    print('files written: {} reads per sample in {:.1f} s'.format(n, time.time() - t0), flush=True)
    base = [sys.executable, '-m', 'kevlar_amd', 'novel', '--ksize', str(K), '--memory', str(MEM), '--case', os.path.join(tmp, 'proband.fq'),
            '--control', os.path.join(tmp, 'mother.fq'), '--control', os.path.join(tmp, 'father.fq'), '--num-bands', str(NB)]
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(cmd):
        t = time.perf_counter()
        p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        dt = time.perf_counter() - t
        if p.returncode != 0:
            print(p.stdout.decode(errors='replace')[-3000:], flush=True)
            raise SystemExit('a step failed with {}: nothing more is started'.format(p.returncode))
        return dt, p.stdout.decode(errors='replace')

    def all_bands():
        return run(base + ['--all-bands', '-o', os.path.join(tmp, 'all.augfastq')])

    def per_band():
        parts, total = [], 0.0
        for b in range(1, NB + 1):
            dt, _ = run(base + ['--band', str(b), '-o', os.path.join(tmp, 'band{}.augfastq'.format(b))])
            parts.append(round(dt, 3)); total += dt
        dt, _ = run([sys.executable, '-m', 'kevlar_amd', 'unband', '-o', os.path.join(tmp, 'unbanded.augfastq')] +
                    [os.path.join(tmp, 'band{}.augfastq'.format(b)) for b in range(1, NB + 1)])
        parts.append(round(dt, 3))
        return total + dt, parts

    for rep in range(6):          # the first round warms the file cache and is not counted
        dt_a, log = all_bands()
        dt_b, parts = per_band()
        if rep == 0:
            print(log[-1500:], flush=True)
            import kevlar_amd
            def table(path):
                return {r.name: (r.sequence, tuple((k.offset, tuple(k.abund)) for k in r.annotations))
                        for r in kevlar_amd.parse_augmented_fastx(open(path)) if r is not None}
            a, b = table(os.path.join(tmp, 'all.augfastq')), table(os.path.join(tmp, 'unbanded.augfastq'))
            print('records: all-bands {}, unband {}, equal {}'.format(len(a), len(b), a == b), flush=True)
            assert a == b and len(a) > 0
        else:
            res['all_bands_s'].append(round(dt_a, 3)); res['per_band_plus_unband_s'].append(round(dt_b, 3)); res['per_band_parts_s'].append(parts)
        print(rep, round(dt_a, 3), round(dt_b, 3), parts, flush=True)
    for key in ('all_bands_s', 'per_band_plus_unband_s'):
        res[key + '_median'] = float(np.median(res[key])); res[key + '_min_max'] = [min(res[key]), max(res[key])]
    print(json.dumps(res), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
