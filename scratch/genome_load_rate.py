"""What loading the reference costs `kevlar localize`, the host path against the device path (kevlar_amd/csrc/kv_genome.hip): a
synthetic genome of 256 Mb in 8 sequences, wrapped at 60, seeded, written as plain text, as one gzip stream and as BGZF; against it
1 M seeds of length 51 (10 % of them cut from the genome, every other one reverse-complemented).  Per container, each way in a
process of its own under its own time limit (so that the peak memory is that way's alone), one warm-up and five timed rounds by
the host clock:
  old   Genome.from_file + SeedSet.scan over the joined text                  (the parent commit's way)
  new   DeviceGenome (kv_genome_open) + SeedSet.scan_genome, and a second scan_genome with another seed set on the resident genome
with the library's kv_prof kernel times, the card's clock and power, and the peak resident memory (resource.getrusage) beside
them.  The matches of both ways are compared before anything is timed.  The script stops at the first step that fails.
DESIGN.md section 9.  `python scratch/genome_load_rate.py [megabases] [seeds] [workdir]`"""
import ctypes, gzip, json, os, resource, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

Z, NSEQ, WIDTH = 51, 8, 60
CONTAINERS = ('plain', 'gzip', 'bgzf')
STEP_LIMIT = {'make': 600, 'old': 900, 'new': 600}          # seconds


def paths(work):
    return {'plain': os.path.join(work, 'genome.fa'), 'gzip': os.path.join(work, 'genome.fa.gz'), 'bgzf': os.path.join(work, 'genome.bgzf.fa.gz'),
            'seeds': os.path.join(work, 'seeds.npy')}


def make(work, megabases, n_seeds):
    """the three files and two seed sets (rows of Z bytes), all from one seed"""
    from kevlar_amd import bgzf
    rng = np.random.default_rng(9)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8); comp[list(b'ACGT')] = list(b'TGCA')
    per = megabases * 1000000 // NSEQ // WIDTH * WIDTH
    pieces, seqs = [], []
    for s in range(NSEQ):
        seq = letters[rng.integers(0, 4, size=per, dtype=np.uint8)]
        seqs.append(seq)
        lines = np.empty((per // WIDTH, WIDTH + 1), dtype=np.uint8)
        lines[:, :WIDTH] = seq.reshape(-1, WIDTH); lines[:, WIDTH] = 10
        pieces += ['>chr{} synthetic sequence {} of {}\n'.format(s + 1, s + 1, NSEQ).encode(), lines.tobytes()]
    data = b''.join(pieces)
    p = paths(work)
    open(p['plain'], 'wb').write(data)
    with gzip.open(p['gzip'], 'wb', compresslevel=1) as fh:
        fh.write(data)
    bgzf.write_file(p['bgzf'], data, level=1, threads=16)
    sets = []
    for _ in range(2):
        planted = n_seeds // 10
        rows = letters[rng.integers(0, 4, size=(n_seeds, Z), dtype=np.uint8)]
        which, at = rng.integers(0, NSEQ, size=planted), rng.integers(0, per - Z, size=planted)
        for i in range(planted):
            rows[i] = seqs[which[i]][at[i]:at[i] + Z]
        rows[1:planted:2] = comp[rows[1:planted:2, ::-1]]
        sets.append(rows)
    np.save(p['seeds'], np.stack(sets))
    print(json.dumps({'step': 'make', 'bases': per * NSEQ, 'bytes': {c: os.path.getsize(p[c]) for c in CONTAINERS}}), flush=True)


def prof_all(lib):
    buf = ctypes.create_string_buffer(1 << 14)
    lib.kv_prof_names(buf, len(buf))
    out = {}
    for name in filter(None, buf.value.decode().split(',')):
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        lib.kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
        if cnt.value:
            out[name] = [round(ms.value, 3), int(cnt.value)]
    return out


def measure(work, way, container):
    import torch
    torch.cuda.init()
    from kevlar_amd import _lib
    from kevlar_amd.localize import DeviceGenome, Genome, SeedSet
    from bench import ClockWatch
    lib = _lib.load(); _lib.require_device()
    p = paths(work)
    sets = np.load(p['seeds'])
    seeds = [[row.tobytes().decode() for row in rows] for rows in sets]
    path = p[container]

    def canonical(seedset, ids, pos):
        order = np.lexsort((pos, seedset.seed_of_window[ids]))
        return pos[order]
    with SeedSet(seeds[0], Z) as first, SeedSet(seeds[1], Z) as second:
        # the answer of this way, for the driver to compare with the other way's
        if way == 'old':
            genome = Genome.from_file(path)
            ids, pos = first.scan(genome.text)
        else:
            genome = DeviceGenome(path)
            ids, pos = first.scan_genome(genome)
        answer = {'matches': int(len(ids)), 'positions_sum': int(pos.astype(np.uint64).sum()), 'ids': genome.ids, 'starts': genome.starts.tolist()}
        if way == 'new':
            genome.close()
        del genome
        lib.kv_prof_enable(1)
        rounds, watch = [], None
        for rep in range(6):                 # the first is a warm-up
            if rep == 1:
                watch = ClockWatch(0)
            lib.kv_prof_reset()
            t0 = time.perf_counter()
            if way == 'old':
                genome = Genome.from_file(path)
                t1 = time.perf_counter()
                first.scan(genome.text)
                t2 = t3 = time.perf_counter()
            else:
                genome = DeviceGenome(path)
                t1 = time.perf_counter()
                first.scan_genome(genome)
                t2 = time.perf_counter()
                second.scan_genome(genome)
                t3 = time.perf_counter()
                genome.close()
            del genome
            if rep:
                rounds.append({'load_s': round(t1 - t0, 4), 'scan_s': round(t2 - t1, 4), 'load_and_scan_s': round(t2 - t0, 4),
                               'second_scan_s': round(t3 - t2, 4), 'kernels_ms': prof_all(lib)})
        clock = watch.stop()
    med = lambda key: float(np.median([r[key] for r in rounds]))          # noqa: E731
    print(json.dumps({'step': way, 'container': container, 'answer': answer, 'load_s': med('load_s'), 'scan_s': med('scan_s'),
                      'load_and_scan_s': med('load_and_scan_s'), 'second_scan_s': med('second_scan_s'),
                      'load_and_scan_all': [r['load_and_scan_s'] for r in rounds], 'kernels_ms_last': rounds[-1]['kernels_ms'],
                      'peak_rss_mb': resource.getrusage(resource.RUSAGE_SELF).ru_maxrss // 1024, 'clock': clock}), flush=True)


def step(args, limit):
    """one step in a process of its own, under its own time limit; its last line of output is its JSON result"""
    done = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(done.stdout)
    sys.stdout.flush()
    if done.returncode != 0:
        sys.exit('step {} failed with status {}'.format(' '.join(args), done.returncode))
    return json.loads(done.stdout.strip().split('\n')[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--make':
        return make(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    if len(sys.argv) > 1 and sys.argv[1] == '--measure':
        return measure(sys.argv[2], sys.argv[3], sys.argv[4])
    megabases = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n_seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    work = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'bench_out', 'genome_load_rate')
    os.makedirs(work, exist_ok=True)
    step(['--make', work, str(megabases), str(n_seeds)], STEP_LIMIT['make'])
    verdict = {}
    for container in CONTAINERS:
        old = step(['--measure', work, 'old', container], STEP_LIMIT['old'])
        new = step(['--measure', work, 'new', container], STEP_LIMIT['new'])
        if old['answer'] != new['answer']:
            sys.exit('the two ways disagree on {}'.format(container))
        verdict[container] = {'old_load_and_scan_s': old['load_and_scan_s'], 'new_load_and_scan_s': new['load_and_scan_s'],
                              'new_second_scan_s': new['second_scan_s'], 'old_peak_rss_mb': old['peak_rss_mb'], 'new_peak_rss_mb': new['peak_rss_mb'],
                              'new_is_not_slower': new['load_and_scan_s'] <= old['load_and_scan_s']}
    print(json.dumps({'step': 'verdict', 'megabases': megabases, 'seeds': n_seeds, 'seedsize': Z, 'by_container': verdict}), flush=True)
    for name in paths(work).values():
        if os.path.exists(name):
            os.remove(name)


if __name__ == '__main__':
    main()
