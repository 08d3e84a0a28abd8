"""bench.py's plain line and --dump-outputs: a plain run times its steps and prints the line, every other leg waits for --full;
--dump-outputs writes the hits of the last timed step as float .npy files within a byte budget, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def hits(n, reads, S=3, seed=3):
    rng = np.random.default_rng(seed)
    r = np.sort(rng.integers(0, reads, n)).astype(np.uint32)
    o = rng.integers(0, 70, n).astype(np.uint32)
    a = rng.integers(0, 256, (n, S)).astype(np.uint8)
    return r, o, a


def load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path) if f.endswith('.npy')}


def test_dump_outputs_writes_every_hit_as_exact_floats(tmp_path):
    r, o, a = hits(5000, 1 << 20)
    bench.dump_outputs(str(tmp_path), r, o, a, 123456)
    got = load(str(tmp_path))
    assert sorted(got) == ['hit_abundance', 'hit_offset', 'hit_read', 'kmers_counted']
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got['hit_read'].dtype == np.float32 and got['hit_abundance'].shape == (5000, 3)
    assert np.array_equal(got['hit_read'].astype(np.uint32), r) and np.array_equal(got['hit_offset'].astype(np.uint32), o)
    assert np.array_equal(got['hit_abundance'].astype(np.uint8), a)
    assert got['kmers_counted'].tolist() == [123456.0]
    assert bench.hits_checksum(got['hit_read'].astype(np.uint32), got['hit_offset'].astype(np.uint32),
                               got['hit_abundance'].astype(np.uint8)) == bench.hits_checksum(r, o, a)


def test_dump_outputs_samples_beyond_the_budget_the_same_rows_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 200_000)
    r, o, a = hits(40000, 1 << 30)          # read indices beyond 2**24: float64
    picks = []
    for sub in ('one', 'two'):
        path = str(tmp_path / sub)
        bench.dump_outputs(path, r, o, a, 7)
        assert sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path)) <= 200_000
        got = load(path)
        assert got['hit_read'].dtype == np.float64 and got['hit_offset'].dtype == np.float32
        rows = got['hit_rows'].astype(np.int64)
        assert 0 < len(rows) < 40000 and np.all(np.diff(rows) > 0)
        assert np.array_equal(got['hit_read'].astype(np.uint64), r[rows]) and np.array_equal(got['hit_abundance'].astype(np.uint8), a[rows])
        picks.append(rows)
    assert np.array_equal(picks[0], picks[1])
    # a later dump that fits leaves no stale row list behind
    bench.dump_outputs(str(tmp_path / 'one'), r[:100], o[:100], a[:100], 7)
    assert 'hit_rows' not in load(str(tmp_path / 'one'))


def test_plain_and_full_options(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    args = bench.parse_args()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    args = bench.parse_args()
    assert args.full and args.dump_outputs == 'out' and args.steps == 20
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args()


def run_bench(*args, timeout=600):
    env = dict(os.environ)
    for key in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(key, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=timeout, universal_newlines=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith('{')]
    assert lines, 'no JSON line in: ' + res.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_steps_hits(tmp_path):
    dumps = []
    for sub in ('one', 'two'):
        out = run_bench('--gpus', '1', '--workload', 'cfg1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / sub))
        assert out['steps'] == 3 and out['warmup'] == 1 and out['ms_per_step'] > 0
        assert out['value'] == pytest.approx(3 * 5000 / (out['ms_per_step'] * 1e-3), rel=1e-2)
        assert out['cpu_baseline'] is None and out['end_to_end'] is None and 'banded_checksums' not in out['selfcheck']
        got = load(str(tmp_path / sub))
        assert 'hit_rows' not in got and len(got['hit_read']) == out['config']['interesting_kmer_instances']
        assert bench.hits_checksum(got['hit_read'].astype(np.uint32), got['hit_offset'].astype(np.uint32),
                                   got['hit_abundance'].astype(np.uint8)) == out['selfcheck']['hits_checksum']
        assert got['kmers_counted'].tolist() == [3 * 5000 * (100 - 31 + 1)]
        dumps.append(got)
    assert all(np.array_equal(dumps[0][name], dumps[1][name]) for name in dumps[0])


@pytest.mark.gpu
def test_full_run_keeps_every_leg():
    out = run_bench('--gpus', '1', '--workload', 'cfg1', '--steps', '1', '--warmup', '1', '--full')
    assert set(out['selfcheck']['banded_checksums']) == {'2', '4', '8'}
    assert out['cpu_baseline']['value'] > 0 and out['end_to_end']['value'] > 0
