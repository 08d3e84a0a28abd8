"""`kevlar novel --num-bands N --all-bands`: kv_hits_merge against numpy.lexsort, the one-command run against the product's own
per-band runs + `unband`, against the oracle's all-band count and scan, and shared between ranks."""
import contextlib
import gzip
import io
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, data_file

pytestmark = pytest.mark.gpu

FOUND = re.compile(r'Found (\d+) instances of (\d+) unique novel kmers in (\d+) reads')


def run_cli(arglist):
    import kevlar_amd
    args = kevlar_amd.cli.parser().parse_args(arglist)
    out, err = io.StringIO(), io.StringIO()
    old = kevlar_amd.logstream
    kevlar_amd.logstream = err
    try:
        with contextlib.redirect_stdout(out):
            kevlar_amd.cli.mains[args.cmd](args)
    finally:
        kevlar_amd.logstream = old
    return out.getvalue(), err.getvalue()


# ---- 2. kv_hits_merge against numpy.lexsort ------------------------------------------------------------------------------
def dealt_runs(seed, R, S, n, wide=False, empty=()):
    """n unique (read, offset) pairs dealt at random to the R runs (none to the runs in `empty`), sorted inside each run;
    returns (read, offset, abund, run starts) with the runs back to back"""
    rng = np.random.default_rng(seed)
    if wide:        # offsets of 65 536 and more, reads up to 2^32 - 1: what a 16-bit offset under the read index cannot hold
        keys = np.unique(np.concatenate((rng.integers(0, 1 << 64, size=n + 64, dtype=np.uint64),
                                         np.array([(0xffffffff << 32) | 0xffffffff, (0xffffffff << 32) | 65536, 65536, 0], dtype=np.uint64))))
    else:           # a scan's shape: reads with a few dozen hits each, offsets inside a read
        keys = np.unique((rng.integers(0, max(1, n // 20), size=n + n // 8 + 8, dtype=np.uint64) << np.uint64(32))
                         | rng.integers(0, 120, size=n + n // 8 + 8, dtype=np.uint64))
    keys = keys[rng.permutation(len(keys))[:n]] if n else keys[:0]
    assert len(keys) == n
    fed = [r for r in range(R) if r not in empty]
    owner = np.asarray(fed, dtype=np.int64)[rng.integers(0, len(fed), size=n)]
    abund = rng.integers(0, 256, size=(n, S), dtype=np.uint8)
    order = np.lexsort((keys, owner))
    keys, owner, abund = keys[order], owner[order], abund[order]
    starts = np.searchsorted(owner, np.arange(R + 1)).astype(np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xffffffff)).astype(np.uint32), abund, starts


def merge_on_device(hk, read, offset, abund, starts):
    import torch
    d_read = torch.from_numpy(read.view(np.int32)).cuda()
    d_offset = torch.from_numpy(offset.view(np.int32)).cuda()
    d_abund = torch.from_numpy(np.ascontiguousarray(abund)).cuda()
    torch.cuda.synchronize()
    return hk.hits_merge(d_read.data_ptr(), d_offset.data_ptr(), d_abund.data_ptr(), starts, abund.shape[1])


@pytest.mark.parametrize('R,S,n,wide,empty', [
    (1, 1, 50000, False, ()), (1, 3, 50000, False, ()), (1, 16, 50000, False, ()),
    (2, 1, 50000, False, ()), (2, 3, 50000, False, ()), (2, 16, 2000000, False, ()),
    (3, 1, 50000, False, (1,)), (3, 3, 50000, False, (0,)), (3, 16, 50000, False, (2,)),
    (8, 1, 50000, False, (0, 7)), (8, 3, 2000000, False, ()), (8, 16, 50000, False, (3,)),
    (8, 3, 0, False, ()), (1, 3, 0, False, ()), (8, 3, 1, False, ()), (1, 1, 1, False, ()), (3, 16, 1, False, (0, 1)),
    (3, 3, 100000, True, ()), (8, 1, 2000000, True, (2,)),
])
def test_hits_merge_equals_lexsort(hk, R, S, n, wide, empty):
    """read for read, offset for offset, abundance row for abundance row: the merged handle is numpy.lexsort of the rows"""
    read, offset, abund, starts = dealt_runs(1000 + 17 * R + S + n % 97, R, S, n, wide, empty)
    assert len(starts) == R + 1 and int(starts[-1]) == n and all(int(starts[r]) == int(starts[r + 1]) for r in empty)
    if wide:
        assert int(offset.max()) >= 65536 and int(read.max()) == 0xffffffff
    got_read, got_offset, got_abund, discarded = merge_on_device(hk, read, offset, abund, starts)
    order = np.lexsort((offset, read))
    assert got_read.dtype == np.uint32 and got_offset.dtype == np.uint32 and got_abund.shape == (n, S) and len(discarded) == 0
    assert np.array_equal(got_read, read[order])
    assert np.array_equal(got_offset, offset[order])
    assert np.array_equal(got_abund, abund[order])


def test_hits_merge_refuses_a_key_in_two_runs_and_an_unsorted_run(hk):
    from kevlar_amd._lib import KvArgError
    read, offset, abund, starts = dealt_runs(5, 3, 3, 30000)
    lo, hi = int(starts[1]), int(starts[2])
    assert hi - lo > 10 and int(starts[1]) > 10
    twice = (read.copy(), offset.copy())
    twice[0][lo + 5], twice[1][lo + 5] = read[3], offset[3]            # a pair of run 0 once more in run 1 ...
    order = np.lexsort((twice[1][lo:hi], twice[0][lo:hi])) + lo       # ... which stays sorted
    twice[0][lo:hi], twice[1][lo:hi] = twice[0][order], twice[1][order]
    with pytest.raises(KvArgError, match='two runs'):
        merge_on_device(hk, twice[0], twice[1], abund, starts)
    swapped = (read.copy(), offset.copy())
    for column in swapped:
        column[[lo + 2, lo + 3]] = column[[lo + 3, lo + 2]]
    with pytest.raises(KvArgError, match='not sorted'):
        merge_on_device(hk, swapped[0], swapped[1], abund, starts)
    with pytest.raises(KvArgError):                                   # run starts that do not begin at 0 / that go backwards
        merge_on_device(hk, read, offset, abund, np.array([1, 5, 9, len(read)], dtype=np.uint64))
    with pytest.raises(KvArgError):
        merge_on_device(hk, read, offset, abund, np.array([0, 9, 5, len(read)], dtype=np.uint64))
    got = merge_on_device(hk, read, offset, abund, starts)          # and the rows as they were still merge
    assert np.array_equal(got[0], read[np.lexsort((offset, read))])


# ---- 3. the fixture trios against the product's own per-band path ------------------------------------------------------
def records_of(text):
    import kevlar_amd
    return [rec for rec in kevlar_amd.parse_augmented_fastx(io.StringIO(text)) if rec is not None]


def as_table(records):
    table = {rec.name: (rec.sequence, rec.quality, [(k.offset, tuple(k.abund)) for k in rec.annotations]) for rec in records}
    assert len(table) == len(records), 'a read name twice'
    return table


def trio_args(trio):
    return ['novel', '--case', data_file('microtrios/trio-{}-proband.fq.gz'.format(trio)), '--ksize', '25', '--case-min', '7',
            '--ctrl-max', '0', '--memory', '500K', '--control', data_file('microtrios/trio-{}-father.fq.gz'.format(trio)),
            '--control', data_file('microtrios/trio-{}-mother.fq.gz'.format(trio))]


def per_band_then_unband(base, nbands, tmp):
    """the N `--band i` commands and `unband` through the command line: (unbanded records, records per band, summed X, summed Y)"""
    paths, bands, x, y = [], [], 0, 0
    for band in range(1, nbands + 1):
        paths.append(os.path.join(str(tmp), 'band{}.augfastq'.format(band)))
        _, log = run_cli(base + ['--num-bands', str(nbands), '--band', str(band), '-o', paths[-1]])
        found = FOUND.search(log)
        x, y = x + int(found.group(1)), y + int(found.group(2))
        bands.append(records_of(open(paths[-1]).read()))
        assert int(found.group(3)) == len(bands[-1])
    merged = os.path.join(str(tmp), 'unbanded.augfastq')
    run_cli(['unband', '-o', merged] + paths)
    return records_of(open(merged).read()), bands, x, y


def all_bands(base, nbands, path, extra=()):
    _, log = run_cli(base + ['--num-bands', str(nbands), '--all-bands', '-o', path] + list(extra))
    return open(path).read(), log


def fastq_names(path):
    with gzip.open(path, 'rt') as text:
        return [line[1:].rstrip('\n') for i, line in enumerate(text) if i % 4 == 0]


@pytest.mark.parametrize('trio,nbands,annotations,reads,by_band,from_two', [
    ('li', 4, 186, 11, [51, 48, 48, 39], 11),
    ('na', 4, 251, 13, [98, 51, 74, 28], 13),
    ('li', 3, 186, 11, [90, 50, 46], 1),
])
def test_all_bands_equals_unband_of_the_per_band_runs(hk, tmp_path, trio, nbands, annotations, reads, by_band, from_two):
    """The same records by name -- name, sequence, quality, [(offset, abundances)] -- as the N `--band i` commands and `unband`
    give, in the order of the proband file; X, Y, Z of the closing line from the per-band lines.  The counts are what the
    reference arithmetic gives for these inputs at 500 K per band sketch (the oracle's all-band count and scan)."""
    base = trio_args(trio)
    want, bands, x, y = per_band_then_unband(base, nbands, tmp_path)
    text, log = all_bands(base, nbands, str(tmp_path / 'all.augfastq'))
    got = records_of(text)
    assert [sum(len(rec.annotations) for rec in band) for band in bands] == by_band
    assert sum(len(rec.annotations) for rec in want) == annotations and len(want) == reads
    seen_in = {}
    for band in bands:
        for rec in band:
            seen_in[rec.name] = seen_in.get(rec.name, 0) + 1
    assert sum(1 for n in seen_in.values() if n >= 2) >= from_two, 'no record carries annotations of two bands: the merge is not exercised'
    assert as_table(got) == as_table(want)
    names = fastq_names(data_file('microtrios/trio-{}-proband.fq.gz'.format(trio)))
    assert len(set(names)) == len(names) == 6000
    position = {name: i for i, name in enumerate(names)}
    assert [position[rec.name] for rec in got] == sorted(position[rec.name] for rec in got), 'not in the order of the proband file'
    for rec in got:
        assert [k.offset for k in rec.annotations] == sorted(k.offset for k in rec.annotations)
    found = FOUND.search(log)
    assert (int(found.group(1)), int(found.group(2)), int(found.group(3))) == (x, y, len(got)) and x == annotations
    for band in range(1, nbands + 1):
        assert '[kevlar::novel] band {}/{}'.format(band, nbands) in log
        assert 'Done loading k-mers (band {}/{})'.format(band, nbands) in log


# ---- 4. against the oracle, several batches ----------------------------------------------------------------------------
SYNTH = dict(genome=300000, coverage=30, seed=11, k=31, memory=4e6, nbands=5, casemin=6, ctrlmax=1, read_len=100)


def synth_trio_files(directory):
    from kevlar_amd import synth
    packed = synth.trio_reads_packed(SYNTH['genome'], SYNTH['coverage'], SYNTH['read_len'], SYNTH['seed'])
    reads, paths = {}, {}
    for name in ('proband', 'mother', 'father'):
        reads[name] = synth.unpack_reads(packed[name], SYNTH['read_len'])
        paths[name] = os.path.join(str(directory), name + '.fq')
        with open(paths[name], 'w') as out:
            for i, seq in enumerate(reads[name]):
                out.write('@{}{}\n{}\n+\n{}\n'.format(name[0], i, seq, 'I' * len(seq)))
    return reads, paths


def oracle_all_bands(ok, reads):
    """every (read, offset, abundances, band) of the proband the reference arithmetic finds, band by band, in (read, offset) order"""
    k, nbands = SYNTH['k'], SYNTH['nbands']
    by_band = {}
    for name, seqs in reads.items():
        bases, offs = ok.concat_reads(seqs)
        by_band[name] = [ok.Counttable(k, SYNTH['memory'] / 4, 4) for _ in range(nbands)]
        ok.consume_reads_mt_allbands(by_band[name], bases, offs, len(seqs), 4)
    bases, offs = ok.concat_reads(reads['proband'])
    return ok.novel_scan_mt_allbands([[by_band['proband'][b]] for b in range(nbands)],
                                     [[by_band['mother'][b], by_band['father'][b]] for b in range(nbands)],
                                     bases, offs, len(reads['proband']), k, SYNTH['casemin'], SYNTH['ctrlmax'], 4)


def test_all_bands_equals_the_oracle_over_several_batches(hk, ok, tmp_path):
    """A synthetic trio in files, five bands, five scan batches: the output's records are exactly the oracle's (read, offset,
    abundances) of all bands, in input order."""
    from kevlar_amd import allbands
    reads, paths = synth_trio_files(tmp_path)
    n = len(reads['proband'])
    batch = n // 5
    want_read, want_offset, want_abund, want_band = oracle_all_bands(ok, reads)
    # the input is not an easy one: asserted on the oracle's side
    assert len(np.unique(want_read)) >= 1000
    assert sorted(set((want_read // batch).tolist())) == list(range(-(-n // batch))), 'a batch without annotated reads'
    assert sorted(set(want_band.tolist())) == list(range(SYNTH['nbands'])), 'a band that judged no hit'
    tally = {}
    text = b''.join(allbands.novel_all_bands([[paths['proband']]], [[paths['mother']], [paths['father']]], SYNTH['k'], SYNTH['memory'], 0.2,
                                             SYNTH['nbands'], SYNTH['casemin'], SYNTH['ctrlmax'], batchsize=batch, tally=tally))
    got = records_of(text.decode('latin-1'))
    rows = [(int(rec.name[1:]), k.offset, tuple(k.abund)) for rec in got for k in rec.annotations]
    want = list(zip(want_read.tolist(), want_offset.tolist(), (tuple(row) for row in want_abund.tolist())))
    assert rows == want
    for rec in got:
        assert rec.sequence == reads['proband'][int(rec.name[1:])] and rec.quality == 'I' * len(rec.sequence)
    assert tally['instances'] == len(want) and tally['reads'] == len(got) == len(np.unique(want_read))


# ---- 5. --abund-screen and --skip-until ----------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['abund-screen', 'skip-until'])
def test_all_bands_with_screen_and_with_skip(hk, tmp_path, which):
    if which == 'abund-screen':
        base = ['novel', '--ksize', '25', '--ctrl-max', '1', '--case-min', '8', '--case', data_file('screen-case.fa'),
                '--control', data_file('screen-ctrl.fa'), '--abund-screen', '3']
    else:
        base = ['novel', '--ctrl-max', '0', '--case-min', '6', '--case', data_file('trio1/case1.fq.gz'), '--control', data_file('trio1/ctrl1.fq.gz'),
                '--control', data_file('trio1/ctrl2.fq.gz'), '--skip-until', 'bogus-genome-chr1_115_449_0:0:0_0:0:0_1f4/1']
    want, bands, x, y = per_band_then_unband(base, 2, tmp_path)
    text, log = all_bands(base, 2, str(tmp_path / 'all.aug'))
    got = records_of(text)
    assert len(want) > 0 and as_table(got) == as_table(want)
    found = FOUND.search(log)
    assert (int(found.group(1)), int(found.group(2)), int(found.group(3))) == (x, y, len(got))


# ---- 6. / 7. ranks ---------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def start_ranks(world, backend, outs, extra_env=None):
    """fresh `python -m kevlar_amd novel ... --all-bands --distributed` children with the rank environment; (processes, outputs)"""
    assert world <= 3
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0', **(extra_env or {}))
        cmd = [sys.executable, '-m', 'kevlar_amd'] + trio_args('li') + ['--num-bands', '4', '--all-bands', '--distributed',
                                                                         '--dist-backend', backend, '-o', outs[rank]]
        procs.append(subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    said, killed = [], []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
            killed.append(False)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            killed.append(True)
        said.append(out.decode(errors='replace'))
    return procs, said, killed


@pytest.mark.parametrize('world,backend', [(2, 'gloo'), (3, 'gloo'), (1, 'nccl')])
def test_all_bands_shared_between_ranks(hk, tmp_path, world, backend):
    """bands 2+2 and 2+1+1 over gloo on this one GPU, and the RCCL transport with the one rank the box allows: rank 0's file is
    byte for byte the single-process file, the other ranks write nothing"""
    single, log = all_bands(trio_args('li'), 4, str(tmp_path / 'single.augfastq'))
    assert len(records_of(single)) == 11
    outs = [str(tmp_path / 'rank{}.augfastq'.format(rank)) for rank in range(world)]
    procs, said, killed = start_ranks(world, backend, outs)
    for rank, p in enumerate(procs):
        assert not killed[rank], 'rank {} hung:\n{}'.format(rank, said[rank][-3000:])
        assert p.returncode == 0, 'rank {} failed:\n{}'.format(rank, said[rank][-3000:])
    assert open(outs[0]).read() == single
    assert FOUND.search(said[0]).group(0) == FOUND.search(log).group(0)
    for rank in range(1, world):
        assert not os.path.exists(outs[rank]) and FOUND.search(said[rank]) is None


def test_all_bands_ranks_agree_on_a_failure(hk, tmp_path):
    """rank 1 fails before its second band (0-based band 3): both ranks stop with an error before the timeout, both name rank 1
    and its reason, nobody is left in a collective, no output remains"""
    outs = [str(tmp_path / 'rank{}.augfastq'.format(rank)) for rank in range(2)]
    procs, said, killed = start_ranks(2, 'gloo', outs, {'KV_ALLBANDS_TEST_FAIL': '1:3'})
    for rank, p in enumerate(procs):
        assert not killed[rank], 'rank {} hung:\n{}'.format(rank, said[rank][-3000:])
        assert p.returncode not in (0, None, -9), said[rank][-3000:]
        assert 'rank 1 failed' in said[rank] and 'forced by KV_ALLBANDS_TEST_FAIL' in said[rank], said[rank][-3000:]
        assert not os.path.exists(outs[rank])
