"""Every template instance of the partitioned count, by name, at the edges of the planner that chooses among them
(tests/bin_instances_common.py is the table: the cases, and for each the exact instances kv_bin_last_instances and the plan numbers
kv_bin_last_plan must report).  A row sets its knobs, runs its entry point, asserts both reports, and holds the result to a reference
that is never the device: reads to the scalar oracle with the same explicit primes, hash lists to h % size in numpy's exact uint64 with
a saturating sum per bin -- the return value, every byte of every table, and n_occupied.  Everything is exact.

Before the device is looked at, a row asserts on the reference that its input does what the row is there for: every coarse bucket of
every table holds a non-zero bin, the few-bin last slice of an `above` sketch is hit by the list, the poly-A bin of a skew row is
saturated.  A failure there means the input is wrong, not the kernel.

A count that declined into the atomic kernels would leave the previous call's report standing: every row also asserts that k_consume,
k_add_hashes and k_add_hashes_weighted did not run.

Cost, measured in one job with the rest of the GPU suite on one MI355X: the module's 138 rows 16.8 s of the suite's 945 s (the suite
without it: 928 s, so 1.8 %).  The slowest three rows: wide-packed-k16 0.45 s, wide-packed-k64 0.43 s, wide-packed-k51 0.41 s.  The rows of
the three geometries with 2^30 bins (S16384-below, S16384-above and the `wide` rows: two 128 MB tables read back and compared with the
oracle's) take 0.2 to 0.45 s each, every other row under 0.2 s.  No read count was cut."""
import ctypes
import gc
import os

import numpy as np
import pytest

from bigtables_common import device_table, first_difference, oracle_table, storage_of
from bin_instances_common import (BINS_PER_BYTE, CASES, COUNTER_MAX, KNOBS, N_FIRST_BATCH, N_MASK_READS, SKM_BUCKET_KMERS, SMALL, STORAGE, any_bin_in_use,
                                  bucket_ranges, expected_table, hashes, reads, skewed_reads, split_report)
from test_gpu_bin_split_flush import WEIGHTS
from test_gpu_skm_instances import shape_reads

pytestmark = pytest.mark.gpu

ATOMIC_SCOPES = ('k_consume', 'k_add_hashes', 'k_add_hashes_weighted')


def report(entry):
    from kevlar_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    assert getattr(_lib.load(), entry)(buf, len(buf)) == 0
    return split_report(buf.value.decode())


def last_plan():
    """T, maxsl, cmax, F, C, ringB, threadsA, nwgA, nwgB, cap1, cap2, weighted, fast4"""
    from kevlar_amd import _lib
    out = (ctypes.c_uint64 * 13)()
    assert _lib.load().kv_bin_last_plan(out, 13) == 0
    return [int(v) for v in out]


def launches(name):
    from kevlar_amd import _lib
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.load().kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return n.value


@pytest.fixture
def knobs():
    """launch counts on; every knob a row sets is removed behind it"""
    from kevlar_amd import _lib
    lib = _lib.load()
    lib.kv_prof_reset()
    lib.kv_prof_enable(1)
    yield lib
    lib.kv_prof_enable(0)
    for name in KNOBS:
        os.environ.pop(name, None)


def assert_reports(row, weighted):
    assert {s: launches(s) for s in ATOMIC_SCOPES} == {s: 0 for s in ATOMIC_SCOPES}, (row['id'], 'the count declined into the atomic kernels')
    assert report('kv_bin_last_instances') == row['expect'], (row['id'], row['why'])
    if row['skm'] is not None:
        assert report('kv_skm_last_instances') == row['skm'], (row['id'], row['why'])
    plan = last_plan()
    assert plan[0] == len(row['primes']) and tuple(plan[1:7]) == row['plan'], (row['id'], row['why'], plan)
    nwgA, nwgB, cap1, cap2 = plan[7:11]
    assert nwgA >= 1 and 1 <= nwgB <= 512 and cap1 % 64 == 0 and cap2 % 64 == 0 and cap1 > 0 and cap2 > 0, plan
    assert plan[11] == (1 if weighted else 0) and plan[12] == 0, plan                   # (fast4 needs four tables)


def assert_buckets_hit(row, tables):
    """on the reference: every coarse bucket of every table holds a non-zero bin"""
    F = row['plan'][2]
    n_buckets = 0
    for t, (size, table) in enumerate(zip(row['primes'], tables)):
        for lo, hi in bucket_ranges(size, F):
            assert any_bin_in_use(table, row['cls'], lo, hi), '{}: the reference has nothing in bins [{}, {}) of table {}'.format(row['id'], lo, hi, t)
            n_buckets += 1
    assert n_buckets >= row['plan'][3]              # the larger table has all C of them


# ---- reads ------------------------------------------------------------------------------------------------------------------------
def inputs(row):
    """(strings, packed words or None, read length)"""
    if row['variant'] == 'skew':
        words, strings = skewed_reads()
        return strings, words, 100
    if row['entry'] == 'packed':
        words, strings = reads(row['n'], row['shape'])
        return strings, words, row['shape']
    strings, _ = shape_reads(row['shape'], row['n'])
    return strings, None, 0


def n_leading(row, n):
    """the reads a mask or a first batch is made of: N_MASK_READS = N_FIRST_BATCH = 2000 of 8000, and a third of a shorter batch"""
    assert N_MASK_READS == N_FIRST_BATCH
    return N_MASK_READS if row['n'] >= 4 * N_MASK_READS else row['n'] // 3


MASKED = {'mask': (0, False), 'mask-kept': (1, True)}      # (threshold, consume_masked): k-mers the mask lacks | k-mers the mask holds

_reference = {}             # one entry: the rows of one input and geometry stand next to each other in the table


def reference(ok, row):
    """the oracle's sketch after the row's reads, its return value, its mask; made once for the rows that share it"""
    key = (row['cls'], tuple(row['primes']), row['k'], row['entry'], row['shape'], row['n'], row['variant'])
    if key not in _reference:
        _reference.clear()
        gc.collect()
        strings, _, _ = inputs(row)
        k, variant = row['k'], row['variant']
        bases, offs = ok.concat_reads(list(strings))
        ref = getattr(ok, row['cls'])(k, 0, 0, primes=row['primes'])
        total = sum(max(0, len(r) - k + 1) for r in strings)
        mask = None
        if variant == 'band':
            n_ref = ok.consume_reads(ref, bases, offs, len(strings), 4, 3)
            assert total // 6 < n_ref < total // 3
        elif variant in MASKED:
            mask = ok.Nodetable(k, 0, 0, primes=SMALL['primes'])
            assert ok.consume_reads(mask, bases, offs, n_leading(row, len(strings))) > 0
            n_ref = ok.consume_reads(ref, bases, offs, len(strings), mask=mask, threshold=MASKED[variant][0], consume_masked=MASKED[variant][1])
            assert total // 8 < n_ref < total - total // 8
        else:
            if variant == 'second':
                assert ok.consume_reads(ref, bases, offs, n_leading(row, len(strings))) > 0
            n_ref = ok.consume_reads_mt(ref, bases, offs, len(strings), 4) if len(strings) >= 4000 else ok.consume_reads(ref, bases, offs, len(strings))
            assert n_ref == total               # (of a second batch: what the second call returns)
        _reference[key] = (ref, n_ref, mask)
    return _reference[key]


def same_tables(ok, dev, ref, what):
    assert dev.hashsizes() == ref.hashsizes()
    storage = storage_of(ref)
    for t, size in enumerate(ref.hashsizes()):
        diff = first_difference(device_table(dev, t), oracle_table(ok, ref, t), storage)
        assert diff is None, '{}: table {} ({} bins, {}): bin {} holds {}, the oracle {}'.format(what, t, size, storage, *diff)
    assert dev.n_occupied() == ref.n_occupied(), what


def run_reads(hk, ok, lib, row):
    strings, words, read_len = inputs(row)
    k, variant = row['k'], row['variant']
    ref, n_ref, ref_mask = reference(ok, row)
    assert_buckets_hit(row, [oracle_table(ok, ref, t) for t in range(len(row['primes']))])
    top = COUNTER_MAX[STORAGE[row['cls']]]
    if variant == 'skew':
        assert ref.get('A' * k) == top

    def batch_of(n):
        return hk.ReadBatch.from_packed(np.ascontiguousarray(words[:n]), read_len) if words is not None else hk.ReadBatch(list(strings[:n]))
    dev = getattr(hk, row['cls'])(k, 0, 0, primes=row['primes'])
    args = {}
    if variant == 'band':
        args = dict(nbands=4, band=3)
    elif variant in MASKED:
        dev_mask = hk.Nodetable(k, 0, 0, primes=SMALL['primes'])
        assert dev_mask.consume_batch(batch_of(n_leading(row, len(strings)))) > 0
        same_tables(ok, dev_mask, ref_mask, row['id'] + ': the mask')
        args = dict(mask=dev_mask, threshold=MASKED[variant][0], consume_masked=MASKED[variant][1])
    os.environ['KV_COUNT_PATH'] = row['path']
    os.environ['KV_SKM_BUCKET_KMERS'] = SKM_BUCKET_KMERS
    if variant == 'second':
        assert dev.consume_batch(batch_of(n_leading(row, len(strings)))) > 0
    lib.kv_prof_reset()
    n_dev = dev.consume_batch(batch_of(len(strings)), **args)
    assert_reports(row, row['path'] == 'skm')
    assert n_dev == n_ref, row['id']
    same_tables(ok, dev, ref, row['id'])
    if variant == 'skew':
        assert dev.get('A' * k) == top


# ---- hash lists -------------------------------------------------------------------------------------------------------------------
def run_list(hk, ok, lib, row):
    import torch
    primes, cls = row['primes'], row['cls']
    h = hashes(tuple(primes), row['n'])
    w = WEIGHTS[np.arange(len(h)) % len(WEIGHTS)] if row['weighted'] else None
    want = [expected_table(h, size, cls, w) for size in primes]
    assert_buckets_hit(row, [table for table, _ in want])
    maxsl = row['plan'][0]
    last_slice = (maxsl - 1) << 16
    assert any_bin_in_use(want[0][0], cls, last_slice, primes[0])
    if primes[0] - last_slice < 100:                # an `above` sketch: that slice is a handful of bins, and table 1 ends a slice earlier
        assert primes[1] <= last_slice
        per = BINS_PER_BYTE[STORAGE[cls]]
        assert want[0][0][(primes[0] - 1) // per] != 0
    os.environ['KV_COUNT_PATH'] = 'binned'
    dev = getattr(hk, cls)(31, 0, 0, primes=primes)
    lib.kv_prof_reset()
    if w is None:
        d_h = torch.from_numpy(h.view(np.int64)).cuda()
        assert dev.consume_hashes(d_h.data_ptr(), len(h)) == len(h)
    else:
        d_pairs = torch.from_numpy(np.stack([h.view(np.int64), w], axis=1)).cuda()
        assert dev.consume_hashes_weighted(d_pairs.data_ptr(), len(h)) == int(w.sum())
    assert_reports(row, row['weighted'])
    storage = storage_of(dev)
    for t, size in enumerate(primes):
        diff = first_difference(device_table(dev, t), want[t][0], storage)
        assert diff is None, '{}: table {} ({} bins, {}): bin {} holds {}, expected {}'.format(row['id'], t, size, storage, *diff)
    assert dev.n_occupied() == want[0][1], row['id']


@pytest.mark.parametrize('row', CASES, ids=[c['id'] for c in CASES])
def test_bin_instance_row(hk, ok, knobs, row):
    (run_list if row['entry'] == 'list' else run_reads)(hk, ok, knobs, row)


def test_the_reports_say_when_they_do_not_fit(hk, knobs):
    """KV_ERR_CAPACITY (-6) for a list that does not fit with its terminating zero and for fewer than 13 numbers; the report itself is unchanged"""
    import torch
    from kevlar_amd import _lib
    lib = knobs
    os.environ['KV_COUNT_PATH'] = 'binned'
    dev = hk.Counttable(31, 0, 0, primes=SMALL['primes'])
    h = hashes(tuple(SMALL['primes']), 4096)
    d_h = torch.from_numpy(h.view(np.int64)).cuda()
    assert dev.consume_hashes(d_h.data_ptr(), len(h)) == len(h)
    want = ['k_bin_list<512,false>', 'k_bin_split<false>', 'k_bin_apply<ST_BYTE,false>', 'k_bin_spill']
    assert report('kv_bin_last_instances') == want
    text = ','.join(want)
    exact, short = ctypes.create_string_buffer(len(text) + 1), ctypes.create_string_buffer(len(text))
    assert lib.kv_bin_last_instances(exact, len(exact)) == 0 and exact.value.decode() == text
    assert lib.kv_bin_last_instances(short, len(short)) == -6 and 'kv_bin_last_instances' in _lib.last_error()
    out = (ctypes.c_uint64 * 13)()
    assert lib.kv_bin_last_plan(out, 12) == -6 and not any(out)
    assert lib.kv_bin_last_plan(out, 13) == 0 and tuple(out[1:7]) == SMALL['plan']
