"""The first-toucher kernels of kevlar_amd/csrc/kv_graph.hip (k_first_touch, k_mark_first, k_mark_first_untracked, k_popcount,
k_abund_hist) behind kv_unique_new, kv_unique_exact and kv_abundance_distribution, held to the oracle's single thread at their edges:
every kind (byte, nibble and bit storage, both hash families) over tables of a few dozen bins, sixteen tables, sizes on both sides of
2^16 and one table; k of 21, 32, 33 and 51; on top of reads counted before; with bands, masks with a threshold and consume_masked,
reads with an N and lowercase bases, uniform batches from packed words, tracking that starts right after clear(); an empty batch, a
batch without k-mers, a batch of one k-mer, a batch whose k-mer total is a multiple of 32 with its first and last k-mer new; the
abundance distribution over 1, 2 and 4 batches per call with counter sketches as tracking tables and a saturated entry; the public
kv_unique_exact nobody calls.  All comparisons are exact.  tests/test_first_touch_reference.py holds, with the oracle alone, that
these inputs tell a wrong first-toucher rule from the right one."""
import ctypes

import numpy as np
import pytest

import first_touch_common as ft
import tables_common as tc

pytestmark = pytest.mark.gpu

_u64p = ctypes.POINTER(ctypes.c_uint64)
_masks = {}


def device_mask(hk, ok, case):
    """the case's mask on the device, counted once per process and held to the oracle's"""
    if not case.mask:
        return None
    key = (case.mask[0], case.k)
    if key not in _masks:
        mask = ft.make(hk, case.mask[0], case.k, ft.MASK_GEOMETRY[case.mask[0]])
        mask.consume_batch(hk.ReadBatch(ft.MASK_READS))
        tc.assert_same_state(mask, tc.snapshot(ft.oracle_mask(ok, case)), 'the mask')
        _masks[key] = mask
    return _masks[key]


def device_batch(hk, case, reads):
    if case.variant == 'packed':
        return hk.ReadBatch.from_packed(ft.pack_words(reads), ft.UNIFORM_LEN)
    return hk.ReadBatch(reads)


def count_args(hk, ok, case):
    mask = device_mask(hk, ok, case)
    return (case.nbands, case.band, mask, case.mask[1] if case.mask else 0, bool(case.mask[2]) if case.mask else False)


@pytest.mark.parametrize('case', ft.CASES, ids=ft.case_id)
def test_exact_unique_batch_by_batch(hk, ok, case):
    """track_exact_unique (kv_unique_new before every count): n_unique_kmers() after every batch, the tables at the end"""
    want = ft.oracle_tracked(ok, case)
    batches, prior = ft.batches_of(case)
    args = count_args(hk, ok, case)
    dev = ft.make(hk, case.kind, case.k, ft.geometry(ok, case.geometry))
    dev.consume_batch(device_batch(hk, case, prior))
    if case.variant == 'cleared':
        dev.clear()                         # lazy: the tables still hold the prior reads when tracking asks what is new
    dev.track_exact_unique(True)
    try:
        if case.variant != 'cleared':
            tc.assert_same_state(dev, want.prior_state, 'before tracking')
        total = 0
        for i, batch in enumerate(batches):
            assert dev.consume_batch(device_batch(hk, case, batch), *args) == want.consumed[i], i
            total += want.new[i]
            assert dev.n_unique_kmers() == total, 'batch {}: the oracle found {} new k-mers per batch'.format(i, want.new)
        tc.assert_same_state(dev, want.state, 'after the last batch')
    finally:
        dev.track_exact_unique(False)


def handles(batches):
    return (ctypes.c_void_p * max(1, len(batches)))(*[b._h for b in batches])


def abundance_distribution(lib, counts, tracking, batches):
    hist = np.zeros(65536, dtype=np.uint64)
    rc = lib.kv_abundance_distribution(counts._h, tracking._h, handles(batches), len(batches), hist.ctypes.data_as(_u64p))
    return rc, [int(v) for v in hist]


@pytest.mark.parametrize('n_batches', [1, 2, 4])
@pytest.mark.parametrize('d', ft.DIST_CASES, ids=ft.dist_id)
def test_abundance_distribution_over_an_array_of_batches(hk, ok, d, n_batches):
    """kv_abundance_distribution with 1, 2 and 4 batches in one call (an empty batch and one without k-mers among the four): the
    histogram and the tracking tables are the oracle's loop over the same reads, whatever the split; a second call goes on from the
    tracking state the first left behind"""
    from kevlar_amd import _lib
    lib = _lib.load()
    want = ft.oracle_dist(ok, d)
    counts = ft.make(hk, d.counts, d.k, ft.geometry(ok, d.counts_geometry))
    counts.consume_batch(hk.ReadBatch(ft.MAIN))
    tc.assert_same_state(counts, want.counts_state, 'the counts')
    tracking = ft.make(hk, d.tracking, d.k, ft.geometry(ok, d.tracking_geometry))
    tracking.consume_batch(hk.ReadBatch(ft.dist_prior(d)))
    tc.assert_same_state(tracking, want.prior_state, 'the tracking sketch before the first call')
    for call, reads in enumerate(ft.DIST_CALLS):
        batches = [hk.ReadBatch(part) for part in ft.dist_splits(reads, d.k, n_batches)]
        rc, hist = abundance_distribution(lib, counts, tracking, batches)
        assert rc == _lib.KV_OK, _lib.last_error()
        assert sum(hist[256:]) == 0
        got = {c: n for c, n in enumerate(hist) if n}
        assert got == {c: n for c, n in enumerate(want.hists[call]) if n}, 'call {}'.format(call)
        tc.assert_same_state(tracking, want.states[call], 'the tracking sketch after call {}'.format(call))
    tc.assert_same_state(counts, want.counts_state, 'the counts afterwards')


def unique_exact(lib, sketch, batches, nbands, band, mask, threshold, consume_masked):
    out = ctypes.c_uint64(12345)
    rc = lib.kv_unique_exact(sketch._h, handles(batches), len(batches), nbands, band, mask._h if mask is not None else None, threshold,
                             1 if consume_masked else 0, ctypes.byref(out))
    return rc, out.value


@pytest.mark.parametrize('n_batches', [1, 3])
@pytest.mark.parametrize('case', ft.EXACT_CASES, ids=ft.case_id)
def test_unique_exact_takes_the_sketch_for_empty_and_leaves_it_alone(hk, ok, case, n_batches):
    """kv_unique_exact over all batches at once: n_unique_kmers() of a fresh oracle sketch, although the sketch it is given holds counts
    ("an initially empty sketch": it reads the geometry, not the tables), the tables byte for byte as they were, and the sum of
    kv_unique_new before every kv_consume of a fresh device sketch"""
    from kevlar_amd import _lib
    lib = _lib.load()
    want = ft.oracle_exact(ok, case)
    held = ft.oracle_tracked(ok, case).prior_state
    parts, prior = ft.batches_of(case)
    if n_batches == 1:
        parts = [[r for part in parts for r in part]]
    batches = [hk.ReadBatch(part) for part in parts]
    nbands, band, mask, threshold, consume_masked = count_args(hk, ok, case)
    dev = ft.make(hk, case.kind, case.k, ft.geometry(ok, case.geometry))
    dev.consume_batch(hk.ReadBatch(prior))
    rc, got = unique_exact(lib, dev, batches, nbands, band, mask, threshold, consume_masked)
    assert rc == _lib.KV_OK, _lib.last_error()
    assert got == want
    tc.assert_same_state(dev, held, 'the sketch kv_unique_exact was given')
    fresh = ft.make(hk, case.kind, case.k, ft.geometry(ok, case.geometry))
    total, n_new, n = 0, ctypes.c_uint64(), ctypes.c_uint64()
    margs = (nbands, band, mask._h if mask is not None else None, threshold, 1 if consume_masked else 0)
    try:
        for batch in batches:
            assert lib.kv_unique_new(fresh._h, batch._h, *margs, ctypes.byref(n_new)) == _lib.KV_OK, _lib.last_error()
            assert lib.kv_consume(fresh._h, batch._h, *margs, ctypes.byref(n)) == _lib.KV_OK, _lib.last_error()
            total += n_new.value
    finally:
        lib.kv_unique_release()
    assert total == want
    tc.assert_same_state(fresh, ft.oracle_tracked(ok, case._replace(variant='cleared')).state, 'the fresh sketch after the batches')


def test_argument_errors_leave_the_next_call_working(hk, ok):
    """a null batch in the array, a band out of range, counts and tracking of different k: KV_ERR_ARG each, nothing changed, and the
    same call with good arguments answers as the oracle does"""
    from kevlar_amd import _lib
    lib = _lib.load()
    case = ft.EXACT_CASES[0]
    d = ft.DIST_CASES[0]
    parts, prior = ft.batches_of(case)
    batches = [hk.ReadBatch(part) for part in parts]
    with_null = (ctypes.c_void_p * 3)(batches[0]._h, None, batches[2]._h)
    out = ctypes.c_uint64()
    dev = ft.make(hk, case.kind, case.k, ft.geometry(ok, case.geometry))
    dev.consume_batch(hk.ReadBatch(prior))
    held = ft.oracle_tracked(ok, case).prior_state
    assert lib.kv_unique_exact(dev._h, with_null, 3, 0, 0, None, 0, 0, ctypes.byref(out)) == _lib.KV_ERR_ARG
    for nbands, band in ((4, 4), (4, -1), (-1, 0)):
        assert lib.kv_unique_exact(dev._h, handles(batches), 3, nbands, band, None, 0, 0, ctypes.byref(out)) == _lib.KV_ERR_ARG, (nbands, band)
        assert lib.kv_unique_new(dev._h, batches[0]._h, nbands, band, None, 0, 0, ctypes.byref(out)) == _lib.KV_ERR_ARG, (nbands, band)
    assert lib.kv_unique_new(dev._h, None, 0, 0, None, 0, 0, ctypes.byref(out)) == _lib.KV_ERR_ARG
    tc.assert_same_state(dev, held, 'after the refused calls')
    assert unique_exact(lib, dev, batches, 0, 0, None, 0, False) == (_lib.KV_OK, ft.oracle_exact(ok, case))
    try:
        assert lib.kv_unique_new(dev._h, batches[0]._h, 0, 0, None, 0, 0, ctypes.byref(out)) == _lib.KV_OK, _lib.last_error()
    finally:
        lib.kv_unique_release()
    assert out.value == ft.oracle_tracked(ok, case).new[0]

    want = ft.oracle_dist(ok, d)
    counts = ft.make(hk, d.counts, d.k, ft.geometry(ok, d.counts_geometry))
    counts.consume_batch(hk.ReadBatch(ft.MAIN))
    tracking = ft.make(hk, d.tracking, d.k, ft.geometry(ok, d.tracking_geometry))
    tracking.consume_batch(hk.ReadBatch(ft.dist_prior(d)))
    other_k = ft.make(hk, d.tracking, d.k + 2, ft.geometry(ok, d.tracking_geometry))
    hist = np.zeros(65536, dtype=np.uint64)
    whole = [hk.ReadBatch(ft.MAIN)]
    assert lib.kv_abundance_distribution(counts._h, other_k._h, handles(whole), 1, hist.ctypes.data_as(_u64p)) == _lib.KV_ERR_ARG
    halves = [hk.ReadBatch(part) for part in ft.dist_splits(ft.MAIN, d.k, 2)]
    with_null = (ctypes.c_void_p * 3)(halves[0]._h, None, halves[1]._h)
    assert lib.kv_abundance_distribution(counts._h, tracking._h, with_null, 3, hist.ctypes.data_as(_u64p)) == _lib.KV_ERR_ARG
    assert lib.kv_abundance_distribution(counts._h, tracking._h, handles(whole), -1, hist.ctypes.data_as(_u64p)) == _lib.KV_ERR_ARG
    tc.assert_same_state(tracking, want.prior_state, 'the tracking sketch after the refused calls')
    assert other_k.n_occupied() == 0
    rc, got = abundance_distribution(lib, counts, tracking, halves)
    assert rc == _lib.KV_OK and got == want.hists[0]
    tc.assert_same_state(tracking, want.states[0], 'the tracking sketch after the good call')
