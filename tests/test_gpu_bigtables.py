"""Sketches of 2^30 to 6e9 bins per table against the oracle: the sizes the project is built for (bench.py's cfg4-band tables of
1,999,999,973 bins, the README's `novel --memory 24G` with four tables of 6e9 bins), where the library changes its behaviour in
five places that the rest of the suite, which stops at 5e8 bins, never reaches:

  > 2^30 bins     stage A of the bin path: 64 coarse buckets, 1024-thread workgroups        (kv_bin_plan)
  < 2^31 bins     fast4: the super-k-mer count's 32-bit remainder, its sign in bit 31        (kv_fastmod32, k_skm_count)
  > 2^31 bins     the partitioned and super-k-mer counts decline: k_consume's atomics only   (kv_binned_eligible)
  2^31 .. 2^32    FP64 fastmod with bins that no longer fit an int32                         (kv_fastmod.h)
  >= 2^32 bins    Barrett fastmod, 64-bit bin indices, byte offsets beyond 4 GB              (kv_device.h, kv_novel_device.h, save / load)

The axis is table size on the paths the production dispatch picks by itself, plus the count paths KV_COUNT_PATH names; no tuning
variant is pinned.  Every comparison is against the oracle (oracle/kvoracle.c through okhmer, itself pinned at these sizes by
tests/test_oracle_bigtables.py) or, for the point queries and hash lists, against numpy's exact uint64 `%`; never device path
against device path alone.  Every count and scan asserts by launch count which kernel gave the result, and every size class asserts
on the ORACLE's tables that bins beyond the class boundary are in use.

Input: synth.trio_reads_packed(3_400_000, 30, 100), 1.02 M reads = 71.4 M k-mers per sample at k = 31: about the smallest family
for which the default dispatch still takes the super-k-mer count at 2e9 bins (kv_binned_eligible: expected * 32 >= pmax).

Cost.  The oracle keeps on the host every table the device holds; the largest single test is the [5999999989 + three 2.5e8] trio
of the scans, 3 x 6.75 GB of oracle tables, and the counts hold one oracle sketch (at most 8.8 GB) plus one 6 GB read buffer.
Measured on an MI355X box whose job limit is 322 GB of host memory (memory.max; MemTotal 3.1 TB): peak resident set 33.9 GB, far
below half the limit, so the trio keeps its four tables per sketch.  The save / load test writes a 6 GB file under tmp_path and
removes it: about 7 GB must be free there (79 GB were; no run-time skip).  The module took 295 s of wall time and the rest of the GPU
suite 560 s in the same job on the same box: 53 % where a quarter was the aim.  Oracle sketches that two tests need are shared
(oracle_counted), a KV_COUNT_PATH setting that ends in k_consume again is not byte-compared a second time, and the tables come back
through one page-locked buffer; what is left is the oracle's own counting (~140 s) and one byte compare per distinct kernel
(DESIGN.md section 2).  The module's last test prints the peak resident set.

G-edge31 (tables of 2^31 - 1, 2^30 +, 2^30 - and 65537 bins) showed a limit, not a wrong table: asked for by name, the super-k-mer
and partitioned counts decline it (the bin plan sizes its staging for the densest table: terabytes here) and k_consume counts it,
bit for bit.  The test asserts exactly that, reason included, and G-edge31-even puts the same switches through k_skm_count."""
import ctypes
import gc
import os

import numpy as np
import pytest

from bigtables_common import ALL_SIZES, COUNTER_MAX, FILLERS, P_BAND, P_MID, P_README, SWITCH_PRIMES, crafted_hashes, device_table, \
    expected_table, first_bin_above, first_difference, occupied, oracle_table, stored, storage_of, table_nbytes
from test_gpu_fullsize import Profiled, ascii_block, assert_hits_equal, host_cores, scan_all_ways

pytestmark = pytest.mark.gpu

L, K = 100, 31
NK = L - K + 1
G_BAND = [1999999973, 1999999943, 1999999927, 1999999913]
G_32 = [4294967291, 4294967311, P_MID, P_README]
# name -> (sketch class, primes, what runs with KV_COUNT_PATH unset / skm / binned / atomic)
GEOMETRIES = {
    'G-band': ('Counttable', G_BAND, ('skm', 'skm', 'bins', 'atomic')),
    # the smallest table is below the 2^20 floor of the default dispatch.  Asked for by name, the partitioned paths DECLINE: kv_bin_plan
    # sizes every segment for the densest table, so a 65537-bin table beside one of 2^31 - 1 bins asks for T x items x pmax / pmin x 4 B
    # = terabytes of staging; the plan answers KV_ERR_CAPACITY and the count falls through to k_consume.
    # The tables are held to the oracle all the same, and G-edge31-even takes the same switches through k_skm_count.
    'G-edge31': ('SmallCounttable', [2147483647, 1073741827, 1073741789, 65537], ('atomic', 'declined', 'declined', 'atomic')),
    # fast4 at the top of its range (2^31 - 1 and the prime before it) and both sides of the 2^30 switch in one plan the bin path can hold
    'G-edge31-even': ('SmallCounttable', [2147483647, 2147483629, 1073741827, 1073741789], ('skm', 'skm', 'bins', 'atomic')),
    # one table one prime past 2^31: nothing but k_consume may touch it, whatever is asked for
    'G-past31': ('Nodetable', FILLERS + [2147483659], ('atomic',) * 4),
    'G-32-bits': ('Nodetable', G_32, ('atomic',) * 4),
    'G-32-nibbles': ('SmallCounttable', G_32, ('atomic',) * 4),
    'G-readme-first': ('Counttable', [P_README] + FILLERS, ('atomic',) * 4),
    'G-readme-last': ('Counttable', FILLERS + [P_README], ('atomic',) * 4),
}
# the boundary each table size is there to cross: a non-zero bin of the ORACLE's table must lie beyond it
BOUNDARY = {p: 2**30 for p in G_BAND + [2147483647, 2147483629, 2147483659]}                          # (1073741827 has 3 bins beyond 2^30)
BOUNDARY.update({P_MID: 2**31, 4294967291: 2**31, 4294967311: 2**31, P_README: 2**32})      # (4294967311 has 15 bins beyond 2^32: nothing to ask there)
COUNT_SCOPES = ('k_skm_count', 'k_bin_hash_2bit', 'k_bin_hash_direct', 'k_bin_apply', 'k_consume')


@pytest.fixture(scope='module')
def family(hk):
    """the three samples: packed words, device batches, and the oracle's input (bases back to back, offsets)"""
    from kevlar_amd import synth
    packed = synth.trio_reads_packed(3_400_000, 30, L)
    assert packed['proband'].shape[0] == 1_020_000
    batches = {n: hk.ReadBatch.from_packed(w, L) for n, w in packed.items()}
    blocks = {n: ascii_block(w, L) for n, w in packed.items()}
    return packed, batches, blocks


@pytest.fixture(scope='module')
def readback(hk):
    """one host buffer for every table read of the module, as large as the largest table (6 GB); page-locked where torch can give
    that, so that a read is a DMA at link speed and not a staged copy"""
    nbytes = table_nbytes('byte', P_README)
    try:
        import torch
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy()
    except (ImportError, RuntimeError):
        return np.empty(nbytes, dtype=np.uint8)


# oracle sketches more than one test needs: (class, primes, sample) -> the tests that use it, so that the last one lets it go
SHARED = {('Nodetable', tuple(G_32), 'proband'): 2,                        # counts G-32-bits, save / load
          ('Counttable', (P_README,) + tuple(FILLERS), 'proband'): 2}      # counts G-readme-first, scans readme


@pytest.fixture(scope='module')
def oracle_counted(ok, family):
    """get(cls, primes, sample): the oracle sketch of that geometry filled with all reads of the sample by the threaded count; built
    once for the tests that share it (SHARED) and dropped after the last of them"""
    packed, batches, blocks = family
    cache, left = {}, dict(SHARED)

    def get(cls, primes, sample='proband'):
        key = (cls, tuple(primes), sample)
        ref = cache.get(key)
        if ref is None:
            n_reads = packed[sample].shape[0]
            ref = getattr(ok, cls)(K, 0, 0, primes=list(primes))
            assert ok.consume_reads_mt(ref, blocks[sample][0], blocks[sample][1], n_reads, host_cores()) == n_reads * NK
            if key in left:
                cache[key] = ref
        if key in left:
            left[key] -= 1
            if left[key] == 0:
                cache.pop(key, None)
        return ref
    yield get
    cache.clear()


def test_the_sizes_are_what_the_prime_search_gives(hk, ok):
    for bits, (below, above) in SWITCH_PRIMES.items():
        assert hk.primes_below(2**bits, 1) == ok.primes_below(2**bits, 1) == [below] and below < 2**bits < above
    assert hk.primes_below(2e9, 4) == ok.primes_below(2e9, 4) == G_BAND and G_BAND[0] == P_BAND
    assert hk.primes_below(3e9, 1) == [P_MID] and hk.primes_below(6e9, 1) == [P_README]
    assert hk.primes_below(2.5e8, 3) == ok.primes_below(2.5e8, 3) == FILLERS
    assert len(ALL_SIZES) == 11


def which_ran(prof):
    return {s: prof.count(s) for s in COUNT_SCOPES}


def assert_count_path(ran, want, what):
    if want == 'skm':
        good = ran['k_skm_count'] == 1 and ran['k_consume'] == 0 and ran['k_bin_hash_2bit'] + ran['k_bin_hash_direct'] == 0
    elif want == 'bins':
        good = ran['k_skm_count'] == 0 and ran['k_consume'] == 0 and ran['k_bin_hash_2bit'] + ran['k_bin_hash_direct'] == 1 and ran['k_bin_apply'] == 1
    else:
        good = ran['k_consume'] == 1 and ran['k_skm_count'] == 0 and ran['k_bin_apply'] == 0 and ran['k_bin_hash_2bit'] + ran['k_bin_hash_direct'] == 0
    assert good, '{}: expected the {} count, launches were {}'.format(what, want, ran)
    if want == 'declined':
        # (kv_last_error() keeps the last message, a successful call does not clear it: it is this call's because nothing else in
        # this module declines for capacity, and the launches above show that neither partitioned path got as far as a kernel)
        from kevlar_amd import _lib
        assert 'staging buffers' in _lib.last_error(), '{}: declined, but not for the staging buffers: {!r}'.format(what, _lib.last_error())


def assert_same_tables(dev, ref, ok, buf, what, twice=False):
    """every byte of every table, and n_occupied, against the oracle sketch `ref` (twice: against its saturating double)"""
    sizes = ref.hashsizes()
    assert dev.hashsizes() == sizes
    storage = storage_of(ref)
    for t, size in enumerate(sizes):
        got, want = device_table(dev, t, buf), oracle_table(ok, ref, t)
        diff = first_difference(got, want, storage, twice=twice)
        assert diff is None, '{}: table {} ({} bins, {}): bin {} holds {}, the oracle {}'.format(what, t, size, storage, *diff)
    assert dev.n_occupied() == ref.n_occupied(), what


def set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv('KV_COUNT_PATH', raising=False)
    else:
        monkeypatch.setenv('KV_COUNT_PATH', path)


def assert_reference_crosses_the_boundaries(ok, ref, name):
    """conditions on the REFERENCE: if one fails the input is wrong, not the kernel"""
    storage = storage_of(ref)
    for t, size in enumerate(ref.hashsizes()):
        view = oracle_table(ok, ref, t)
        if size in BOUNDARY:
            assert first_bin_above(view, storage, BOUNDARY[size]), '{}: the oracle\'s table {} ({} bins) has nothing beyond bin {}'.format(name, t, size, BOUNDARY[size])
        head = view[:1 << 26]
        if storage == 'nibble':
            assert bool(((head & np.uint8(15)) == 15).any() or ((head >> 4) == 15).any()), 'no saturated nibble'
        if name == 'G-band':
            assert bool((head > 30).any()), 'no count above 30'


# ---- 1 + 2: counts equal the oracle, every table byte, on every count path ---------------------------------------------------

@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_counts_equal_the_oracle(hk, ok, family, oracle_counted, readback, monkeypatch, name):
    """every table byte and n_occupied on every count path.  Where a setting of KV_COUNT_PATH provably ends in the kernel another
    setting of the same geometry was already compared under -- k_consume and nothing else, by its launch count -- the kernel, the
    k-mer count and n_occupied are asserted and the byte compare is not repeated: same kernel, same arguments, same tables"""
    packed, batches, blocks = family
    cls, primes, expect = GEOMETRIES[name]
    n_reads = packed['proband'].shape[0]
    ref = oracle_counted(cls, primes)
    assert_reference_crosses_the_boundaries(ok, ref, name)
    buf = readback
    by_consume = False                      # k_consume's tables of this geometry were compared byte by byte
    for path, want in zip((None, 'skm', 'binned', 'atomic'), expect):
        what = '{}, KV_COUNT_PATH={}'.format(name, path)
        set_path(monkeypatch, path)
        dev = getattr(hk, cls)(K, 0, 0, primes=primes)
        with Profiled(hk) as prof:
            assert dev.consume_batch(batches['proband']) == n_reads * NK
            assert_count_path(which_ran(prof), want, what)
        if want in ('atomic', 'declined') and by_consume:
            assert dev.hashsizes() == ref.hashsizes() and dev.n_occupied() == ref.n_occupied(), what
        else:
            assert_same_tables(dev, ref, ok, buf, what)
            by_consume = by_consume or want in ('atomic', 'declined')
        if path is None:
            # the lazy zero of kv_sketch_clear and the apply stage at these sizes; then the saturating add
            dev.clear()
            with Profiled(hk) as prof:
                assert dev.consume_batch(batches['proband']) == n_reads * NK
                assert_count_path(which_ran(prof), want, what + ' after clear()')
            assert_same_tables(dev, ref, ok, buf, what + ' after clear()')
            assert dev.consume_batch(batches['proband']) == n_reads * NK
            assert_same_tables(dev, ref, ok, buf, what + ', the same batch twice', twice=True)
        del dev
        gc.collect()
    del ref
    gc.collect()


# ---- 3: masked and banded counts ------------------------------------------------------------------------------------------------

MASK_PRIMES = [4294967311, P_README]
N_MASKED = 300_000           # the oracle's masked leg is single-threaded


@pytest.fixture(scope='module')
def masks(hk, ok, family, readback):
    """a Nodetable of 4294967311 and 5999999989 bins (1.3 GB) filled from the mother's reads, on the device and in the oracle -- equal"""
    packed, batches, blocks = family
    n_reads = packed['mother'].shape[0]
    dev, ref = hk.Nodetable(K, 0, 0, primes=MASK_PRIMES), ok.Nodetable(K, 0, 0, primes=MASK_PRIMES)
    assert dev.consume_batch(batches['mother']) == n_reads * NK
    assert ok.consume_reads_mt(ref, blocks['mother'][0], blocks['mother'][1], n_reads, host_cores()) == n_reads * NK
    assert_same_tables(dev, ref, ok, readback, 'the mask')
    assert first_bin_above(oracle_table(ok, ref, 1), 'bit', 2**32)
    return dev, ref


@pytest.mark.parametrize('name', ['G-band', 'G-32-bits'])
def test_masked_counts_equal_the_oracle(hk, ok, family, masks, readback, monkeypatch, name):
    """a mask switches fast4 off: at G-band this is the general drain skm_count_kmer at 2e9 bins; the mask's own probe has 64-bit bins"""
    packed, batches, blocks = family
    cls, primes, expect = GEOMETRIES[name]
    dev_mask, ref_mask = masks
    part = hk.ReadBatch.from_packed(packed['proband'][:N_MASKED], L)
    bases, offs_p, _ = blocks['proband']
    buf = readback
    for consume_masked in (False, True):
        by_consume = False
        ref = getattr(ok, cls)(K, 0, 0, primes=primes)
        n_ref = ok.consume_reads(ref, bases, offs_p, N_MASKED, mask=ref_mask, threshold=0, consume_masked=consume_masked)
        # (threshold 0: consume_masked keeps every k-mer -- mask.get() >= 0 --, the plain form keeps those the mother does not have)
        assert n_ref == N_MASKED * NK if consume_masked else 0 < n_ref < N_MASKED * NK // 4
        for path, want in zip(('skm', 'binned', 'atomic'), expect[1:]):
            what = '{}, mask, consume_masked={}, KV_COUNT_PATH={}'.format(name, consume_masked, path)
            set_path(monkeypatch, path)
            dev = getattr(hk, cls)(K, 0, 0, primes=primes)
            with Profiled(hk) as prof:
                assert dev.consume_batch(part, mask=dev_mask, threshold=0, consume_masked=consume_masked) == n_ref, what
                assert_count_path(which_ran(prof), want, what)
            if want == 'atomic' and by_consume:             # (k_consume again, as in test_counts_equal_the_oracle)
                assert dev.n_occupied() == ref.n_occupied(), what
            else:
                assert_same_tables(dev, ref, ok, buf, what)
                by_consume = by_consume or want == 'atomic'
            del dev
            gc.collect()
        del ref
        gc.collect()


@pytest.mark.parametrize('name', ['G-band', 'G-32-nibbles'])
def test_banded_counts_equal_the_oracle(hk, ok, family, readback, monkeypatch, name):
    """the whole proband, first and last of eight hash bands, on the default path (an eighth of 71 M k-mers is too sparse for the
    partitioned counts at 2e9 bins: k_consume at both geometries)"""
    packed, batches, blocks = family
    cls, primes, _ = GEOMETRIES[name]
    n_reads = packed['proband'].shape[0]
    bases, offs_p, _ = blocks['proband']
    set_path(monkeypatch, None)
    buf = readback
    for band in (0, 7):
        ref = getattr(ok, cls)(K, 0, 0, primes=primes)
        n_ref = ok.consume_reads_mt_banded(ref, bases, offs_p, n_reads, host_cores(), 8, band)
        assert n_reads * NK // 10 < n_ref < n_reads * NK // 6
        dev = getattr(hk, cls)(K, 0, 0, primes=primes)
        with Profiled(hk) as prof:
            assert dev.consume_batch(batches['proband'], 8, band) == n_ref
            assert_count_path(which_ran(prof), 'atomic', '{}, band {} of 8'.format(name, band))
        assert_same_tables(dev, ref, ok, buf, '{}, band {} of 8'.format(name, band))
        del dev, ref
        gc.collect()


# ---- 4: scans equal the oracle, every hit -------------------------------------------------------------------------------------------

SCANS = {
    'band': ('Counttable', [P_BAND] + FILLERS, 6, 1, True),             # (class, primes, case_min, ctrl_max, the count is the super-k-mer one)
    'mid': ('Counttable', [P_MID] + FILLERS, 6, 1, False),
    'readme': ('Counttable', [P_README] + FILLERS, 6, 1, False),
    'nibbles': ('SmallCounttable', [4294967311, P_README], 6, 1, False),
}


@pytest.mark.parametrize('name', list(SCANS))
def test_scans_equal_the_oracle(hk, ok, family, oracle_counted, monkeypatch, name):
    """trios with the large table at index 0 -- the scan's first probe and k_case_bits --: every hit of every scan kernel (the walk, the
    tile scan, the 2-bit tile scan a small batch takes, and the distinct list behind a hinted count) against the oracle's scan loop.
    The distinct list exists only behind a super-k-mer count, and that count declines tables above 2^31 bins: k_skm_novel_list is
    proven at the 'band' trio alone, the first scan of the three others is a walk and is asserted to be one"""
    import torch
    from kevlar_amd import bandmerge
    packed, batches, blocks = family
    cls, primes, case_min, ctrl_max, by_skm = SCANS[name]
    names = ('mother', 'father', 'proband')
    n_reads = packed['proband'].shape[0]
    cores = host_cores()
    set_path(monkeypatch, None)
    monkeypatch.setenv('KV_SKM_DL', '1')           # (a stream's first batch gets no list unless asked: bench.py asks the same way)
    dev = {n: getattr(hk, cls)(K, 0, 0, primes=primes) for n in names}
    dev['proband'].expect_scan()
    with Profiled(hk) as prof:
        for n in names:
            assert dev[n].consume_batch(batches[n]) == n_reads * NK
        ran = which_ran(prof)
        assert (ran['k_skm_count'], ran['k_consume']) == ((3, 0) if by_skm else (0, 3)), ran
    cases, ctrls = [dev['proband']], [dev['mother'], dev['father']]
    first = None
    if not by_skm:
        with Profiled(hk) as prof:          # no list behind k_consume: the first scan cuts the reads and walks
            first = hk.novel_scan(cases, ctrls, batches['proband'], case_min, ctrl_max)[:3]
            assert prof.count('k_skm_novel') == 1 and prof.count('k_skm_novel_list') + prof.count('k_novel_mark') + prof.count('k_novel_mark_2bit') == 0
    scans = scan_all_ways(hk, cases, ctrls, batches['proband'], case_min, ctrl_max, first_from_list=by_skm)
    if first is not None:
        scans['list'] = first               # (what scan_all_ways ran first there was one more walk, whose kernel it does not assert)
    n_small = 50_000                                # 3.5 M k-mers: below the super-k-mer threshold
    small = hk.ReadBatch.from_packed(packed['proband'][:n_small], L)
    with Profiled(hk) as prof:
        scans['small'] = hk.novel_scan(cases, ctrls, small, case_min, ctrl_max)[:3]
        assert prof.count('k_novel_mark_2bit') == 1 and prof.count('k_novel_mark') + prof.count('k_skm_novel') + prof.count('k_skm_novel_list') == 0
    masked = None
    if name == 'readme':
        mask = torch.zeros((n_reads * NK + 31) // 32, dtype=torch.int32, device='cuda')
        masked = hk.novel_scan(cases, ctrls, batches['proband'], case_min, ctrl_max, mask_ptr=mask.data_ptr(), mask_stride=NK)[:3]
        torch.cuda.synchronize()
        masked = (masked, bandmerge.mask_to_hits(mask, NK))
        del mask
    ref = {n: oracle_counted(cls, primes, n) for n in names}
    assert first_bin_above(oracle_table(ok, ref['proband'], 0), storage_of(ref['proband']), BOUNDARY[primes[0]])
    assert dev['proband'].n_occupied() == ref['proband'].n_occupied()
    want = ok.novel_scan_mt([ref['proband']], [ref['mother'], ref['father']], blocks['proband'][0], blocks['proband'][1], n_reads, K,
                            case_min, ctrl_max, cores)
    assert len(want[0]) >= 1000, 'the oracle finds {} hits: an empty answer must not pass'.format(len(want[0]))
    for way in ('list', 'walk', 'tiles'):
        assert_hits_equal(scans[way], want, '{} trio, scan by {}'.format(name, way if by_skm or way != 'list' else 'the first walk'))
    sel = want[0] < n_small
    assert int(sel.sum()) >= 20
    assert_hits_equal(scans['small'], (want[0][sel], want[1][sel], want[2][sel]), '{} trio, the first {} reads by the 2-bit tile scan'.format(name, n_small))
    if masked is not None:
        assert_hits_equal(masked[0], want, 'readme trio, scan with a bit mask')
        assert np.array_equal(masked[1][0], want[0]) and np.array_equal(masked[1][1], want[1].astype(np.uint32)), 'the bit mask and the hit list differ'
    del dev, ref, cases, ctrls
    gc.collect()


# ---- 5: point queries and hash lists, with hashes chosen to hurt ------------------------------------------------------------------------

POINT_CASES = [('Nodetable', p) for p in ALL_SIZES] + [('SmallCounttable', 4294967291), ('SmallCounttable', 4294967311)] + \
    [('Counttable', 2147483647), ('Counttable', 2147483659), ('Counttable', P_README)]
WEIGHTS = np.array([1, 127, 128, 255, 256, 1000], dtype=np.int64)


def assert_table_is(dev, uniq, vals, buf, what):
    """the counters at the touched bins, nothing set anywhere else in the whole table, and n_occupied"""
    storage = storage_of(dev)
    view = device_table(dev, 0, buf)
    got = stored(view, storage, uniq)
    bad = np.flatnonzero(got != vals)
    assert len(bad) == 0, '{}: bin {} holds {}, expected {} ({} bins differ)'.format(what, int(uniq[bad[0]]), int(got[bad[0]]), int(vals[bad[0]]), len(bad))
    assert occupied(view, storage) == len(uniq), '{}: a counter outside the touched bins is set'.format(what)
    assert dev.n_occupied() == len(uniq), what


@pytest.mark.parametrize('cls,size', POINT_CASES, ids=['{}-{}'.format(c, p) for c, p in POINT_CASES])
def test_point_queries_and_hash_lists(hk, readback, cls, size):
    """m * size + d, the top of the 64-bit range, the edges of a double's mantissa and random hashes through the device's FP64 pipe and
    __umul64hi: get / add, the plain and the strided hash list, the weighted list -- against h % size in numpy's uint64"""
    import torch
    rng = np.random.default_rng(size & 0xffffffff)
    new = lambda: getattr(hk, cls)(K, 0, 0, primes=[size])
    h = crafted_hashes(size, rng)
    what = '{} of {} bins'.format(cls, size)
    dev = new()
    storage = storage_of(dev)
    buf = readback
    uniq, vals = expected_table(h, size, storage)
    assert int(uniq[0]) == 0 and int(uniq[-1]) == size - 1 and vals.max() == COUNTER_MAX[storage]
    assert not dev.get_hashes(h).any()
    with Profiled(hk) as prof:
        was_new = dev.add_hashes(h)
        assert prof.count('k_add_hashes') == 1
    assert int(np.count_nonzero(was_new)) == len(uniq), what          # (which of several hashes of a bin got the answer is the device's business)
    want = vals[np.searchsorted(uniq, h % np.uint64(size))]
    got = dev.get_hashes(h)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, '{}: get({}) = {}, expected {}'.format(what, int(h[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    assert_table_is(dev, uniq, vals, buf, what + ', add_hashes')
    del dev
    d_h = torch.from_numpy(h.view(np.int64)).cuda()
    d_pairs = torch.full((len(h), 2), -1, dtype=torch.int64, device='cuda')           # (hash, junk) pairs: stride 2
    d_pairs[:, 0] = d_h
    for stride, tensor in ((1, d_h), (2, d_pairs)):
        dev = new()
        with Profiled(hk) as prof:
            assert dev.consume_hashes(tensor.data_ptr(), len(h), stride) == len(h)
            assert prof.count('k_add_hashes') == 1 and prof.count('k_bin_list') == 0
        assert np.array_equal(dev.get_hashes(h), want), what
        assert_table_is(dev, uniq, vals, buf, '{}, consume_hashes stride {}'.format(what, stride))
        del dev
    w = WEIGHTS[np.arange(len(h)) % len(WEIGHTS)]
    d_pairs[:, 1] = torch.from_numpy(w).cuda()
    uniq_w, vals_w = expected_table(h, size, storage, w)
    dev = new()
    with Profiled(hk) as prof:
        assert dev.consume_hashes_weighted(d_pairs.data_ptr(), len(h)) == int(w.sum())
        assert prof.count('k_add_hashes_weighted') == 1 and prof.count('k_bin_list_w') == 0
    assert np.array_equal(dev.get_hashes(h), vals_w[np.searchsorted(uniq_w, h % np.uint64(size))]), what
    assert_table_is(dev, uniq_w, vals_w, buf, what + ', consume_hashes_weighted')
    del dev, d_h, d_pairs
    gc.collect()


@pytest.mark.parametrize('size', [1073741789, 1073741827, P_BAND, 2147483647])
def test_long_hash_lists_go_through_the_bin_path(hk, readback, size):
    """size / 32 random hashes (at least 2^22): kv_binned_eligible sends a list of this density through k_bin_list -- with 64 coarse
    buckets and 1024-thread workgroups above 2^30 bins.  Nibble counters: the storage is not the point, a weight still shows."""
    import torch
    rng = np.random.default_rng(size & 0xffffffff)
    n = size // 32 + 1
    assert n >= 1 << 22 and n * 32 >= size
    h = rng.integers(0, 2**64, n, dtype=np.uint64)
    h[:7] = np.array([0, size - 1, size, 2 * size - 1, 2**64 - 1, (2**64 - 1) // size * size, (2**64 - 1) // size * size - 1], dtype=np.uint64)
    bins = h % np.uint64(size)
    uniq, counts = np.unique(bins, return_counts=True)
    assert int(uniq[0]) == 0 and int(uniq[-1]) == size - 1 and int(uniq[len(uniq) // 2]) > size // 4
    buf = readback
    d_pairs = torch.empty((n, 2), dtype=torch.int64, device='cuda')
    d_pairs[:, 0] = torch.from_numpy(h.view(np.int64)).cuda()
    # every hash of a bin carries the same weight, so that the expected counter needs no sum over 67 M items
    w_of = lambda b: WEIGHTS[(b % np.uint64(len(WEIGHTS))).astype(np.int64)]
    w = w_of(bins)
    d_pairs[:, 1] = torch.from_numpy(w).cuda()
    what = 'SmallCounttable of {} bins, {} hashes'.format(size, n)
    dev = hk.SmallCounttable(K, 0, 0, primes=[size])
    with Profiled(hk) as prof:
        assert dev.consume_hashes(d_pairs.data_ptr(), n, 2) == n
        assert prof.count('k_bin_list') == 1 and prof.count('k_add_hashes') == 0, what
    assert_table_is(dev, uniq, np.minimum(counts, 15).astype(np.uint8), buf, what + ', consume_hashes')
    del dev
    dev = hk.SmallCounttable(K, 0, 0, primes=[size])
    with Profiled(hk) as prof:
        assert dev.consume_hashes_weighted(d_pairs.data_ptr(), n) == int(w.sum())
        assert prof.count('k_bin_list_w') == 1 and prof.count('k_add_hashes_weighted') == 0, what
    assert_table_is(dev, uniq, np.minimum(counts * w_of(uniq), 15).astype(np.uint8), buf, what + ', consume_hashes_weighted')
    del dev, d_pairs
    gc.collect()


# ---- 6: save, load, occupancy ---------------------------------------------------------------------------------------------------------------

def test_save_and_load_beyond_4_gb(hk, ok, family, oracle_counted, readback, tmp_path):
    """a Counttable of 5999999989 bins saved by the device (a 6 GB file under tmp_path, removed here; about 7 GB must be free) and
    loaded by the oracle; the Nodetable of G-32 both ways, with the occupancy recount of a load (kv_sketch_refresh_occupancy)"""
    packed, batches, blocks = family
    n_reads = packed['proband'].shape[0]
    path = str(tmp_path / 'big.ct')
    dev = hk.Counttable(K, 0, 0, primes=[P_README])
    assert dev.consume_batch(batches['proband']) == n_reads * NK
    try:
        dev.save(path)
        assert os.path.getsize(path) > P_README
        back = ok.Counttable.load(path)
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert back.hashsizes() == [P_README] and back.ksize() == K
    view = oracle_table(ok, back, 0)
    diff = first_difference(device_table(dev, 0, readback), view, 'byte')
    assert diff is None, 'saved Counttable: bin {} was {} on the device, {} in the file'.format(*diff)
    assert first_bin_above(view, 'byte', 2**32)
    assert back.n_occupied() == dev.n_occupied() == occupied(view, 'byte')
    del dev, back, view
    gc.collect()
    ref = oracle_counted('Nodetable', G_32)
    dev = hk.Nodetable(K, 0, 0, primes=G_32)
    assert dev.consume_batch(batches['proband']) == n_reads * NK
    buf = readback
    p_dev, p_ref = str(tmp_path / 'dev.nt'), str(tmp_path / 'ref.nt')
    try:
        dev.save(p_dev)
        ref.save(p_ref)
        from_dev, from_ref = ok.Nodetable.load(p_dev), hk.Nodetable.load(p_ref)
    finally:
        for p in (p_dev, p_ref):
            if os.path.exists(p):
                os.remove(p)
    assert from_dev.hashsizes() == G_32 and from_ref.hashsizes() == G_32 and from_ref.ksize() == K
    for t in range(4):
        assert np.array_equal(oracle_table(ok, from_dev, t), oracle_table(ok, ref, t)), 'device save -> oracle load, table {}'.format(t)
    assert from_dev.n_occupied() == ref.n_occupied()
    assert_same_tables(from_ref, ref, ok, buf, 'oracle save -> device load')
    assert from_ref.n_occupied() == occupied(oracle_table(ok, ref, 0), 'bit')
    del dev, ref, from_dev, from_ref
    gc.collect()


# ---- 7: dist and the exact distinct count ---------------------------------------------------------------------------------------------------------

N_SINGLE = 200_000          # reads of the oracle's single-thread legs


def test_abundance_distribution_with_2_pow_32_bins(hk, ok, family, readback):
    """`kevlar dist`'s second pass with one table of 4294967311 bins: the histogram and the tracking table against the oracle's"""
    packed, batches, blocks = family
    n_reads = packed['proband'].shape[0]
    size = SWITCH_PRIMES[32][1]
    dev_counts, ref_counts = hk.Counttable(K, 0, 0, primes=[size]), ok.Counttable(K, 0, 0, primes=[size])
    assert dev_counts.consume_batch(batches['proband']) == n_reads * NK
    assert ok.consume_reads_mt(ref_counts, blocks['proband'][0], blocks['proband'][1], n_reads, host_cores()) == n_reads * NK
    dev_track, ref_track = hk.Nodetable(K, 0, 0, primes=[size]), ok.Nodetable(K, 0, 0, primes=[size])
    part = hk.ReadBatch.from_packed(packed['proband'][:N_SINGLE], L)
    got = dev_counts.abundance_distribution(part, dev_track)
    hist = (ctypes.c_uint64 * 65536)()
    bases = blocks['proband'][0]
    for i in range(N_SINGLE):
        ok.lib.kvo_abundance_distribution(ref_counts._h, ref_track._h, bases[i * L:(i + 1) * L], L, hist)
    want = list(hist)
    assert got == want
    assert sum(want) > 1_000_000 and sum(1 for v in want if v) > 20
    assert_same_tables(dev_track, ref_track, ok, readback, 'tracking table of dist')
    assert first_bin_above(oracle_table(ok, ref_track, 0), 'bit', 2**31)
    del dev_counts, ref_counts, dev_track, ref_track
    gc.collect()


def test_exact_distinct_count_with_2_pow_32_bins(hk, ok, family, readback):
    """track_exact_unique() with a table of 4294967311 bins: the first-toucher array is 4 bytes per bin, 17 GB.  consume_batch() swallows
    a capacity error of kv_unique_new and falls back to the estimate, so the call is also made directly and its return code seen"""
    from kevlar_amd import _lib
    packed, batches, blocks = family
    size = SWITCH_PRIMES[32][1]
    part = hk.ReadBatch.from_packed(packed['proband'][:N_SINGLE], L)
    ref = ok.Nodetable(K, 0, 0, primes=[size])
    assert ok.consume_reads(ref, blocks['proband'][0], blocks['proband'][1], N_SINGLE) == N_SINGLE * NK
    want = ref.n_unique_kmers()
    assert 1_000_000 < want < N_SINGLE * NK
    dev = hk.Nodetable(K, 0, 0, primes=[size])
    fresh = ctypes.c_uint64()
    rc = _lib.load().kv_unique_new(dev._h, part._h, 0, 0, None, 0, 0, ctypes.byref(fresh))
    assert rc == 0, 'kv_unique_new returned {} for a table of {} bins'.format(rc, size)
    assert fresh.value == want
    dev.track_exact_unique(True)
    try:
        assert dev.consume_batch(part) == N_SINGLE * NK
        assert dev._exact is not None, 'consume_batch fell back to the estimate'
        assert dev.n_unique_kmers() == want
        assert_same_tables(dev, ref, ok, readback, 'tracked Nodetable')
    finally:
        dev.track_exact_unique(False)
    del dev, ref
    gc.collect()


def test_report_peak_host_memory():
    """prints the process's peak resident set (with -s, or in the captured output): the figure DESIGN.md section 2 records"""
    import resource
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print('peak resident set of this process: {:.1f} GB'.format(peak / 1e9))
    assert peak > 0
