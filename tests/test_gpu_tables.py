"""Sketches of 1 to 16 tables (KV_MAX_TABLES), scans of up to 16 samples (KV_MAX_SAMPLES) whose sketches differ in table count and
storage: the kernels branch on both numbers, and the rest of the suite counts into (k, size, 4) sketches and scans with two or three
controls.  Here every count path -- the atomic kernel, the partition, the super-k-mer count -- meets every table count (five tables or
more must land on the atomic kernel whatever is asked for; fewer than four, tables below 2^16 bins or a mask take the general drain of
k_skm_count, not its four-table form), every scan kernel meets samples of 1, 2, 3, 4, 6, 9, 11 and 16 tables in byte, nibble and bit
storage side by side, with the parents behind the eight controls the list scan's predicate unrolls, and the other consumers of the
table count (point queries, hash lists, the exact distinct-k-mer figure, the abundance distribution, files) meet 1, 5, 7 and 16.
Every comparison is exact against the CPU oracle -- table bytes, occupancy, k-mers consumed, hits as (read, offset, abundances) --
and the launch counts say which kernel answered.  tests/test_tables_reference.py holds, with the oracle alone, that these inputs tell
a missing loop from a present one."""
import os

import numpy as np
import pytest

import tables_common as tc
from tables_common import launches

pytestmark = pytest.mark.gpu

KNOBS = ('KV_COUNT_PATH', 'KV_NOVEL_PATH', 'KV_SKM_BUCKET_KMERS', 'KV_SKM_DL', 'KV_BIN_2BIT')
PATHS = ('atomic', 'binned', 'skm')
SCAN_KERNELS = ('k_skm_novel_list', 'k_skm_novel', 'k_novel_mark', 'k_novel_mark_2bit')


@pytest.fixture
def prof():
    """launch counts on, every knob a test sets popped again"""
    from kevlar_amd import _lib
    lib = _lib.load()
    lib.kv_prof_reset()
    lib.kv_prof_enable(1)
    yield lib
    lib.kv_prof_enable(0)
    for name in KNOBS:
        os.environ.pop(name, None)


def pin_count(path):
    if path:
        os.environ['KV_COUNT_PATH'] = path
    else:
        os.environ.pop('KV_COUNT_PATH', None)
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'


def assert_count_kernels(path, ntables, n):
    """n batches were counted into a sketch of `ntables` tables with `path` asked for by name"""
    ran = {name: launches(name) for name in ('k_consume', 'k_bin_apply', 'k_bin_apply_w', 'k_skm_count')}
    if path == 'atomic' or ntables > tc.BIN_MAX_T:
        assert ran == {'k_consume': n, 'k_bin_apply': 0, 'k_bin_apply_w': 0, 'k_skm_count': 0}, (path, ntables, ran)
    elif path == 'binned':
        assert ran == {'k_consume': 0, 'k_bin_apply': n, 'k_bin_apply_w': 0, 'k_skm_count': 0}, (path, ntables, ran)
    else:
        assert ran == {'k_consume': 0, 'k_bin_apply': 0, 'k_bin_apply_w': n, 'k_skm_count': n}, (path, ntables, ran)


def two_batches(hk, ok, prof, spec, k, first='proband', nbands=0, band=0):
    """`first`, then the mother's reads on top, through each path by name: k-mers consumed, table bytes and occupancy after either"""
    want = tc.oracle_two_batches(ok, spec, k, first=first, nbands=nbands, band=band)
    ntables = len(tc.primes_of(ok, spec))
    # the first batch as packed words (the front ends that hash from the 2-bit form), the second as text (the tile front ends)
    batches = [hk.ReadBatch.from_packed(tc.words(first), tc.READ_LEN) if first in ('proband',) else hk.ReadBatch(tc.reads(first)),
               hk.ReadBatch(tc.reads('mother'))]
    out = None
    for path in PATHS:
        pin_count(path)
        prof.kv_prof_reset()
        dev = tc.make(hk, spec, k, ok)
        for i, (batch, (n, state)) in enumerate(zip(batches, want)):
            if i == 1:
                os.environ['KV_BIN_2BIT'] = '0'
            assert dev.consume_batch(batch, nbands, band) == n, (path, i)
            tc.assert_same_state(dev, state, '{} path, batch {}'.format(path, i))
        os.environ.pop('KV_BIN_2BIT')
        assert_count_kernels(path, ntables, 2)
        if path == 'binned' and ntables <= tc.BIN_MAX_T and first == 'proband':
            assert launches('k_bin_hash_2bit') == 1 and launches('k_bin_hash_direct') == 1
        out = dev
    return out


@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('geometry', list(tc.COUNT_GEOMETRIES))
def test_every_count_path_at_every_table_count(hk, ok, prof, geometry, k):
    two_batches(hk, ok, prof, tc.COUNT_GEOMETRIES[geometry], k)


@pytest.mark.parametrize('k', tc.KS)
def test_three_tables_one_band_of_four(hk, ok, prof, k):
    two_batches(hk, ok, prof, tc.COUNT_GEOMETRIES['C3x3e5'], k, nbands=4, band=3)


@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('geometry,top', [('C3x3e5', 255), ('S3x3e5', 15)])
def test_three_tables_skew_saturates_every_table(hk, ok, prof, geometry, top, k):
    """700 copies of one read of one k-mer: weights split at 128, segments overflowing into the spill list, and a counter that stops at
    255 / 15 in each of the three tables"""
    from bigtables_common import stored, storage_of
    spec = tc.COUNT_GEOMETRIES[geometry]
    dev = two_batches(hk, ok, prof, spec, k, first='skew')
    assert dev.get('A' * k) == top
    h = dev.hash('A' * k)
    for t, size in enumerate(dev.hashsizes()):
        view = np.frombuffer(dev.table_bytes(t), dtype=np.uint8)
        assert int(stored(view, storage_of(dev), [h % size])[0]) == top, t


@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('case', list(tc.MASK_CASES))
def test_mask_and_target_of_different_table_counts_and_storages(hk, ok, prof, case, k):
    mask_spec, threshold, target = tc.MASK_CASES[case]
    ntables = len(tc.primes_of(ok, target))
    pin_count(None)
    mask = tc.make(hk, mask_spec, k, ok)
    mask.consume_batch(hk.ReadBatch(tc.reads(mask_spec.reads)))
    tc.assert_same_state(mask, tc.snapshot(tc.oracle_sketch(ok, mask_spec, k)), 'the mask')
    batch = hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN)
    for consume_masked in (False, True):
        n, state = tc.oracle_masked(ok, case, k, consume_masked)
        for path in PATHS:
            pin_count(path)
            prof.kv_prof_reset()
            dev = tc.make(hk, target, k, ok)
            assert dev.consume_batch(batch, 0, 0, mask, threshold, consume_masked) == n, (path, consume_masked)
            tc.assert_same_state(dev, state, '{} path, consume_masked {}'.format(path, consume_masked))
            assert_count_kernels(path, ntables, 1)


# ---- scans ------------------------------------------------------------------------------------------------------------------------
def counted_on_device(hk, ok, scan, k, hint=True):
    """the device's sketches of a scan, the controls counted first and the cases last (the last case's buckets, and with the hint its
    distinct list, are then what the stream holds), each held to the oracle's bytes; returns (cases, controls, batch of every sample)"""
    os.environ['KV_SKM_DL'] = '1'
    batches, sketches = {}, {}
    for spec in scan.ctrls + scan.cases:
        # the family through the super-k-mer count by name (sketches of up to four tables leave their abundance list there, the others
        # land on the atomic kernel); the small samples of the strangers as the library likes
        pin_count(None if spec.reads.startswith('stranger') else 'skm')
        if spec.reads not in batches:
            batches[spec.reads] = hk.ReadBatch.from_packed(tc.words(spec.reads), tc.READ_LEN)
        dev = tc.make(hk, spec, k, ok)
        if hint and spec in scan.cases:
            dev.expect_scan()
        n = len(tc.words(spec.reads)) * (tc.READ_LEN - k + 1)
        assert dev.consume_batch(batches[spec.reads]) == n
        tc.assert_same_state(dev, tc.snapshot(tc.oracle_sketch(ok, spec, k)), str(spec))
        sketches[spec] = dev
    os.environ.pop('KV_COUNT_PATH', None)
    return [sketches[s] for s in scan.cases], [sketches[s] for s in scan.ctrls], batches


def run_scan(hk, prof, cases, ctrls, batch, scan, path):
    """one scan with the kernel asked for by name ('list' and 'walk' both ask for the super-k-mer scan: which of the two answers depends
    on what the count left); returns the hits and the launches of each scan kernel"""
    os.environ['KV_NOVEL_PATH'] = {'list': 'skm', 'walk': 'skm', 'tiles': 'tiles', 'tiles2bit': 'per-kmer'}[path]
    prof.kv_prof_reset()
    try:
        r, o, a, disc = hk.novel_scan(cases, ctrls, batch, scan.case_min, scan.ctrl_max)
    finally:
        os.environ.pop('KV_NOVEL_PATH', None)
    assert len(disc) == 0
    return (np.asarray(r, dtype=np.uint32), np.asarray(o, dtype=np.uint32), np.asarray(a, dtype=np.uint8)), {name: launches(name) for name in SCAN_KERNELS}


def every_scan_kernel(hk, prof, cases, ctrls, batch, scan, want, with_list):
    """the scan from the distinct list (where the count left one), the walk over the buckets and both tile kernels against `want`"""
    only = lambda name: {n: (1 if n == name else 0) for n in SCAN_KERNELS}
    got, ran = run_scan(hk, prof, cases, ctrls, batch, scan, 'list')
    # (no list: the count went through the atomic kernel, or another batch was counted on the stream since; the walk answers)
    assert ran == only('k_skm_novel_list' if with_list else 'k_skm_novel'), ran
    assert tc.hits_difference(got, want) is None, ('list scan' if with_list else 'walk', tc.hits_difference(got, want))
    if with_list:
        # one scan per list: the next one by the same name finds the list gone, cuts the reads again and walks the buckets
        got, ran = run_scan(hk, prof, cases, ctrls, batch, scan, 'walk')
        assert ran == only('k_skm_novel'), ran
        assert tc.hits_difference(got, want) is None, ('walk', tc.hits_difference(got, want))
    for path, kernel in (('tiles', 'k_novel_mark'), ('tiles2bit', 'k_novel_mark_2bit')):
        got, ran = run_scan(hk, prof, cases, ctrls, batch, scan, path)
        assert ran == only(kernel), ran
        assert tc.hits_difference(got, want) is None, (kernel, tc.hits_difference(got, want))


@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('case_tables', [1, 3, 4, 9, 16])
def test_mixed_sketches_every_scan_kernel(hk, ok, prof, case_tables, k):
    """a byte-counter case of 1 to 16 tables against 16 crowded byte tables, 3 nibble tables and 2 bit tables in one scan; at ctrl_max 0
    the bit table rejects too.  A case of more than four tables is counted by the atomic kernel and leaves no distinct list."""
    scan = tc.mixed_scan(case_tables, 1)
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    assert launches('k_skm_count') == (3 if case_tables <= tc.BIN_MAX_T else 2)         # (the nibble and the bit control, and the case)
    with_list = case_tables <= tc.BIN_MAX_T
    for ctrl_max in (1, 0):
        scan = tc.mixed_scan(case_tables, ctrl_max)
        if ctrl_max == 0 and with_list:
            # a distinct list serves one scan: the case is counted again (the hint stays with the sketch) for the second
            pin_count('skm')
            cases[0].clear()
            cases[0].consume_batch(batches['proband'])
            os.environ.pop('KV_COUNT_PATH')
        every_scan_kernel(hk, prof, cases, ctrls, batches['proband'], scan, tc.oracle_hits(ok, scan, k), with_list=with_list)


@pytest.mark.parametrize('k', tc.KS)
def test_nibble_case_against_byte_controls(hk, ok, prof, k):
    scan = tc.NIBBLE_CASE_SCAN
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    every_scan_kernel(hk, prof, cases, ctrls, batches['proband'], scan, tc.oracle_hits(ok, scan, k), with_list=True)


@pytest.mark.parametrize('k', tc.KS)
def test_sixteen_crowded_tables_on_case_and_control(hk, ok, prof, k):
    """the abundances of a hit are the minimum over all 16 tables of either sample (tests/test_tables_reference.py: over the first four
    they are something else)"""
    scan = tc.SIXTEEN_TABLES
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    every_scan_kernel(hk, prof, cases, ctrls, batches['proband'], scan, tc.oracle_hits(ok, scan, k), with_list=False)


@pytest.mark.parametrize('k', tc.KS)
def test_one_case_and_fifteen_controls(hk, ok, prof, k):
    """16 samples, the limit: the mother is sample 9 and the father sample 12, behind eight strangers who reject nothing"""
    scan = tc.SIXTEEN
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    assert len(cases) + len(ctrls) == tc.MAX_SAMPLES
    every_scan_kernel(hk, prof, cases, ctrls, batches['proband'], scan, tc.oracle_hits(ok, scan, k), with_list=True)


@pytest.mark.parametrize('k', tc.KS)
def test_two_cases_and_fourteen_controls(hk, ok, prof, k):
    """the parents at the last two places; the reads of both cases are scanned, the second case's (counted last) from its distinct list"""
    scan = tc.TWO_CASES
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    every_scan_kernel(hk, prof, cases, ctrls, batches['sibling'], scan, tc.oracle_hits(ok, scan, k, scanned='sibling'), with_list=True)
    every_scan_kernel(hk, prof, cases, ctrls, batches['proband'], scan, tc.oracle_hits(ok, scan, k), with_list=False)


def test_seventeen_samples_are_refused_and_sixteen_still_scan(hk, ok, prof):
    from kevlar_amd import _lib
    k, scan = 31, tc.SEVENTEEN
    cases, ctrls, batches = counted_on_device(hk, ok, scan, k)
    assert len(cases) + len(ctrls) == tc.MAX_SAMPLES + 1
    for path in ('skm', 'tiles', 'per-kmer', None):
        if path:
            os.environ['KV_NOVEL_PATH'] = path
        with pytest.raises(_lib.KvArgError, match='at most 16 samples'):
            hk.novel_scan(cases, ctrls, batches['proband'], scan.case_min, scan.ctrl_max)
        os.environ.pop('KV_NOVEL_PATH', None)
    want = tc.oracle_hits(ok, tc.SIXTEEN, k)
    for path in ('walk', 'tiles', 'tiles2bit'):
        got, _ = run_scan(hk, prof, cases, ctrls[:15], batches['proband'], tc.SIXTEEN, path)
        assert tc.hits_difference(got, want) is None, (path, tc.hits_difference(got, want))


# ---- the other consumers of the table count -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('ntables', [1, 5, 16])
def test_point_queries(hk, ok, ntables, k):
    """get, get_kmer_counts and add (k_get_hashes, k_add_hashes): a k-mer is new when ANY of the T bins was zero"""
    spec = tc.C(1e5, ntables)
    ref = tc.make(ok, spec, k, ok)
    tc.oracle_count(ok, ref, 'proband')
    dev = tc.make(hk, spec, k, ok)
    dev.consume_batch(hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN))
    seqs = tc.reads('proband')[:3] + tc.reads('stranger0')[:3]
    for seq in seqs:
        assert dev.get_kmer_counts(seq) == ref.get_kmer_counts(seq)
    assert max(ref.get_kmer_counts(seqs[0])) > 1 and (ntables == 1 or 0 in ref.get_kmer_counts(seqs[3]))
    kmers = [s[i:i + k] for s in tc.reads('stranger1')[:4] for i in range(0, tc.READ_LEN - k + 1, 5)]
    kmers += kmers[:7] + ['A' * k] * 3
    assert [dev.add(km) for km in kmers] == [ref.add(km) for km in kmers]
    assert [dev.get(km) for km in kmers] == [ref.get(km) for km in kmers]
    assert dev.get('A' * k) == ref.get('A' * k) >= 3
    tc.assert_same_state(dev, tc.snapshot(ref))


@pytest.mark.parametrize('force', [None, 'binned'])
@pytest.mark.parametrize('ntables', [2, 5])
def test_consume_hashes_equals_banded_consume(hk, ok, prof, ntables, force):
    """band b of a banded count == the hashes routed to destination b, then kv_consume_hashes: through the atomic kernel, and by name
    through the partition's list front end (which five tables do not take)"""
    import torch
    k, nb = 31, 3
    spec = tc.C(3e5, ntables)
    batch = hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN)
    nk = batch.num_kmers(k)
    send = torch.zeros((nk, 1), dtype=torch.int64, device='cuda')
    counts = hk.route_hashes(batch, hk.Counttable, k, nb, 0, False, send.data_ptr(), nk)
    starts = np.concatenate(([0], np.cumsum(counts)))
    for b in range(nb):
        ref = tc.make(ok, spec, k, ok)
        n_ref = tc.oracle_count(ok, ref, 'proband', nb, b)
        pin_count(None)
        banded = tc.make(hk, spec, k, ok)
        assert banded.consume_batch(batch, nb, b) == n_ref == counts[b]
        pin_count(force)
        prof.kv_prof_reset()
        routed = tc.make(hk, spec, k, ok)
        assert routed.consume_hashes(send[int(starts[b]):].data_ptr(), counts[b]) == counts[b]
        by_list = force == 'binned' and ntables <= tc.BIN_MAX_T
        assert (launches('k_bin_list'), launches('k_bin_apply'), launches('k_add_hashes')) == ((1, 1, 0) if by_list else (0, 0, 1))
        for dev in (banded, routed):
            tc.assert_same_state(dev, tc.snapshot(ref), 'band {}'.format(b))


@pytest.mark.parametrize('ntables', [1, 16])
def test_exact_unique_over_three_batches(hk, ok, ntables):
    """track_exact_unique: a first-toucher array per table (FirstTouchParams::first[KV_MAX_TABLES])"""
    k, spec = 31, tc.C(1e5, ntables)
    dev, ref = tc.make(hk, spec, k, ok), tc.make(ok, spec, k, ok)
    dev.track_exact_unique(True)
    try:
        proband, mother = tc.reads('proband'), tc.reads('mother')
        for part in (proband[:3000], proband[2000:5000], mother[:3000]):
            bases, offs = ok.concat_reads(part)
            assert dev.consume_batch(hk.ReadBatch(part)) == ok.consume_reads(ref, bases, offs, len(part))
            assert dev.n_unique_kmers() == ref.n_unique_kmers()
        tc.assert_same_state(dev, tc.snapshot(ref))
    finally:
        dev.track_exact_unique(False)


def test_abundance_distribution_with_sixteen_tables(hk, ok):
    import ctypes
    k, spec = 31, tc.C(1e5, 16)
    ref = tc.oracle_sketch(ok, spec, k)
    dev = tc.make(hk, spec, k, ok)
    dev.consume_batch(hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN))
    dev_track, ref_track = hk.Nodetable(k, 1, 1, primes=dev.hashsizes()), ok.Nodetable(k, 1, 1, primes=ref.hashsizes())
    assert dev_track.n_tables() == 16
    for name in ('mother-head', 'proband'):
        got = dev.abundance_distribution(hk.ReadBatch(tc.reads(name)), dev_track)
        hist = (ctypes.c_uint64 * 65536)()
        for seq in tc.reads(name):
            b = seq.encode()
            ok.lib.kvo_abundance_distribution(ref._h, ref_track._h, b, len(b), hist)
        assert got == list(hist) and sum(got) > 1000
        tc.assert_same_state(dev_track, tc.snapshot(ref_track), 'tracking table after ' + name)


@pytest.mark.parametrize('kind,ntables', [('Counttable', 1), ('Nodetable', 7), ('SmallCounttable', 16)])
def test_save_and_load_both_ways(hk, ok, tmp_path, kind, ntables):
    k, spec = 31, tc.Spec(kind, 1e5, ntables, 'proband')
    ref = tc.oracle_sketch(ok, spec, k)
    path = str(tmp_path / 'oracle.sketch')
    ref.save(path)
    dev = getattr(hk, kind).load(path)
    assert dev.hashsizes() == ref.hashsizes() and dev.ksize() == k
    tc.assert_same_state(dev, tc.snapshot(ref), 'loaded from the oracle\'s file')
    for seq in tc.reads('proband')[:2] + tc.reads('stranger0')[:2]:
        assert dev.get_kmer_counts(seq) == ref.get_kmer_counts(seq)
    counted = tc.make(hk, spec, k, ok)
    counted.consume_batch(hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN))
    path = str(tmp_path / 'device.sketch')
    counted.save(path)
    back = getattr(ok, kind).load(path)
    assert back.hashsizes() == ref.hashsizes() and back.ksize() == k
    assert tc.snapshot(back) == tc.snapshot(ref)


def test_a_file_of_seventeen_tables_is_refused(hk, ok, tmp_path):
    k = 31
    wide = ok.Counttable(k, 1e4, tc.MAX_TABLES + 1)
    wide.consume(tc.reads('proband')[0])
    path = str(tmp_path / 'seventeen.ct')
    wide.save(path)
    assert ok.Counttable.load(path).n_tables() == 17
    with pytest.raises(OSError, match='unsupported sketch header'):
        hk.Counttable.load(path)
    spec = tc.C(1e5, 16)
    dev = tc.make(hk, spec, k, ok)
    dev.consume_batch(hk.ReadBatch.from_packed(tc.words('proband'), tc.READ_LEN))
    tc.assert_same_state(dev, tc.snapshot(tc.oracle_sketch(ok, spec, k)))
