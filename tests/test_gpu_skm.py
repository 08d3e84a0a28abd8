"""The super-k-mer front end (kv_skm.hip and its kv_skm_*_device.h kernels): reads cut into minimizer-bucketed super-k-mers, every distinct k-mer
of a bucket counted once with its multiplicity and evaluated once by the novel scan.  It must give the same
table bytes, occupancy, k-mer totals and hits as the scalar oracle (which adds and evaluates k-mer by k-mer, as
khmer / kevlar/novel.py:123-169 do) -- for every k it accepts, every storage, with bands and masks, on ragged,
long and non-ACGT reads, on skewed input, and when its segments or LDS tables overflow into the loose list."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ('KV_COUNT_PATH', 'KV_NOVEL_PATH', 'KV_SKM_BUCKET_KMERS', 'KV_SKM_CAP_PCT', 'KV_SKM_LOOSE_CAP', 'KV_SKM_NO_REUSE', 'KV_SKM_FORCE_LOOSE', 'KV_SKM_DL', 'KV_SKM_ANY_K',
         'KV_BIN_2BIT', 'KV_NOVEL_2BIT', 'KV_NOVEL_BITS')


def instances():
    """the super-k-mer kernel instances the last call launched, in launch order (kv_skm_last_instances)"""
    from kevlar_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    assert _lib.load().kv_skm_last_instances(buf, len(buf)) == 0
    return re.split(r',(?![^<]*>)', buf.value.decode())          # (a name's own commas stand between its angle brackets)


def launches(name):
    from kevlar_amd import _lib
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.load().kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return n.value


@pytest.fixture
def skm():
    """Force the super-k-mer path (it is the default only from 4 M k-mers up) and record which kernels ran."""
    from kevlar_amd import _lib
    lib = _lib.load()
    lib.kv_prof_reset()
    lib.kv_prof_enable(1)
    os.environ['KV_COUNT_PATH'] = 'skm'
    os.environ['KV_NOVEL_PATH'] = 'skm'
    yield lib
    lib.kv_prof_enable(0)
    for name in KNOBS:
        os.environ.pop(name, None)


def stage_a():
    """launches of the partitioned count's per-k-mer front end: the tile kernel, or (reads of one length) the one that hashes from the 2-bit form"""
    return launches('k_bin_hash_direct') + launches('k_bin_hash_2bit')


def trio_reads(genome_len, n, seed, read_len=100):
    from kevlar_amd import synth
    trio = synth.make_trio(genome_len, seed, inherited_per_mb=400, denovo_per_mb=400)
    out = {}
    for i, name in enumerate(('proband', 'mother', 'father')):
        words = synth.sample_reads_packed(trio[name], n, read_len, 0.005, seed + 1 + i)
        out[name] = synth.unpack_reads(words, read_len)
    return out


def count_both(hk, ok, kind, k, tablesize, reads):
    dev, ref = getattr(hk, kind)(k, tablesize, 4), getattr(ok, kind)(k, tablesize, 4)
    n_dev = dev.consume_batch(hk.ReadBatch(reads))
    bases, offs = ok.concat_reads(reads)
    n_ref = ok.consume_reads(ref, bases, offs, len(reads))
    return dev, ref, n_dev, n_ref


def assert_same_tables(dev, ref):
    for t in range(len(ref.hashsizes())):
        assert dev.table_bytes(t) == ref.table_bytes(t), 'table {} differs from the oracle'.format(t)
    assert dev.n_occupied() == ref.n_occupied()


@pytest.mark.parametrize('kind,k,tablesize', [('Counttable', 31, 1.5e6), ('SmallCounttable', 31, 1.2e6), ('Nodetable', 31, 4e6),
                                              ('Counttable', 21, 1.5e6), ('Counttable', 16, 8e5), ('Counttable', 32, 1.5e6),
                                              ('Counttable', 33, 1.5e6), ('Counttable', 51, 1.5e6), ('Counttable', 64, 1.5e6)])
def test_skm_count_matches_oracle(hk, ok, skm, kind, k, tablesize):
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'      # ~600 fine buckets on this input
    reads = trio_reads(150000, 18000, 5)['proband']
    dev, ref, n_dev, n_ref = count_both(hk, ok, kind, k, tablesize, reads)
    assert launches('k_skm_count') == 1 and launches('k_bin_apply_w') == 1 and launches('k_consume') == 0
    assert n_dev == n_ref == 18000 * (100 - k + 1)
    assert_same_tables(dev, ref)
    assert abs(dev.n_unique_kmers() - ref.n_unique_kmers()) < 0.03 * ref.n_unique_kmers()
    # a second batch lands on top of the first
    more = trio_reads(150000, 9000, 8)['mother']
    dev.consume_batch(hk.ReadBatch(more))
    bases, offs = ok.concat_reads(more)
    ok.consume_reads(ref, bases, offs, len(more))
    assert_same_tables(dev, ref)


def test_scratch_trim_between_count_and_scan(hk, ok, skm):
    """kv_scratch_trim gives the per-stream working buffers back: a scan that would have reused the case sample's buckets (and its distinct
    list) cuts them again, a later count allocates again -- same hits, same tables"""
    reads = trio_reads(100000, 30000, 44)
    for hint in (False, True):
        names = ('proband', 'mother', 'father')
        dev = {n: hk.Counttable(31, 1.5e6, 4) for n in names}
        ref = {n: ok.Counttable(31, 1.5e6, 4) for n in names}
        if hint:
            dev['proband'].expect_scan()
        batches = {n: hk.ReadBatch(reads[n]) for n in names}
        for n in ('mother', 'father', 'proband'):
            dev[n].consume_batch(batches[n])
            if n == 'father':
                hk.scratch_trim()
            bases, offs = ok.concat_reads(reads[n])
            ok.consume_reads(ref[n], bases, offs, len(reads[n]))
            assert_same_tables(dev[n], ref[n])
        hk.scratch_trim()
        r, o, a, _ = hk.novel_scan([dev['proband']], [dev['mother'], dev['father']], batches['proband'], 6, 1)
        bases, offs = ok.concat_reads(reads['proband'])
        hits, _ = ok.novel_scan([ref['proband']], [ref['mother'], ref['father']], bases, offs, len(reads['proband']), 31, 6, 1, 0, 0, 0, 0)
        assert len(hits) > 50
        assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == hits


@pytest.mark.parametrize('read_len,k', [(36, 31), (75, 25), (150, 31), (151, 51), (251, 31), (600, 31)])
def test_skm_equal_length_reads_of_other_lengths(hk, ok, skm, read_len, k):
    """batches of equal-length reads handed over as packed words (what the device ingest and the generators produce): the layout is
    arithmetic, and skm_launch_emit chooses S1 by k and the read length -- the lane-per-read cut (k_skm_emit_lane: k = 31 or 51, up to
    224 bases) for (36, 31), (150, 31) and (151, 51); the wave-per-group kernel (k_skm_emit_wave: one packed word and one chunk of k-mer
    starts per lane) for (75, 25) and (251, 31); the tile kernel (k_skm_emit) for (600, 31), where a wave would hold a single read.  The
    group size, the padding of a read's last word and the chunks or blocks per read all follow the read length.
    (tests/instances_common.py holds every instance of these families at the planners' edges.)"""
    s1_family = {(36, 31): 'k_skm_emit_lane', (75, 25): 'k_skm_emit_wave', (150, 31): 'k_skm_emit_lane', (151, 51): 'k_skm_emit_lane',
                 (251, 31): 'k_skm_emit_wave', (600, 31): 'k_skm_emit'}[(read_len, k)]
    from kevlar_amd import synth
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    os.environ['KV_SKM_DL'] = '1'
    n = max(2000, 1500000 // read_len)
    trio = synth.make_trio(60000, 61, inherited_per_mb=400, denovo_per_mb=400)
    names = ('proband', 'mother', 'father')
    words = {s: synth.sample_reads_packed(trio[s], n, read_len, 0.005, 62 + i) for i, s in enumerate(names)}
    reads = {s: synth.unpack_reads(words[s], read_len) for s in names}
    for hint in (False, True):
        dev = {s: hk.Counttable(k, 2e6, 4) for s in names}
        ref = {s: ok.Counttable(k, 2e6, 4) for s in names}
        if hint:
            dev['proband'].expect_scan()
        batches = {s: hk.ReadBatch.from_packed(words[s], read_len) for s in names}
        for s in ('mother', 'father', 'proband'):
            assert dev[s].consume_batch(batches[s]) == n * (read_len - k + 1)
            assert instances()[0].split('<')[0] == s1_family
            bases, offs = ok.concat_reads(reads[s])
            ok.consume_reads(ref[s], bases, offs, n)
            assert_same_tables(dev[s], ref[s])
        r, o, a, _ = hk.novel_scan([dev['proband']], [dev['mother'], dev['father']], batches['proband'], 6, 1)
        bases, offs = ok.concat_reads(reads['proband'])
        hits, _ = ok.novel_scan([ref['proband']], [ref['mother'], ref['father']], bases, offs, n, k, 6, 1, 0, 0, 0, 0)
        assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == hits and len(hits) > 10
    assert launches('k_skm_novel_list') == 1 and launches('k_skm_novel') == 1


def test_skm_single_bucket_and_default_geometry(hk, ok, skm):
    """one coarse x one fine bucket (everything in one LDS table, most of it overflowing into the loose list), and
    the geometry the library picks by itself"""
    reads = trio_reads(60000, 2500, 3)['proband']
    for target in ('100000000', None):
        if target:
            os.environ['KV_SKM_BUCKET_KMERS'] = target
        else:
            os.environ.pop('KV_SKM_BUCKET_KMERS', None)
        dev, ref, n_dev, n_ref = count_both(hk, ok, 'Counttable', 31, 9e5, reads)
        assert n_dev == n_ref
        assert_same_tables(dev, ref)
    assert launches('k_skm_count') == 2


def test_skm_ragged_short_long_and_non_acgt_reads(hk, ok, skm):
    rng = np.random.default_rng(12)
    letters = np.array(list('ACGT'))

    def rnd(n):
        return ''.join(letters[rng.integers(0, 4, size=n)])
    chrom = rnd(60011)
    reads = [rnd(int(rng.integers(10, 260))) for _ in range(3000)]
    reads += ['', 'ACG', rnd(30), rnd(31), rnd(32), chrom, rnd(7680), rnd(7681 + 30), rnd(8200), 'A' * 150, 'ACGT' * 40]
    reads += [chrom[100:400], chrom[100:400], chrom[30000:30300]]
    bad = list(rnd(140)); bad[70] = 'N'
    low = rnd(50) + 'acgtn' + rnd(50)
    reads += [''.join(bad), low]
    os.environ['KV_SKM_BUCKET_KMERS'] = '1024'
    for kind, k in (('Counttable', 31), ('Counttable', 45), ('SmallCounttable', 19)):
        dev, ref, n_dev, n_ref = count_both(hk, ok, kind, k, 7e5, reads)
        assert n_dev == n_ref
        assert_same_tables(dev, ref)
    assert launches('k_skm_count') == 3 and launches('k_consume') == 0


def test_skm_skew_saturation_and_overflow_paths(hk, ok, skm):
    """thousands of copies of a few k-mers (weights above 128 are split, counters saturate at 255 / 15), segments
    sized at a fraction of what they need (records travel through the loose list), then a loose list that is too
    small: the library must notice, leave the tables alone and fall back"""
    base = trio_reads(100000, 9000, 21)['proband']
    reads = base + ['A' * 100] * 700 + ['ACGT' * 25] * 300 + [base[0]] * 400
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    for kind in ('Counttable', 'SmallCounttable'):
        dev, ref, n_dev, n_ref = count_both(hk, ok, kind, 31, 1e6, reads)
        assert n_dev == n_ref
        assert_same_tables(dev, ref)
        assert dev.get('A' * 31) == ref.get('A' * 31) == (255 if kind == 'Counttable' else 15)
    os.environ['KV_SKM_CAP_PCT'] = '30'
    dev, ref, n_dev, n_ref = count_both(hk, ok, 'Counttable', 31, 1e6, reads)
    assert n_dev == n_ref
    assert_same_tables(dev, ref)
    assert launches('k_skm_count') == 3 and stage_a() == 0
    os.environ['KV_SKM_LOOSE_CAP'] = '64'
    dev, ref, n_dev, n_ref = count_both(hk, ok, 'Counttable', 31, 1e6, reads)
    assert n_dev == n_ref
    assert_same_tables(dev, ref)
    assert stage_a() + launches('k_consume') >= 1      # the fallback ran


def test_skm_band_and_mask(hk, ok, skm):
    reads = trio_reads(120000, 12000, 31)['proband']
    dmask, rmask = hk.Nodetable(31, 1e6, 4), ok.Nodetable(31, 1e6, 4)
    dmask.consume_batch(hk.ReadBatch(reads[:4000]))
    bases, offs = ok.concat_reads(reads[:4000])
    ok.consume_reads(rmask, bases, offs, 4000)
    bases, offs = ok.concat_reads(reads)
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    for nbands, band, mask_args in [(4, 3, None), (4, 0, None), (0, 0, (0, False)), (2, 0, (1, True))]:
        dev, ref = hk.Counttable(31, 9e5, 4), ok.Counttable(31, 9e5, 4)
        if mask_args is None:
            n_dev = dev.consume_batch(hk.ReadBatch(reads), nbands, band)
            n_ref = ok.consume_reads(ref, bases, offs, len(reads), nbands, band)
        else:
            n_dev = dev.consume_batch(hk.ReadBatch(reads), nbands, band, dmask, mask_args[0], mask_args[1])
            n_ref = ok.consume_reads(ref, bases, offs, len(reads), nbands, band, rmask, mask_args[0], mask_args[1])
        assert n_dev == n_ref and n_dev > 0
        assert_same_tables(dev, ref)
    assert launches('k_skm_count') >= 4


def scan_both(hk, ok, reads, k, mem, case_min=6, ctrl_max=1, nctrl=2, order=('mother', 'father', 'proband'), hint=False, kind='Counttable', **kw):
    names = ('proband', 'mother', 'father')[:1 + nctrl]
    dev = {n: getattr(hk, kind)(k, mem / 4, 4) for n in names}
    if hint:
        os.environ['KV_SKM_DL'] = '1'                           # (also for the first batch this process buckets)
        dev['proband'].expect_scan()                            # the count keeps the batch's distinct k-mers with their hashes
    ref = {n: getattr(ok, kind)(k, mem / 4, 4) for n in names}
    batches = {n: hk.ReadBatch(reads[n]) for n in names}
    for n in [x for x in order if x in names]:                  # the case sample last: the scan can reuse its buckets
        dev[n].consume_batch(batches[n])
    for n in names:
        bases, offs = ok.concat_reads(reads[n])
        ok.consume_reads(ref[n], bases, offs, len(reads[n]))
        assert_same_tables(dev[n], ref[n])
    r, o, a, _ = hk.novel_scan([dev['proband']], [dev[n] for n in names[1:]], batches['proband'], case_min, ctrl_max, **kw)
    bases, offs = ok.concat_reads(reads['proband'])
    hits, _ = ok.novel_scan([ref['proband']], [ref[n] for n in names[1:]], bases, offs, len(reads['proband']), k,
                            case_min, ctrl_max, 0, kw.get('band_mode', 0), kw.get('nbands', 0), kw.get('band', 0))
    got = [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))]
    return got, hits


@pytest.mark.parametrize('k', [31, 25, 51])
def test_skm_novel_scan_matches_oracle(hk, ok, skm, k):
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    reads = trio_reads(100000, 30000, 41)           # 30x: inherited k-mers well above case-min
    got, hits = scan_both(hk, ok, reads, k, 6e6)
    assert len(hits) > 50
    assert got == hits
    assert launches('k_skm_novel') == 1 and launches('k_novel_mark') == 0
    # the scan reused the buckets the case count had built -- unless that count wrote 16-byte records without read positions (k = 31,
    # reads of one length, and nobody said a scan would follow: Counttable.expect_scan), which the scan cannot answer from: it cuts again
    assert launches('k_skm_emit') == (4 if k == 31 else 3)


def test_list_scan_takes_every_entry_of_buckets_that_nearly_fill_the_table(hk, ok, skm):
    """Long reads with many errors at 30x and no control: buckets whose distinct k-mers fill most of the count's LDS table, every one of
    them with four occurrences or more interesting.  The scan from the distinct list takes SKM_LIST_MAX entries of a bucket -- as many as
    the count's table has slots: a static assertion in k_skm_count since round 6, when a 4608-slot table let a bucket's list outgrow the
    4096 the scan took (scratch/fuzz_list.py seed 702, trial 149, lost 8 % of its hits; a table and a list limit that agree cannot be told
    apart at run time, so this test only holds the dense regime against the oracle)."""
    from kevlar_amd import synth
    os.environ['KV_SKM_BUCKET_KMERS'] = '8192'
    os.environ['KV_SKM_DL'] = '1'
    k, L, n = 31, 250, 48000
    trio = synth.make_trio(400000, 977, inherited_per_mb=400, denovo_per_mb=400)
    words = synth.sample_reads_packed(trio['proband'], n, L, 0.012, 4242)
    reads = synth.unpack_reads(words, L)
    dev, ref = hk.Counttable(k, 2e6, 4), ok.Counttable(k, 2e6, 4)
    dev.expect_scan()
    batch = hk.ReadBatch.from_packed(words, L)
    bases, offs = ok.concat_reads(reads)
    assert dev.consume_batch(batch) == ok.consume_reads(ref, bases, offs, n)
    assert launches('k_skm_count') == 1
    assert_same_tables(dev, ref)
    r, o, a, _ = hk.novel_scan([dev], [], batch, 4, 1)
    assert launches('k_skm_novel_list') == 1, 'the scan must go by the distinct list'
    wr, wo, wa = ok.novel_scan_mt([ref], [], bases, offs, n, k, 4, 1, 4)
    assert len(wr) > 3_000_000
    assert len(r) == len(wr) and np.array_equal(r, wr) and np.array_equal(o, wo.astype(np.uint32)) and np.array_equal(a, wa)


@pytest.mark.parametrize('path', ['skm', 'tiles'])
def test_lazy_hits_are_the_hits_and_survive_the_next_count(hk, ok, skm, path):
    """hk.novel_scan(lazy=True) (kv_hits_lazy): the call returns when its kernels are done, the hit arrays follow on a copy stream of
    their own.  From then on the sketches may be cleared and counted into again -- bench.py's next step does exactly that -- and a
    second scan on the stream reuses the device buffers the first one's hits are leaving: the arrays that arrive must be the first
    scan's, hit for hit the oracle's.  With an abundance screen the call stays eager (its bookkeeping reads the hits on the host)."""
    reads = trio_reads(50000, 20000, 61)
    names = ('proband', 'mother', 'father')
    dev = {n: hk.Counttable(31, 1.5e6, 4) for n in names}
    ref = {n: ok.Counttable(31, 1.5e6, 4) for n in names}
    for n in names:
        dev[n].consume_batch(hk.ReadBatch(reads[n]))
        bases, offs = ok.concat_reads(reads[n])
        ok.consume_reads(ref[n], bases, offs, len(reads[n]))
    os.environ['KV_NOVEL_PATH'] = path
    batch = hk.ReadBatch(reads['proband'])
    bases, offs = ok.concat_reads(reads['proband'])
    want, _ = ok.novel_scan([ref['proband']], [ref['mother'], ref['father']], bases, offs, len(reads['proband']), 31, 6, 1)
    assert len(want) > 50
    cases, ctrls = [dev['proband']], [dev['mother'], dev['father']]
    first = hk.novel_scan(cases, ctrls, batch, 6, 1, lazy=True)
    assert isinstance(first, hk.LazyHits) and len(first) == len(want)
    # the sketches change under the copy, and another scan (different thresholds: other hits) writes the same device buffers
    second = hk.novel_scan(cases, ctrls, batch, 2, 3, lazy=True)
    assert len(second) > len(first)
    dev['mother'].clear()
    dev['mother'].consume_batch(hk.ReadBatch(reads['proband']))
    r, o, a, disc = first.arrays()
    assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == want and len(disc) == 0
    r2, o2, a2, _ = second.arrays()
    assert len(r2) == len(second) and (a2[:, 0] >= 2).all() and (a2[:, 1:] <= 3).all()
    del first, second
    third = hk.novel_scan(cases, [dev['father']], batch, 6, 1, lazy=True)           # a handle nobody reads: destroyed while its copy may be in flight
    del third
    screened = hk.novel_scan(cases, [dev['father']], batch, 6, 1, screen=2, lazy=True)
    eager = hk.novel_scan(cases, [dev['father']], batch, 6, 1, screen=2)
    for x, y in zip(screened.arrays(), eager):
        assert np.array_equal(x, y)


def test_skm_novel_scan_rebuilds_when_the_case_was_counted_first_and_honours_skips(hk, ok, skm):
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    reads = trio_reads(80000, 24000, 43)
    bad = list(reads['proband'][5]); bad[40] = 'N'
    reads['proband'][5] = ''.join(bad)              # flagged: the scan skips it, the count keeps it
    got, hits = scan_both(hk, ok, reads, 31, 5e6, order=('proband', 'mother', 'father'))
    assert got == hits and len(hits) > 20
    assert launches('k_skm_emit') == 4              # case buckets were overwritten by the controls: cut again
    # first_read: reads in front of it are not scanned (--skip-until)
    names = ('proband', 'mother', 'father')
    dev = {n: hk.Counttable(31, 5e6 / 4, 4) for n in names}
    batch = hk.ReadBatch(reads['proband'])
    for n in ('mother', 'father'):
        dev[n].consume_batch(hk.ReadBatch(reads[n]))
    dev['proband'].consume_batch(batch)
    r, o, a, _ = hk.novel_scan([dev['proband']], [dev['mother'], dev['father']], batch, 6, 1, first_read=9000)
    want = [h for h in hits if h[0] >= 9000]
    assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == want


def test_skm_novel_scan_bands_multi_control_and_overflow(hk, ok, skm):
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    reads = trio_reads(80000, 24000, 47)
    union = []
    for band in range(3):
        got, hits = scan_both(hk, ok, reads, 31, 5e6, band_mode=1, nbands=3, band=band)
        assert got == hits
        union += got
    whole, hits = scan_both(hk, ok, reads, 31, 5e6)
    assert sorted(union) == whole == hits
    got, hits = scan_both(hk, ok, reads, 31, 5e6, band_mode=2, nbands=4, band=2)       # the reference's literal rule
    assert got == hits
    os.environ['KV_SKM_CAP_PCT'] = '30'             # loose records in the scan as well
    got, hits = scan_both(hk, ok, reads, 31, 5e6, case_min=5, ctrl_max=2)
    assert got == hits and len(hits) > 20
    assert launches('k_novel_mark') == 0


@pytest.mark.parametrize('k', [31, 25, 51])
def test_skm_scan_from_the_distinct_list_matches_oracle(hk, ok, skm, k):
    """kv_sketch_scan_hint: the case sample's count leaves key + hash of every distinct k-mer, the scan evaluates from that list
    (k_skm_novel_list) and walks only the buckets that hold an interesting k-mer"""
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    reads = trio_reads(100000, 30000, 41)
    got, hits = scan_both(hk, ok, reads, k, 6e6, hint=True)
    assert len(hits) > 50 and got == hits
    assert launches('k_skm_novel_list') == 1 and launches('k_skm_novel') == 0 and launches('k_novel_mark') == 0
    assert launches('k_skm_emit') == 3


def test_exchange_packing_on_the_stream_drops_what_a_scan_could_have_reused(hk, ok, skm):
    """kv_mex_pack writes its segment offsets where the stream's bucketed batch lies.  After it neither the case sample's buckets nor its
    distinct list may be reused: the scan that follows cuts the reads again, walks the buckets, and finds the oracle's hits."""
    import torch
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    k = 31
    reads = trio_reads(100000, 20000, 41)
    names = ('proband', 'mother', 'father')
    os.environ['KV_SKM_DL'] = '1'
    dev = {n: hk.Counttable(k, 1.5e6, 4) for n in names}
    ref = {n: ok.Counttable(k, 1.5e6, 4) for n in names}
    dev['proband'].expect_scan()
    batches = {n: hk.ReadBatch(reads[n]) for n in names}
    for n in ('mother', 'father', 'proband'):                   # the case sample last: its buckets and its list are the stream's state
        dev[n].consume_batch(batches[n])
        bases, offs = ok.concat_reads(reads[n])
        ok.consume_reads(ref[n], bases, offs, len(reads[n]))
    assert launches('k_skm_emit') == 3
    plan = hk.mex_plan(hk.Counttable, k, 1000, 100, 2)          # a shard nobody cut: every exchange segment empty
    seg = torch.zeros(int(plan.seg_words), dtype=torch.int64, device='cuda')
    cnt = torch.zeros(int(plan.cnt_entries), dtype=torch.int32, device='cuda')
    out = torch.zeros(64, dtype=torch.int64, device='cuda')
    assert hk.mex_pack(plan, seg.data_ptr(), cnt.data_ptr(), out.data_ptr()) == [0, 0]
    r, o, a, _ = hk.novel_scan([dev['proband']], [dev['mother'], dev['father']], batches['proband'], 6, 1)
    assert launches('k_skm_emit') == 4 and launches('k_skm_novel') == 1 and launches('k_skm_novel_list') == 0
    bases, offs = ok.concat_reads(reads['proband'])
    hits, _ = ok.novel_scan([ref['proband']], [ref['mother'], ref['father']], bases, offs, len(reads['proband']), k, 6, 1, 0, 0, 0, 0)
    assert len(hits) > 50
    assert [(int(r[i]), int(o[i]), tuple(int(x) for x in a[i])) for i in range(len(r))] == hits


@pytest.mark.parametrize('kind,case_min,ctrl_max', [('SmallCounttable', 6, 1), ('Nodetable', 1, 0)])
def test_skm_scan_from_the_distinct_list_nibble_and_bit_counters(hk, ok, skm, kind, case_min, ctrl_max):
    """four-bit counters saturate at 15, one-bit ones at 1: the controls' abundance lists reject by min(count, what a counter holds)"""
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    reads = trio_reads(80000, 24000, 53)
    got, hits = scan_both(hk, ok, reads, 31, 8e6, hint=True, kind=kind, case_min=case_min, ctrl_max=ctrl_max)
    assert got == hits and len(hits) > 20
    assert launches('k_skm_novel_list') == 1 and launches('k_skm_novel') == 0


def test_skm_scan_from_the_distinct_list_bands_overflow_skips_and_crowded_buckets(hk, ok, skm):
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    reads = trio_reads(80000, 24000, 47)
    bad = list(reads['proband'][5]); bad[40] = 'N'
    reads['proband'][5] = ''.join(bad)              # flagged: the scan skips it, the count keeps it
    union = []
    for band in range(3):
        got, hits = scan_both(hk, ok, reads, 31, 5e6, hint=True, band_mode=1, nbands=3, band=band)
        assert got == hits
        union += got
    whole, hits = scan_both(hk, ok, reads, 31, 5e6, hint=True)
    assert sorted(union) == whole == hits and len(hits) > 20
    assert launches('k_skm_novel_list') == 4 and launches('k_skm_novel') == 0
    # every abundant k-mer of the case sample is interesting when the controls are all but empty and may hold anything up to
    # 255: far more than a quarter of a bucket's table, so the buckets are marked in instalments
    thin = dict(reads, mother=reads['mother'][:200], father=reads['father'][:200])
    got, hits = scan_both(hk, ok, thin, 31, 5e6, hint=True, case_min=2, ctrl_max=255)
    assert got == hits and len(hits) > 200000
    # undersized segments and a tiny loose list budget in S1 / S2: records and single k-mers travel through the loose list
    os.environ['KV_SKM_CAP_PCT'] = '30'
    got, hits = scan_both(hk, ok, reads, 31, 5e6, hint=True, case_min=5, ctrl_max=2)
    assert got == hits and len(hits) > 20
    os.environ.pop('KV_SKM_CAP_PCT')
    # k-mers that missed the count pass's LDS tables (here: one key in 64, by decree) are on the loose list, one occurrence at a
    # time, not in the distinct list: the scan evaluates those records as the count pass left them, positions included
    os.environ['KV_SKM_FORCE_LOOSE'] = '1'
    before = launches('k_skm_novel_list')
    for k in (31, 51):
        got, hits = scan_both(hk, ok, reads, k, 5e6, hint=True)
        assert got == hits and len(hits) > 20
    os.environ.pop('KV_SKM_FORCE_LOOSE')
    assert launches('k_skm_novel_list') == before + 2 and launches('k_novel_mark') == 0
    before = launches('k_skm_novel')
    # the hint without the reuse (controls counted after the case): the list is gone with the buckets, the scan walks
    got, hits = scan_both(hk, ok, reads, 31, 5e6, hint=True, order=('proband', 'mother', 'father'))
    assert got == hits and launches('k_skm_novel') == before + 1


def test_default_paths_on_a_large_batch_agree_with_the_other_implementations(hk, skm):
    """no knobs: 4.9 M k-mers take the super-k-mer path by default; tables equal those of the partitioned and the
    atomic paths, hits equal those of the tile scan"""
    for name in KNOBS:
        os.environ.pop(name, None)
    from kevlar_amd import synth
    reads = trio_reads(400000, 70000, 51)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    # (packed batches: reads of one length with the arithmetic layout, as bench.py and the device FASTQ parser make them)
    batches = {n: hk.ReadBatch.from_packed(synth.pack_codes(np.searchsorted(letters, np.frombuffer(''.join(reads[n]).encode(), dtype=np.uint8).reshape(len(reads[n]), 100))), 100)
               for n in reads}
    sk = {}
    for path in (None, 'binned', 'binned-tiles', 'atomic'):
        if path:
            os.environ['KV_COUNT_PATH'] = path.split('-')[0]
        else:
            os.environ.pop('KV_COUNT_PATH', None)
        if path == 'binned-tiles':
            os.environ['KV_BIN_2BIT'] = '0'              # the partition's tile front end (reads of one length take the 2-bit one by default)
        else:
            os.environ.pop('KV_BIN_2BIT', None)
        sk[path] = {n: hk.Counttable(31, 2e7 / 4, 4) for n in ('mother', 'father', 'proband')}
        for n in ('mother', 'father', 'proband'):
            assert sk[path][n].consume_batch(batches[n]) == 70000 * 70
    os.environ.pop('KV_COUNT_PATH', None)
    os.environ.pop('KV_BIN_2BIT', None)
    assert launches('k_skm_count') == 3 and launches('k_bin_hash_2bit') == 3 and launches('k_bin_hash_direct') == 3 and launches('k_consume') == 3
    for n in reads:
        for t in range(4):
            assert sk[None][n].table_bytes(t) == sk['binned'][n].table_bytes(t) == sk['binned-tiles'][n].table_bytes(t) == sk['atomic'][n].table_bytes(t)
        assert sk[None][n].n_occupied() == sk['atomic'][n].n_occupied()
    res = {}
    for path in (None, 'tiles'):
        if path:
            os.environ['KV_NOVEL_PATH'] = path
        r, o, a, _ = hk.novel_scan([sk[None]['proband']], [sk[None]['mother'], sk[None]['father']], batches['proband'], 6, 1)
        res[path] = (r.tolist(), o.tolist(), a.tolist())
    assert res[None] == res['tiles'] and len(res[None][0]) > 100
    assert launches('k_skm_novel') == 1 and launches('k_novel_mark') == 1


def test_list_scan_first_probe_from_the_bit_map_equals_the_table_probe(hk, ok, skm):
    """the list scan answers its first question -- is table 0 of the first case sample at least case-min here? -- from a bit map of that
    table (k_case_bits: one bit per bin, an eighth of the table); KV_NOVEL_BITS=0 probes the table itself: same hits, both equal to the
    oracle's, for thresholds that few k-mers fail and that most do"""
    os.environ['KV_SKM_BUCKET_KMERS'] = '2048'
    reads = trio_reads(100000, 30000, 91)
    for case_min in (2, 6, 25):
        for bits in ('1', '0'):
            os.environ['KV_NOVEL_BITS'] = bits
            before_bits, before_list = launches('k_case_bits'), launches('k_skm_novel_list')
            got, hits = scan_both(hk, ok, reads, 31, 6e6, hint=True, case_min=case_min)
            assert got == hits, (case_min, bits, len(got), len(hits))
            assert launches('k_skm_novel_list') == before_list + 1
            assert launches('k_case_bits') == before_bits + (1 if bits == '1' else 0)
        assert case_min > 6 or len(hits) > 50           # (at 25 nothing is left: every first probe fails, the bit map's best case)
    os.environ.pop('KV_NOVEL_BITS', None)


@pytest.mark.parametrize('k', [31, 51])
def test_count_instance_compiled_for_k_equals_the_one_that_reads_k(hk, skm, k):
    """k = 31 (kevlar's default) and k = 51 (BASELINE.json configs[4]) have their own instances of the count kernel (k, masks,
    shifts and the murmur tail are constants there); KV_SKM_ANY_K keeps the instance that reads k from the geometry: same
    tables, same occupancy, and the same hits from a scan behind either"""
    reads = trio_reads(300000, 40000, 77)
    batches = {n: hk.ReadBatch(reads[n]) for n in reads}
    sk = {}
    for generic in (False, True):
        if generic:
            os.environ['KV_SKM_ANY_K'] = '1'
        sk[generic] = {n: hk.Counttable(k, 1.5e7 / 4, 4) for n in ('mother', 'father', 'proband')}
        for n in ('mother', 'father', 'proband'):
            if n == 'proband':
                sk[generic][n].expect_scan(True)
            assert sk[generic][n].consume_batch(batches[n]) == 40000 * (100 - k + 1)
    for n in reads:
        for t in range(4):
            assert sk[False][n].table_bytes(t) == sk[True][n].table_bytes(t)
        assert sk[False][n].n_occupied() == sk[True][n].n_occupied()
    res = {}
    for generic in (False, True):
        r, o, a, _ = hk.novel_scan([sk[generic]['proband']], [sk[generic]['mother'], sk[generic]['father']], batches['proband'], 6, 1)
        res[generic] = (r.tolist(), o.tolist(), a.tolist())
    assert res[False] == res[True] and len(res[False][0]) > 50
