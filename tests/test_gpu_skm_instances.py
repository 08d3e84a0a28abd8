"""Every template instance of the super-k-mer kernels, by name, at the edges of the host planners that choose among them
(tests/instances_common.py is the table: the cases, and for each the exact instances kv_skm_last_instances must report).  A row runs
its entry point, asserts the report, and holds the result to the scalar oracle: the return value, every table byte and the occupancy
of a count; every (read, offset, abundances) of a scan; the owners' sketches of a route or an exchange.  Everything is exact."""
import ctypes
import functools
import os

import numpy as np
import pytest

from instances_common import CASES, KNOBS, split_report

pytestmark = pytest.mark.gpu

TABLESIZE, NTABLES = 9e5, 4


def launched():
    from kevlar_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    assert _lib.load().kv_skm_last_instances(buf, len(buf)) == 0
    return split_report(buf.value.decode())


@pytest.fixture
def skm():
    """The super-k-mer path by name (it is the default only from 4 M k-mers up); every knob a row sets is removed behind it."""
    os.environ['KV_COUNT_PATH'] = 'skm'
    os.environ['KV_NOVEL_PATH'] = 'skm'
    yield
    for name in KNOBS:
        os.environ.pop(name, None)


@functools.lru_cache(maxsize=None)
def trio():
    from kevlar_amd import synth
    return synth.make_trio(60000, 61, inherited_per_mb=400, denovo_per_mb=400)


@functools.lru_cache(maxsize=None)
def sampled(sample, n, read_len):
    """n reads of read_len bases of one sample of the trio: (packed words, strings); computed once, shared, never changed"""
    from kevlar_amd import synth
    words = synth.sample_reads_packed(trio()[sample], n, read_len, 0.005, 62 + 7 * ('proband', 'mother', 'father').index(sample) + read_len)
    words.setflags(write=False)
    return words, tuple(synth.unpack_reads(words, read_len))


@functools.lru_cache(maxsize=None)
def shape_reads(shape, n):
    """the named batches of the table: (strings, packed words or None)"""
    if shape == 'polyA_AC':                 # one minimizer from end to end; every m-mer of (AC)n ties with the one two bases on
        reads = ['A' * 100] * (n // 2) + ['AC' * 50] * (n - n // 2)
        return tuple(reads), None
    if shape == 'with_N':                   # reads of one length, as strings: N at base 0, at the last base, at bases 15 and 16; lower case
        reads = list(sampled('proband', n - 5, 100)[1])
        src = reads[:5]
        extra = ['N' + src[0][1:], src[1][:-1] + 'N', src[2][:15] + 'N' + src[2][16:], src[3][:16] + 'N' + src[3][17:], src[4].lower()]
        return tuple(reads[:1000] + extra + reads[1000:]), None
    if shape == 'ragged':                   # the shape of tests/test_gpu_skm.py's ragged batch: lengths 10..259, reads shorter than k, segment tiles
        rng = np.random.default_rng(12)
        letters = np.array(list('ACGT'))

        def rnd(m):
            return ''.join(letters[rng.integers(0, 4, size=m)])
        chrom = rnd(20011)
        reads = [rnd(int(rng.integers(10, 260))) for _ in range(n - 17)]
        reads += ['', 'ACG', rnd(30), rnd(31), rnd(32), chrom, rnd(7680), rnd(7681 + 30), rnd(8200), 'A' * 150, 'ACGT' * 40]
        reads += [chrom[100:400], chrom[100:400], chrom[10000:10300]]
        bad = list(rnd(140)); bad[70] = 'N'
        reads += [''.join(bad), rnd(50) + 'acgtn' + rnd(50), rnd(259)]
        assert len(reads) == n
        return tuple(reads), None
    if shape in ('polyA_547', 'polyA_656'):  # 547 x 120 = 65640 occurrences of A x 31, 656 x 100 = 65600 of A x 51, among ordinary reads
        n_poly = int(shape.split('_')[1])
        words, reads = sampled('proband', n - n_poly, 150)
        poly = np.zeros((n_poly, words.shape[1]), dtype=np.uint32)
        words = np.concatenate([words[:1500], poly, words[1500:]])
        return tuple(reads[:1500]) + ('A' * 150,) * n_poly + tuple(reads[1500:]), words
    raise KeyError(shape)


def reads_of(row, sample='proband'):
    if isinstance(row['shape'], int):
        words, reads = sampled(sample, row['n'], row['shape'])
        return reads, words, row['shape']
    reads, words = shape_reads(row['shape'], row['n'])
    return reads, words, len(reads[0])


def batch_of(hk, row, reads, words, read_len):
    if row['make'] == 'packed':
        return hk.ReadBatch.from_packed(np.ascontiguousarray(words), read_len)
    return hk.ReadBatch(list(reads))


def same_tables(dev, ref, what):
    for t in range(len(ref.hashsizes())):
        assert dev.table_bytes(t) == ref.table_bytes(t), '{}: table {} differs from the oracle'.format(what, t)
    assert dev.n_occupied() == ref.n_occupied(), what


def count_both(hk, ok, row, sample, hint, want):
    """one sample counted on the device and by the oracle: report, return value, tables"""
    reads, words, read_len = reads_of(row, sample)
    dev, ref = hk.Counttable(row['k'], TABLESIZE, NTABLES), ok.Counttable(row['k'], TABLESIZE, NTABLES)
    if hint:
        dev.expect_scan()
    batch = batch_of(hk, row, reads, words, read_len)
    n_dev = dev.consume_batch(batch)
    assert launched() == want, (sample, row['why'])
    bases, offs = ok.concat_reads(list(reads))
    n_ref = ok.consume_reads(ref, bases, offs, len(reads))
    assert n_dev == n_ref == sum(max(0, len(r) - row['k'] + 1) for r in reads)
    same_tables(dev, ref, sample)
    return dev, ref, batch, (bases, offs, len(reads))


def same_hits(ok, got, cases, ctrls, oracle_reads, k, case_min, ctrl_max):
    r, o, a = got
    bases, offs, n = oracle_reads
    wr, wo, wa = ok.novel_scan_mt(cases, ctrls, bases, offs, n, k, case_min, ctrl_max, 4)
    assert len(r) == len(wr)
    assert np.array_equal(np.asarray(r, dtype=np.int64), wr.astype(np.int64)) and np.array_equal(np.asarray(o, dtype=np.int64), wo.astype(np.int64))
    assert np.array_equal(np.asarray(a).reshape(len(wr), -1), wa)
    return len(wr)


def run_count_scan(hk, ok, row):
    dev, ref, batch, oracle_reads = count_both(hk, ok, row, 'proband', row['hint'], row['expect']['count'])
    k = row['k']
    if row['shape'] in ('polyA_547', 'polyA_656'):
        assert dev.get('A' * k) == ref.get('A' * k) == 255
    r, o, a, _ = hk.novel_scan([dev], [], batch, 1, 0)
    assert launched() == row['expect']['scan'], row['why']
    n_hits = same_hits(ok, (r, o, a), [ref], [], oracle_reads, k, 1, 0)
    # (no control, case-min 1: every k-mer position of every read the scan does not skip)
    assert n_hits > 0


def run_trio(hk, ok, row):
    dev, ref = {}, {}
    for sample in ('mother', 'father', 'proband'):            # the case sample last: the scan can reuse its buckets
        case = sample == 'proband'
        dev[sample], ref[sample], batch, oracle_reads = count_both(hk, ok, row, sample, case and row['hint'], row['expect']['case' if case else 'count'])
    r, o, a, _ = hk.novel_scan([dev['proband']], [dev['mother'], dev['father']], batch, 3, 0)
    assert launched() == row['expect']['scan'], row['why']
    assert same_hits(ok, (r, o, a), [ref['proband']], [ref['mother'], ref['father']], oracle_reads, row['k'], 3, 0) > 20


def weighted_sketch(hk, k, pairs, first, n):
    sk = hk.Counttable(k, TABLESIZE, NTABLES)
    got = sk.consume_hashes_weighted(pairs[first:].data_ptr(), n) if n else 0
    return sk, got


def run_route(hk, ok, row):
    import torch
    reads, words, read_len = reads_of(row)
    batch = batch_of(hk, row, reads, words, read_len)
    k, ndest = row['k'], 2
    nk = batch.num_kmers(k)
    pairs = torch.zeros((nk, 2), dtype=torch.int64, device='cuda')
    counts = hk.route_distinct(batch, hk.Counttable, k, ndest, pairs.data_ptr(), nk)
    assert launched() == row['expect']['route'], row['why']
    assert sum(counts) < nk                                   # the shard was deduplicated
    bases, offs = ok.concat_reads(list(reads))
    first = 0
    for b in range(ndest):
        ref = ok.Counttable(k, TABLESIZE, NTABLES)
        n_ref = ok.consume_reads(ref, bases, offs, len(reads), ndest, b)
        sk, n_dev = weighted_sketch(hk, k, pairs, first, counts[b])
        assert n_dev == n_ref
        same_tables(sk, ref, 'band {}'.format(b))
        first += counts[b]


def run_exchange(hk, ok, row):
    import torch
    reads, words, read_len = reads_of(row)
    batch = batch_of(hk, row, reads, words, read_len)
    k = row['k']
    nk = batch.num_kmers(k)
    keep_scan = 'set_scan' in row['expect']
    plan = hk.mex_plan(hk.Counttable, k, len(reads), read_len, 1, short=row['short'])
    assert int(plan.flags) & 1 == (1 if row['short'] else 0)
    seg = torch.zeros(int(plan.seg_words), dtype=torch.int64, device='cuda')
    cnt = torch.zeros(int(plan.cnt_entries), dtype=torch.int32, device='cuda')
    hk.mex_emit(batch, plan, 0, seg.data_ptr(), cnt.data_ptr())
    assert launched() == row['expect']['emit'], row['why']
    pairs = torch.zeros((nk, 2), dtype=torch.int64, device='cuda')
    counts, arrived = hk.mex_route(plan, 0, seg.data_ptr(), cnt.data_ptr(), 1, pairs.data_ptr(), nk, keep_scan=keep_scan)
    assert launched() == row['expect']['route'], row['why']
    assert arrived == nk and counts[0] < nk
    # the band owner's sketch (one owner: the whole sample) against the oracle
    bases, offs = ok.concat_reads(list(reads))
    ref = ok.Counttable(k, TABLESIZE, NTABLES)
    assert ok.consume_reads(ref, bases, offs, len(reads)) == nk
    sk, n_dev = weighted_sketch(hk, k, pairs, 0, counts[0])
    assert n_dev == nk
    same_tables(sk, ref, 'the owner')
    if not keep_scan:
        return
    # the owner judges its distinct k-mers, then answers the scan for its buckets from the set of interesting hashes
    case_min = 3
    hashes = torch.empty(counts[0], dtype=torch.int64, device='cuda')
    abund = torch.empty((counts[0], 1), dtype=torch.uint8, device='cuda')
    n_int = hk.novel_scan_distinct([sk], [], pairs.data_ptr(), counts[0], case_min, 0, hashes.data_ptr(), abund.data_ptr(), counts[0])
    cap = nk + 64
    tags = torch.full((cap,), -1, dtype=torch.int64, device='cuda')              # (padding carries tag ~0, as the gather leaves it)
    rows = torch.zeros((cap, 1), dtype=torch.uint8, device='cuda')
    n_hits = hk.mex_scan_set(hk.Counttable, k, 1, hashes.data_ptr(), abund.data_ptr(), n_int, tags.data_ptr(), rows.data_ptr(), cap)
    assert launched() == row['expect']['set_scan'], row['why']
    tags[n_hits:] = -1
    torch.cuda.synchronize()
    r, o, a = hk.hits_from_tagged(tags.data_ptr(), rows.data_ptr(), cap, n_hits, 1)
    assert same_hits(ok, (r, o, a), [ref], [], (bases, offs, len(reads)), k, case_min, 0) > 20


RUN = {'count_scan': run_count_scan, 'trio': run_trio, 'route': run_route, 'exchange': run_exchange}


@pytest.mark.parametrize('row', CASES, ids=[c['id'] for c in CASES])
def test_instance_row(hk, ok, skm, row):
    os.environ.update(row['knobs'])
    RUN[row['entry']](hk, ok, row)
