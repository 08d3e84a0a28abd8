"""S2's sorted split (k_skm_split_sorted<RECW>, kv_skm_emit_device.h) at the edges of its chunk loop, of its counters in dynamic LDS and
of its segment walk, each case held to the scalar oracle exactly: the k-mers added, every table byte, the occupancy, every hit of the
scan.  A host-only test at the end holds what the kernel's speed rests on: no scratch, and two workgroups of the largest chunk the
source names in a CU's registers and LDS.

How a case knows what an S2 workgroup sees.  The records of a batch of n equal-length homopolymer reads are known without running
anything: every m-mer of a read is the same, so a read is ONE run, and with L - k + 1 = 10 k-mers (fewer than any layout's ncap:
22 / 34 / 46 for 16- / 24- / 32-byte records) one record.  The verbose line's record count is held to n.  Who gets them:

  S1, the lane cut   groups of 64 reads, group g to wave g % 8 of workgroup g / 8 while the batch has at most 8 nwg1 groups, and
                     nwg1 = ceil(ceil(n / 64) / 8) (64 reads a tile at these lengths, 8 tiles a ticket; at most 768): workgroup b
                     cuts reads [512 b, 512 b + 512) into its segment of each coarse bucket
  S2                 nwg2 = min(16, 1024 / C1, nwg1) workgroups per coarse bucket; workgroup x drains segments x, x + nwg2, ...

With ONE bucket (C1 = F2 = 1) S2 workgroup x therefore holds sum over j of |reads of S1 workgroup x + j nwg2|, and n alone places
a workgroup at 1 record, at a chunk less one, a whole chunk (where a segment, the chunk and the prefix all end together: the
segment walk's last step), a chunk and one, and two chunks and one.  F2 = 1 is also the smallest F2 there is: one counter, `hist`
and `off` degenerate.  Poly-A reads alone fall into ONE fine bucket whatever the grid: with two fine buckets that one receives whole
chunks and the other nothing, and with several coarse buckets every workgroup of all but one has 0 records.  The chunk sizes are
read from the kernel's source, not repeated here."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_skm_instances as inst
from instances_common import KNOBS, ONE_BUCKET, SORT_2, SORT_3, SORT_4, LIST_1

import __graft_entry__

TABLESIZE, NTABLES = inst.TABLESIZE, inst.NTABLES
EMIT_HEADER = os.path.join(__graft_entry__.CSRC, 'kv_skm_emit_device.h')
SORTED = {2: SORT_2, 3: SORT_3, 4: SORT_4}
# how a batch gets each record layout: 16 bytes (a control: no scan announced, k <= 32), 24 (a case sample, k = 31), 32 (k = 51)
LAYOUT = {2: dict(k=31, L=40, hint=False), 3: dict(k=31, L=40, hint=True), 4: dict(k=51, L=60, hint=False)}


def chunk_of(recw):
    """records per chunk of k_skm_split_sorted<recw>, from the source"""
    with open(EMIT_HEADER) as fh:
        m = re.search(r'constexpr uint32_t skm_s2_chunk\(int recw\) \{ return recw == 2 \? (\d+)u : recw == 3 \? (\d+)u : (\d+)u; \}', fh.read())
    assert m, 'skm_s2_chunk is no longer the one-liner this test reads'
    return int(m.group(recw - 1))


def bucket_grid(nfine):
    """skm_bucket_grid of kv_skm.hip: (C1, F2)"""
    def pow2_ceil(v):
        p = 1
        while p < v:
            p <<= 1
        return p
    F2 = min(512, pow2_ceil(int(np.ceil(np.sqrt(nfine)))))
    if nfine > 255 * F2:
        F2 = min(4096, pow2_ceil((nfine + 254) // 255))
    return min(255, max(1, (nfine + F2 - 1) // F2)), F2


def s2_totals(n, C1):
    """records of the S2 workgroups of the coarse bucket that receives n one-record reads (module docstring)"""
    groups = -(-n // 64)
    nwg1 = min(768, -(-groups // 8))
    assert groups <= 8 * nwg1
    per_s1 = [min(512, n - 512 * b) for b in range(nwg1)]
    nwg2 = max(1, min(16, 1024 // C1, nwg1))
    return [sum(per_s1[x::nwg2]) for x in range(nwg2)]


@pytest.fixture
def skm():
    os.environ['KV_COUNT_PATH'] = 'skm'
    os.environ['KV_NOVEL_PATH'] = 'skm'
    os.environ['KV_SKM_VERBOSE'] = '1'
    yield
    for name in KNOBS + ('KV_SKM_VERBOSE',):
        os.environ.pop(name, None)


def fresh_geometry(hk, k):
    """A batch whose bucket count lies within a quarter of the previous build's of the same k takes that build's grid: a tiny count at
    another k in front, so that the batch under test gets the grid its own size asks for."""
    os.environ['KV_SKM_BUCKET_KMERS'] = '64'
    hk.Counttable(21, 1e4, 2).consume_batch(hk.ReadBatch(['ACGTTGCAAGGCTTAGCATCGATCGGATTACAGCATCGGCTAAGCTT']))
    assert k != 21


def verbose_records(capfd):
    """(records outside their segments, records, bytes per record) of the count's verbose line"""
    m = re.search(r'(\d+) of (\d+) records \((\d+) bytes each\) outside their segments', capfd.readouterr().err)
    assert m, 'no verbose line of the bucketed count: the batch took another path'
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def count_and_scan(hk, ok, capfd, recw, k, hint, batch, reads, scan_from_list=None):
    """count, then scan with no control and case-min 1 (every k-mer position is a hit), both against the oracle; the count's S2
    instance by name.  Returns the verbose line's figures."""
    dev, ref = hk.Counttable(k, TABLESIZE, NTABLES), ok.Counttable(k, TABLESIZE, NTABLES)
    if hint:
        dev.expect_scan()
    capfd.readouterr()
    n_dev = dev.consume_batch(batch)
    names = inst.launched()
    assert len(names) >= 3 and names[1] == SORTED[recw], names
    figures = verbose_records(capfd)
    assert figures[2] == 8 * recw
    bases, offs = ok.concat_reads(list(reads))
    assert n_dev == ok.consume_reads(ref, bases, offs, len(reads)) == sum(max(0, len(r) - k + 1) for r in reads)
    inst.same_tables(dev, ref, 'the count')
    r, o, a, _ = hk.novel_scan([dev], [], batch, 1, 0)
    if scan_from_list is not None:
        assert scan_from_list in inst.launched(), inst.launched()
    assert inst.same_hits(ok, (r, o, a), [ref], [], (bases, offs, len(reads)), k, 1, 0) == n_dev
    return figures


def homopolymers(n, L):
    """n reads of L bases, A x L, C x L, G x L, T x L in turn: (packed words, strings)"""
    wpr = (L + 15) // 16
    code = (np.arange(n, dtype=np.uint64) % 4)[:, None]
    words = np.repeat(code * 0x55555555, wpr, axis=1)
    if L % 16:
        words[:, -1] &= (1 << (2 * (L % 16))) - 1
    return words.astype(np.uint32), ['ACGT'[i % 4] * L for i in range(n)]


# n by the chunk C of the layout, and what the S2 workgroups then hold (held to s2_totals in the test)
EDGES = {'one-record': (lambda C: 1, lambda C: [1]),
         '512-and-1': (lambda C: 513, lambda C: [512, 1]),
         'chunk-less-1': (lambda C: 16 * C - 1, lambda C: [C] * 15 + [C - 1]),
         'whole-chunks': (lambda C: 16 * C, lambda C: [C] * 16),
         'chunk-and-1': (lambda C: 16 * C + 1, lambda C: [C + 1] + [C] * 15),
         'two-chunks-and-1': (lambda C: 32 * C + 1, lambda C: [2 * C + 1] + [2 * C] * 15)}


@pytest.mark.gpu
@pytest.mark.parametrize('recw', [2, 3, 4])
@pytest.mark.parametrize('edge', list(EDGES))
def test_chunk_edges_one_bucket(hk, ok, skm, capfd, recw, edge):
    lay, C = LAYOUT[recw], chunk_of(recw)
    n, want = EDGES[edge][0](C), EDGES[edge][1](C)
    assert C % 512 == 0 and s2_totals(n, 1) == want
    os.environ['KV_SKM_BUCKET_KMERS'] = ONE_BUCKET
    if lay['hint']:
        os.environ['KV_SKM_DL'] = '1'
    words, reads = homopolymers(n, lay['L'])
    batch = hk.ReadBatch.from_packed(words, lay['L'])
    loose, records, _ = count_and_scan(hk, ok, capfd, recw, lay['k'], lay['hint'], batch, reads)
    assert records == n and loose == 0


@pytest.mark.gpu
@pytest.mark.parametrize('recw', [2, 3, 4])
def test_one_fine_bucket_takes_whole_chunks(hk, ok, skm, capfd, recw):
    """poly-A alone, two fine buckets of one coarse bucket (buckets of half the batch's k-mers): one of them receives a chunk and one
    record in workgroup 0 and a chunk in each of the others, the other one nothing.  (With more coarse buckets S1's segments of the
    one bucket would overflow before a chunk's worth reached S2.)"""
    lay, C = LAYOUT[recw], chunk_of(recw)
    n = 16 * C + 1
    n_kmers = n * (lay['L'] - lay['k'] + 1)
    target = (n_kmers + 1) // 2
    assert bucket_grid(-(-n_kmers // target)) == (1, 2) and s2_totals(n, 1) == [C + 1] + [C] * 15
    fresh_geometry(hk, lay['k'])
    os.environ['KV_SKM_BUCKET_KMERS'] = str(target)
    if lay['hint']:
        os.environ['KV_SKM_DL'] = '1'
    L = lay['L']
    words, reads = np.zeros((n, (L + 15) // 16), dtype=np.uint32), ['A' * L] * n
    batch = hk.ReadBatch.from_packed(words, L)
    loose, records, _ = count_and_scan(hk, ok, capfd, recw, lay['k'], lay['hint'], batch, reads)
    assert records == n and loose == 0


@pytest.mark.gpu
@pytest.mark.parametrize('recw', [2, 3, 4])
def test_workgroups_without_records(hk, ok, skm, capfd, recw):
    """513 poly-A reads among buckets of 64 k-mers: several coarse buckets, and every S2 workgroup of all but one of them has 0 records
    (that one's two workgroups have at most 512 and 1: S1's segments of the one bucket are smaller than 512 records here, the rest
    travels through the loose list)"""
    lay, n = LAYOUT[recw], 513
    C1, F2 = bucket_grid(-(-n * (lay['L'] - lay['k'] + 1) // 64))
    assert C1 > 1 and F2 > 1
    fresh_geometry(hk, lay['k'])
    if lay['hint']:
        os.environ['KV_SKM_DL'] = '1'
    L = lay['L']
    words, reads = np.zeros((n, (L + 15) // 16), dtype=np.uint32), ['A' * L] * n
    batch = hk.ReadBatch.from_packed(words, L)
    _, records, _ = count_and_scan(hk, ok, capfd, recw, lay['k'], lay['hint'], batch, reads)
    assert records == n


@pytest.mark.gpu
@pytest.mark.parametrize('recw', [2, 3, 4])
def test_cap2_overflows_inside_a_chunk(hk, ok, skm, capfd, recw):
    """Segments at 30 % of their size, and 547 / 656 poly-A reads of 150 bases among ordinary ones: their records (three to six a read)
    are cut by two S1 workgroups and all belong to one fine bucket, whose S2 segments hold two dozen -- cap2 is passed inside a chunk, by
    16-byte records (which leave in the loose list's 24-byte form), by 24-byte records of a case sample whose scan is then answered
    from the distinct list, and by 32-byte records."""
    k, shape, n = (51, 'polyA_656', 3656) if recw == 4 else (31, 'polyA_547', 3547)
    os.environ.update(KV_SKM_BUCKET_KMERS='512', KV_SKM_CAP_PCT='30')
    hint = recw == 3
    if hint:
        os.environ['KV_SKM_DL'] = '1'
    reads, words = inst.shape_reads(shape, n)
    batch = hk.ReadBatch.from_packed(np.ascontiguousarray(words), 150)
    loose, records, _ = count_and_scan(hk, ok, capfd, recw, k, hint, batch, reads, scan_from_list=LIST_1 if hint else None)
    assert 0 < loose < records


def random_reads(n, L, seed):
    from kevlar_amd import synth
    assert L % 16 == 0
    words = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, L // 16), dtype=np.uint64).astype(np.uint32)
    return words, synth.unpack_reads(words, L)


# The counters are sized by the launch's F2.  The smallest F2 is 1 (test_chunk_edges_one_bucket).  The largest for which the planner
# starts the sorted kernel is SKM_S2_MAXF = 1024 (every chunk holds two records per bucket of it); the planner's F2 is 1024 from
# 255 x 512 + 1 = 130561 buckets up to 255 x 1024.  Reads of random bases at 64 k-mers a bucket: (recw, k, L, reads)
F2_EDGES = [(2, 31, 96, 132000), (3, 31, 96, 132000), (4, 51, 144, 93000)]


@pytest.mark.gpu
@pytest.mark.parametrize('recw,k,L,n', F2_EDGES, ids=['16-byte', '24-byte', '32-byte'])
def test_largest_f2(hk, ok, skm, capfd, recw, k, L, n):
    C1, F2 = bucket_grid(-(-n * (L - k + 1) // 64))
    assert F2 == 1024 and 2 * F2 <= chunk_of(recw)
    fresh_geometry(hk, k)
    hint = recw == 3
    if hint:
        os.environ['KV_SKM_DL'] = '1'
    words, reads = random_reads(n, L, 900 + recw)
    batch = hk.ReadBatch.from_packed(words, L)
    count_and_scan(hk, ok, capfd, recw, k, hint, batch, reads)


def test_sorted_split_fits_two_workgroups_per_cu(tmp_path):
    """Host only.  kv_skm.hip compiled for gfx950 with the compiler's resource remarks: every instance of the sorted split stays inside
    the 128 registers of four waves per SIMD (two workgroups of 512 threads per CU) without scratch, and its static LDS plus a launch's
    dynamic LDS -- at config 2's F2 = 256 and at the largest F2 -- fits a CU's 160 KB twice.  (Three workgroups per CU at 80 registers
    and chunks of 2048 / 1536 records were measured and lost to this: 0.72 against 0.57 ms per launch of 16-byte records at config 2.)"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    done = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage',
                           '-c', 'kv_skm.hip', '-o', str(tmp_path / 'kv_skm.device.o')], cwd=__graft_entry__.CSRC, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    usage = {}
    for block in done.stderr.split('Function Name: ')[1:]:
        m = re.match(r'\S*k_skm_split_sortedILi(\d)E', block)
        if m:
            usage[int(m.group(1))] = {key: int(val) for key, val in re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', block)}
    assert sorted(usage) == [2, 3, 4]
    for recw in (2, 3, 4):
        u = usage[recw]
        print(recw, u)
        assert u['VGPRs'] <= 128 and u['AGPRs'] == 0 and u['ScratchSize'] == 0 and u['Occupancy'] >= 4
        for F2 in (256, 1024):
            dynamic = chunk_of(recw) * recw * 8 + 3 * F2 * 4
            assert u['LDS Size'] + dynamic <= 160 * 1024 // 2
