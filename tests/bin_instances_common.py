"""The case table of the partitioned count (kv_binned.hip: stage A k_bin_hash_2bit / k_bin_hash_direct / k_bin_list, stage B k_bin_split,
stage C k_bin_apply, k_bin_spill): one row per case, each with the exact list of template instances kv_bin_last_instances must report,
the numbers of the plan kv_bin_last_plan must report, and the planner condition the row stands on.  Shared by
tests/test_gpu_bin_instances.py (runs every row on the GPU, holds it to the oracle), tests/test_bin_instances_ledger.py (no GPU: the
instances named here are exactly the ones the launch sites of kv_binned.hip can launch) and tests/test_bin_plan.py (no GPU: the
planner's header gives every geometry's plan).  Not collected itself.

The plan literals are derived from the planner's arithmetic (bin_shape of kevlar_amd/csrc/kv_bin_plan.h, which kv_bin_plan runs) and
written down; tests/test_bin_plan.py asks the header and the GPU rows ask the report whether the planner still agrees.
With maxsl = the most slices of 2^16 bins of any table of the sketch:

  cmax      the bucket budget: min(32, max(4, ceil(maxsl / 384))) up to 32 x 512 = 16384 slices (2^30 bins), 64 beyond.  Four buckets
            up to 1536 slices, five from 1537; 32 from 11905 slices on.
  F, C      F = ceil(maxsl / cmax) slices per coarse bucket, C = ceil(maxsl / F) buckets in use.  F = 1 up to four slices (recipF == 0:
            the kernels take the slice as the bucket); five slices are F = 2, C = 3, the multiply-high division, and a last bucket of
            one slice.  With cmax pinned at 32 from 12289 slices on F passes the 384 the planner aims at: 385 .. 512, the latter at
            exactly 16384 slices.  One slice more is 64 buckets of 257.
  ringB     stage B's ring entries per slice stream: the largest power of two <= 4096 with ringB x F <= 16384, at least 64 -- 4096 up
            to F = 4, halving behind F = 4, 8, 16, 32, 64, 128, and 64 from F = 129 on.  Weighted items (u32) get half the entries
            per byte: at least 32, ringB x F x 4 <= 32768, so 2048 at F = 4 and 32 from F = 129 on; 4096 for F <= 2.
  threadsA  512 with cmax <= 32, 1024 with 64 buckets.
  waves     stage B has one lane per slice stream, 8 waves: ceil(F / 8) rings per wave -- two from F = 9, nine from F = 65, 33 from
            F = 257.

A boundary S (in slices) is visited from both sides by sketches of two tables: `below` = the two largest primes with S slices (lo(S),
lo2(S): what khmer's prime search gives for a target of S x 2^16), `above` = [hi(S), lo(S)] with hi(S) the smallest prime beyond
S x 2^16 -- S + 1 slices, the last of them a handful of bins wide (stage C sees nb tiny and nvec == 1), beside a table of one slice
less whose last coarse bucket is short or absent.  This is what the prime search produces whenever a target straddles a multiple of
65536.  The primes are literals; tests/test_bin_instances_ledger.py::test_the_primes_are_what_the_table_says holds them to both prime
searches and to trial division."""
import functools
import re

import numpy as np

from instances_common import COUNT_31, COUNT_C_31, LANE_1_8, LOOSE_COUNT_1, SORT_2, SORT_3, TILE_16

# ---- the instances, by the names the launch sites give them (blanks removed) ----------------------------------------------------
STORAGE = {'Counttable': 'ST_BYTE', 'Countgraph': 'ST_BYTE', 'SmallCounttable': 'ST_NIBBLE', 'Nodetable': 'ST_BIT', 'Nodegraph': 'ST_BIT'}
SPILL = 'k_bin_spill'


def two_bit(threads, kw, fixed_k=None):
    return 'k_bin_hash_2bit<{},{}{}>'.format(threads, kw, ',{}'.format(fixed_k) if fixed_k else '')


def direct(threads, nw):
    return 'k_bin_hash_direct<{},{}>'.format(threads, nw)


def from_list(threads, weighted):
    return 'k_bin_list<{},{}>'.format(threads, 'true' if weighted else 'false')


def split(weighted):
    return 'k_bin_split<{}>'.format('true' if weighted else 'false')


def apply(cls, weighted):
    return 'k_bin_apply<{},{}>'.format(STORAGE[cls], 'true' if weighted else 'false')


def after(stage_a, cls, weighted):
    """the whole report of one partitioned count: stage A (None: the super-k-mer count fed the buckets), B, C, the spill list"""
    return ([stage_a] if stage_a else []) + [split(weighted), apply(cls, weighted), SPILL]


# what the super-k-mer count launches in front of the weighted stages (tests/instances_common.py has these at their own edges)
SKM_PACKED_K31 = [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1]       # equal-length reads, k = 31, no scan announced: 16-byte records
SKM_RAGGED_K31 = [TILE_16, SORT_3, COUNT_31, LOOSE_COUNT_1]

# every knob a row may set (the test removes them all after each row)
KNOBS = ('KV_COUNT_PATH', 'KV_SKM_BUCKET_KMERS')
SKM_BUCKET_KMERS = '512'

N_READS, N_HASHES = 8000, 1 << 18
N_MASK_READS, N_FIRST_BATCH = 2000, 2000
N_SKEW, N_POLY_A = 2000, 700

# ---- the geometries ---------------------------------------------------------------------------------------------------------------
# (id, sketch class, [table sizes], (maxsl, cmax, F, C, ringB of u16 items, threadsA), ringB of weighted items, what flips here)
# Counters of a byte below 256 slices; bits from there on, so that a table of 2^30 bins is 128 MB.
GEOMETRIES = [
    ('S1-below', 'Counttable', [65521, 65519], (1, 4, 1, 1, 4096, 512), 4096, 'one slice, one bucket: tables below 2^16 bins'),
    ('S1-above', 'Counttable', [65537, 65521], (2, 4, 1, 2, 4096, 512), 4096, 'a second bucket, one bin wide; table 1 has none'),
    ('S4-below', 'Counttable', [262139, 262133], (4, 4, 1, 4, 4096, 512), 4096, 'F = 1 with all four buckets: recipF == 0, the slice is the bucket'),
    ('S4-above', 'Counttable', [262147, 262139], (5, 4, 2, 3, 4096, 512), 4096, 'F = 2: slice / F by multiply-high; C = 3, the last bucket one slice of 3 bins'),
    ('S16-below', 'Counttable', [1048573, 1048571], (16, 4, 4, 4, 4096, 512), 2048, 'F = 4: the last full u16 ring, the weighted ring already halved'),
    ('S16-above', 'Counttable', [1048583, 1048573], (17, 4, 5, 4, 2048, 512), 1024, 'F = 5: ringB halves'),
    ('S32-below', 'Counttable', [2097143, 2097133], (32, 4, 8, 4, 2048, 512), 1024, 'F = 8: one ring per wave'),
    ('S32-above', 'Counttable', [2097169, 2097143], (33, 4, 9, 4, 1024, 512), 512, 'F = 9: two rings per wave, ringB halves'),
    ('S64-below', 'Counttable', [4194301, 4194287], (64, 4, 16, 4, 1024, 512), 512, 'F = 16'),
    ('S64-above', 'Counttable', [4194319, 4194301], (65, 4, 17, 4, 512, 512), 256, 'F = 17: ringB halves'),
    ('S128-below', 'Counttable', [8388593, 8388587], (128, 4, 32, 4, 512, 512), 256, 'F = 32'),
    ('S128-above', 'Counttable', [8388617, 8388593], (129, 4, 33, 4, 256, 512), 128, 'F = 33: ringB halves'),
    ('S256-below', 'Nodetable', [16777213, 16777199], (256, 4, 64, 4, 256, 512), 128, 'F = 64: eight rings per wave'),
    ('S256-above', 'Nodetable', [16777259, 16777213], (257, 4, 65, 4, 128, 512), 64, 'F = 65: nine rings per wave, ringB halves'),
    ('S512-below', 'Nodetable', [33554393, 33554383], (512, 4, 128, 4, 128, 512), 64, 'F = 128'),
    ('S512-above', 'Nodetable', [33554467, 33554393], (513, 4, 129, 4, 64, 512), 32, 'F = 129: both rings at their minimum'),
    ('S1024-below', 'Nodetable', [67108859, 67108837], (1024, 4, 256, 4, 64, 512), 32, 'F = 256: 32 rings per wave'),
    ('S1024-above', 'Nodetable', [67108879, 67108859], (1025, 4, 257, 4, 64, 512), 32, 'F = 257: 33 rings per wave'),
    ('S1536-below', 'Nodetable', [100663291, 100663261], (1536, 4, 384, 4, 64, 512), 32, 'the last four-bucket geometry, F = 384'),
    ('S1536-above', 'Nodetable', [100663319, 100663291], (1537, 5, 308, 5, 64, 512), 32, 'cmax 4 -> 5'),
    ('S12288-below', 'Nodetable', [805306357, 805306349], (12288, 32, 384, 32, 64, 512), 32, 'the last F <= 384 with 32 buckets'),
    ('S12288-above', 'Nodetable', [805306457, 805306357], (12289, 32, 385, 32, 64, 512), 32, 'F = 385 under 512-thread workgroups'),
    ('S16384-below', 'Nodetable', [1073741789, 1073741783], (16384, 32, 512, 32, 64, 512), 32, 'exactly 2^30 bins: F = 512 = BIN_MAX_F, the last 512-thread geometry'),
    ('S16384-above', 'Nodetable', [1073741827, 1073741789], (16385, 64, 257, 64, 64, 1024), 32, '3 bins beyond 2^30: 64 buckets, 1024 threads'),
]
# lo(S), lo2(S), hi(S) as the geometries use them: S -> (largest prime with S slices, the prime before it, smallest prime beyond S x 2^16)
BOUNDARY_PRIMES = {int(g[0][1:].split('-')[0]): None for g in GEOMETRIES}
for _id, _cls, _primes, _plan, _rw, _why in GEOMETRIES:
    _s = int(_id[1:].split('-')[0])
    if _id.endswith('below'):
        BOUNDARY_PRIMES[_s] = (_primes[0], _primes[1], None)
    else:
        assert BOUNDARY_PRIMES[_s][0] == _primes[1]
        BOUNDARY_PRIMES[_s] = BOUNDARY_PRIMES[_s][:2] + (_primes[0],)

# the two sketches the instance rows run on
SMALL = dict(primes=[917503, 917471], plan=(14, 4, 4, 4, 4096, 512), ring_w=2048, threads=512)      # two tables of 14 slices (lo(14), lo2(14))
WIDE = dict(primes=[1073741827, 1073741789], plan=(16385, 64, 257, 64, 64, 1024), ring_w=32, threads=1024)   # [hi(16384), lo(16384)]

CASES = []


def case(id, entry, cls, primes, plan, expect, why, k=31, path='binned', shape=100, n=N_READS, skm=None, variant=None, weighted=False, big=''):
    """entry     'packed'   ReadBatch.from_packed of n reads of `shape` bases of the trio's proband (reads())
                 'strings'  ReadBatch of the strings of the named batch `shape` (test_gpu_skm_instances.shape_reads)
                 'list'     n hashes (hashes()) through consume_hashes, or with weighted=True (hash, weight) pairs through
                            consume_hashes_weighted
       path      KV_COUNT_PATH of a reads row: 'binned' (one item per k-mer) or 'skm' (one weighted item per distinct k-mer of a bucket;
                 `skm` is then the list kv_skm_last_instances must report as well, so that a decline into another path cannot pass)
       expect    the exact list kv_bin_last_instances must report
       plan      (maxsl, cmax, F, C, ringB, threadsA) kv_bin_last_plan must report
       variant   None | 'band' (nbands = 4, band = 3) | 'mask', 'mask-kept' (a Nodetable of the first 2000 reads as the mask, consume_masked
                 False / True) | 'second' (the first 2000 reads counted before: the tables are loaded, not zero by decree) |
                 'skew' (700 poly-A reads among 2000: one bin takes 700 x (100 - k + 1) items)
       why       the planner condition the row stands on (shown when the row fails)
       big       the reason of a row beyond 8000 reads or 2^18 hashes"""
    assert entry in ('packed', 'strings', 'list') and path in ('binned', 'skm') and (path == 'skm') == (skm is not None)
    assert variant in (None, 'band', 'mask', 'mask-kept', 'second', 'skew') and len(plan) == 6 and expect and why
    CASES.append(dict(id=id, entry=entry, cls=cls, primes=list(primes), plan=tuple(plan), expect=expect, why=why, k=k, path=path, shape=shape, n=n,
                      skm=skm, variant=variant, weighted=weighted, big=big))


def weighted_plan(plan, ring_w):
    return plan[:4] + (ring_w,) + plan[5:]


# ---- geometry rows: every boundary from both sides, four entries each ------------------------------------------------------------
for gid, cls, primes, plan, ring_w, why in GEOMETRIES:
    threads = plan[5]
    case(gid + '-packed', 'packed', cls, primes, plan, after(two_bit(threads, 1, 31), cls, False), why)
    case(gid + '-skm', 'packed', cls, primes, weighted_plan(plan, ring_w), after(None, cls, True), why, path='skm', skm=SKM_PACKED_K31)
    case(gid + '-list', 'list', cls, primes, plan, after(from_list(threads, False), cls, False), why, n=N_HASHES)
    case(gid + '-listw', 'list', cls, primes, weighted_plan(plan, ring_w), after(from_list(threads, True), cls, True), why, n=N_HASHES, weighted=True)

# ---- instance rows: every stage-A instance on SMALL (512 threads) and on WIDE (1024 threads, 64 buckets) -----------------------
for tag, geo, cls in (('small', SMALL, 'Counttable'), ('wide', WIDE, 'Nodetable')):
    T, primes, plan, wplan = geo['threads'], geo['primes'], geo['plan'], weighted_plan(geo['plan'], geo['ring_w'])
    graph = 'Countgraph' if tag == 'small' else 'Nodegraph'
    for k, L, name, why in [(31, 100, two_bit(T, 1, 31), 'k == 31: the fixed-k instance'), (25, 100, two_bit(T, 1), 'one-word k-mers of any k'),
                            (51, 150, two_bit(T, 2), 'two-word k-mers'), (64, 100, two_bit(T, 2), 'k = 64 = SKM_MAX_K: the last k of the 2-bit form'),
                            (16, 100, two_bit(T, 1), 'k = 16 = SKM_MIN_K: the first')]:
        case('{}-packed-k{}'.format(tag, k), 'packed', cls, primes, plan, after(name, cls, False), why, k=k, shape=L)
    for k, c, name, why in [(31, cls, direct(T, 8), 'ragged reads: no 2-bit form; k <= 32 rolls in 8 words'), (51, cls, direct(T, 16), 'k <= 64: 16 words'),
                            (80, cls, direct(T, 0), 'k > 64: no rolling hash'), (31, graph, direct(T, 0), 'the 2-bit hash of the graphs: no rolling hash')]:
        case('{}-ragged-{}-k{}'.format(tag, c, k), 'strings', c, primes, plan, after(name, c, False), why, k=k, shape='ragged', n=1517)
    case(tag + '-list', 'list', cls, primes, plan, after(from_list(T, False), cls, False), 'a hash list', n=N_HASHES)
    case(tag + '-listw', 'list', cls, primes, wplan, after(from_list(T, True), cls, True), 'a list of (hash, weight)', n=N_HASHES, weighted=True)
    case(tag + '-skew', 'packed', cls, primes, plan, after(two_bit(T, 1, 31), cls, False), 'one bin takes 49000 items: its segment fills, the rest spills',
         n=N_SKEW, variant='skew')

# SMALL: the three storage forms through both item forms -- the six k_bin_apply<ST, W> and both k_bin_split<W>
for cls in ('Counttable', 'SmallCounttable', 'Nodetable'):
    primes, plan, wplan = SMALL['primes'], SMALL['plan'], weighted_plan(SMALL['plan'], SMALL['ring_w'])
    if cls != 'Counttable':         # (Counttable: small-packed-k31 and small-ragged-Counttable-k31 above)
        case('small-packed-k31-' + cls, 'packed', cls, primes, plan, after(two_bit(512, 1, 31), cls, False), 'storage form of stage C')
        case('small-ragged-k31-' + cls, 'strings', cls, primes, plan, after(direct(512, 8), cls, False), 'storage form of stage C', shape='ragged', n=1517)
    case('small-packed-k31-skm-' + cls, 'packed', cls, primes, wplan, after(None, cls, True), 'storage form of stage C, weighted', path='skm', skm=SKM_PACKED_K31)
    case('small-ragged-k31-skm-' + cls, 'strings', cls, primes, wplan, after(None, cls, True), 'storage form of stage C, weighted', path='skm', skm=SKM_RAGGED_K31,
         shape='ragged', n=1517)

# WIDE: a band or a mask filter in front of 64 buckets, and tables that are loaded
for variant, why in (('band', 'band 3 of 4 in front of 64 buckets'), ('mask', 'a mask in front of 64 buckets: k-mers the mask lacks'),
                     ('mask-kept', 'consume_masked: k-mers the mask holds'), ('second', 'a second batch: stage C loads the slices')):
    case('wide-packed-k25-' + variant, 'packed', 'Nodetable', WIDE['primes'], WIDE['plan'], after(two_bit(1024, 1), 'Nodetable', False), why, k=25, variant=variant)
    case('wide-ragged-k51-' + variant, 'strings', 'Nodetable', WIDE['primes'], WIDE['plan'], after(direct(1024, 16), 'Nodetable', False), why, k=51, shape='ragged',
         n=1517, variant=variant)

assert len({c['id'] for c in CASES}) == len(CASES)


def split_report(text):
    """a report into names: it is comma separated, and a name's own commas stand between its angle brackets"""
    return re.split(r',(?![^<]*>)', text) if text else []


def declared_instances():
    """every instance some row expects"""
    return {name for c in CASES for name in c['expect']}


def rows_by_instance():
    out = {}
    for c in CASES:
        for name in c['expect']:
            out.setdefault(name, []).append(c['id'])
    return out


# ---- inputs (computed once, shared, never changed) and the references that need no oracle ---------------------------------------
@functools.lru_cache(maxsize=None)
def trio():
    from kevlar_amd import synth
    return synth.make_trio(60000, 61, inherited_per_mb=400, denovo_per_mb=400)


@functools.lru_cache(maxsize=None)
def reads(n, read_len):
    """n reads of read_len bases of the trio's proband: (packed words, strings)"""
    from kevlar_amd import synth
    words = synth.sample_reads_packed(trio()['proband'], n, read_len, 0.005, 62 + read_len)
    words.setflags(write=False)
    return words, tuple(synth.unpack_reads(words, read_len))


@functools.lru_cache(maxsize=None)
def skewed_reads():
    """N_POLY_A reads of 100 x A in the middle of N_SKEW - N_POLY_A reads of the proband"""
    words, strings = reads(N_SKEW - N_POLY_A, 100)
    half = len(strings) // 2
    poly = np.zeros((N_POLY_A, words.shape[1]), dtype=np.uint32)
    out = np.concatenate([words[:half], poly, words[half:]])
    out.setflags(write=False)
    return out, strings[:half] + ('A' * 100,) * N_POLY_A + strings[half:]


def hashes(primes, n=N_HASHES):
    """n random hashes; the first ones touch the first and the last bin of both tables and the top of the 64-bit range"""
    rng = np.random.default_rng(primes[0] % 100003)
    h = rng.integers(0, 2**64, n, dtype=np.uint64)
    h[:5] = np.array([0, primes[0] - 1, primes[0], primes[1] - 1, 2**64 - 1], dtype=np.uint64)
    return h


COUNTER_MAX = {'ST_BYTE': 255, 'ST_NIBBLE': 15, 'ST_BIT': 1}


BINS_PER_BYTE = {'ST_BYTE': 1, 'ST_NIBBLE': 2, 'ST_BIT': 8}


def expected_table(h, size, cls, w=None):
    """(the bytes of a table of `size` bins after the hashes, each w[i] times; its bins in use).  bins = h % size in numpy's exact uint64, a
    saturating sum per bin, and the stored form of tests/bigtables_common.py (table_nbytes, stored): a byte per bin; two bins per byte, the
    even bin in the high nibble, size // 2 + 1 bytes; eight bins per byte from bit 0 up, size // 8 + 1 bytes.  Built from the distinct bins, so
    that a table of 2^30 bins costs its 128 MB and no more."""
    st = STORAGE[cls]
    uniq, inv = np.unique(h % np.uint64(size), return_inverse=True)
    sums = np.bincount(inv.ravel(), weights=None if w is None else w.astype(np.float64), minlength=len(uniq))
    counters = np.minimum(sums, COUNTER_MAX[st]).astype(np.uint8)
    assert counters.all()
    uniq = uniq.astype(np.int64)
    if st == 'ST_BYTE':
        out = np.zeros(size, dtype=np.uint8)
        out[uniq] = counters
    elif st == 'ST_NIBBLE':
        out = np.zeros(size // 2 + 1, dtype=np.uint8)
        np.bitwise_or.at(out, uniq >> 1, counters << np.where(uniq & 1, 0, 4).astype(np.uint8))
    else:
        out = np.zeros(size // 8 + 1, dtype=np.uint8)
        np.bitwise_or.at(out, uniq >> 3, np.uint8(1) << (uniq & 7).astype(np.uint8))
    return out, len(uniq)


def bucket_ranges(size, F):
    """[first bin, end) of every coarse bucket of F slices that a table of `size` bins has a bin in"""
    step = F << 16
    return [(lo, min(lo + step, size)) for lo in range(0, size, step)]


def any_bin_in_use(table, cls, lo, hi):
    """is a counter of bins [lo, hi) of a table's bytes non-zero?  lo is a multiple of 65536, hi another or the table's size (the bytes
    behind the last bin are zero)"""
    per = BINS_PER_BYTE[STORAGE[cls]]
    assert lo % 65536 == 0
    return bool(table[lo // per:(hi + per - 1) // per].any())


if __name__ == '__main__':              # python tests/bin_instances_common.py: every instance with the rows that reach it
    for name, ids in sorted(rows_by_instance().items()):
        print('{:32s} {:3d}  {}'.format(name, len(ids), ' '.join(ids[:5]) + (' ...' if len(ids) > 5 else '')))
    print(len(CASES), 'rows')
