"""What the tests of very large tables share (tests/test_gpu_bigtables.py on the device, tests/test_oracle_bigtables.py and
tests/test_skm_host.py on the host): the table sizes on either side of every size-class switch of the library, hashes
chosen to hurt a quotient estimate, and the numpy restatement of a table -- bins = h % size in exact uint64 arithmetic,
counter = min(max, occurrences) -- with readers of the three storage forms that never unpack a multi-gigabyte table.
Not a test module and not a conftest: nothing here is collected."""
import ctypes

import numpy as np

# primes next to 2^16 (FP64 fastmod begins), 2^30 (stage A of the bin path: 64 coarse buckets, 1024 threads), 2^31 (the 32-bit
# remainder of k_skm_count ends; the partitioned counts end), 2^32 (FP64 -> Barrett, bins beyond 32 bits): (below, above)
SWITCH_PRIMES = {16: (65521, 65537), 30: (1073741789, 1073741827), 31: (2147483647, 2147483659), 32: (4294967291, 4294967311)}
P_BAND, P_MID, P_README = 1999999973, 2999999929, 5999999989      # bench.py's cfg4-band table, a 2^31..2^32 table, `novel --memory 24G`
FILLERS = [249999991, 249999941, 249999917]                        # primes_below(2.5e8, 3)
ALL_SIZES = [p for pair in SWITCH_PRIMES.values() for p in pair] + [P_BAND, P_MID, P_README]
COUNTER_MAX = {'byte': 255, 'nibble': 15, 'bit': 1}


def is_prime(n):
    """deterministic Miller-Rabin for n < 3.3e24"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41):
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def crafted_hashes(size, rng, n_mult=2000, n_random=200000):
    """multiples of `size` and their neighbours (where a quotient estimate is one off), the top of the 64-bit range, the
    edges of the double's mantissa, and random hashes: the set of test_skm_host.py::test_fastmod_is_the_remainder"""
    q = (2**64 - 1) // size
    edge = []
    for mult in [0, 1, 2, q // 3, q // 2, q - 1, q] + [int(x) for x in rng.integers(0, q + 1, n_mult, dtype=np.uint64)]:
        for d in (-2, -1, 0, 1, 2):
            v = mult * size + d
            if 0 <= v < 2**64:
                edge.append(v)
    edge += [2**64 - 1, 2**64 - 2, 2**63, 2**63 - 1, 2**53, 2**53 + 1, 2**52 - 1]
    return np.concatenate([np.array(edge, dtype=np.uint64), rng.integers(0, 2**64, n_random, dtype=np.uint64)])


def storage_of(sketch):
    return {'Counttable': 'byte', 'Countgraph': 'byte', 'SmallCounttable': 'nibble', 'SmallCountgraph': 'nibble'}.get(type(sketch).__name__, 'bit')


def table_nbytes(storage, size):
    return size if storage == 'byte' else (size // 2 + 1 if storage == 'nibble' else size // 8 + 1)


def oracle_table(ok, sketch, t):
    """table t of an oracle sketch as a numpy view of the oracle's own memory (no copy: keep the sketch alive)"""
    n = ctypes.c_uint64()
    p = ok.lib.kvo_table_bytes(sketch._h, t, ctypes.byref(n))
    return np.ctypeslib.as_array(p, shape=(int(n.value),))


def device_table(sketch, t, out=None):
    """table t of a device sketch read into one numpy array (kv_sketch_table_read), without the bytes() copy of table_bytes()"""
    from kevlar_amd import _lib
    nbytes = table_nbytes(storage_of(sketch), sketch.hashsizes()[t])
    buf = out[:nbytes] if out is not None else np.empty(nbytes, dtype=np.uint8)
    _lib.check(_lib.load().kv_sketch_table_read(sketch._h, t, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), nbytes))
    return buf


def stored(view, storage, bins):
    """the counters of `bins` (uint64 array) in a table's on-disk form: a byte per bin, two bins per byte with the even bin in the
    HIGH nibble, or eight bins per byte from bit 0 up"""
    bins = np.asarray(bins, dtype=np.uint64)
    if storage == 'byte':
        return view[bins]
    if storage == 'nibble':
        sh = np.where(bins & np.uint64(1), 0, 4).astype(np.uint8)
        return (view[bins >> np.uint64(1)] >> sh) & np.uint8(15)
    return (view[bins >> np.uint64(3)] >> (bins & np.uint64(7)).astype(np.uint8)) & np.uint8(1)


def occupied(view, storage, chunk=1 << 28):
    """number of non-zero counters of a whole table, by blocks: set bits, non-zero nibbles or non-zero bytes"""
    total = 0
    for lo in range(0, len(view), chunk):
        part = view[lo:lo + chunk]
        if storage == 'byte':
            total += int(np.count_nonzero(part))
        elif storage == 'nibble':
            total += int(np.count_nonzero(part & np.uint8(0xf0))) + int(np.count_nonzero(part & np.uint8(0x0f)))
        else:
            pad = part if len(part) % 8 == 0 else np.concatenate([part, np.zeros(8 - len(part) % 8, dtype=np.uint8)])
            total += int(np.bitwise_count(pad.view(np.uint64)).sum(dtype=np.uint64))
    return total


def doubled(part, storage):
    """the bytes of a table in which every counter was added to itself, saturating: what counting the same batch again leaves.
    min(max, 2 c) = (min(c, max >> 1) << 1) | (c > max >> 1), in uint8 passes only (a table here has gigabytes)"""
    if storage == 'bit':
        return part
    if storage == 'byte':
        return (np.minimum(part, np.uint8(127)) << 1) | (part > 127).astype(np.uint8)
    hi, lo = part >> 4, part & np.uint8(15)
    hi = (np.minimum(hi, np.uint8(7)) << 1) | (hi > 7).astype(np.uint8)
    lo = (np.minimum(lo, np.uint8(7)) << 1) | (lo > 7).astype(np.uint8)
    return (hi << 4) | lo


def first_bin_above(view, storage, boundary):
    """is there a non-zero counter at a bin >= boundary?  (the size class is really used, not just allocated)"""
    per = {'byte': 1, 'nibble': 2, 'bit': 8}[storage]
    start = (boundary + per - 1) // per
    tail = view[start:]
    for lo in range(0, len(tail), 1 << 28):
        if tail[lo:lo + (1 << 28)].any():
            return True
    return False


def expected_table(hashes, size, storage, weights=None):
    """(distinct bins, counter of each) after adding every hash once -- or weights[i] times -- to an empty table of `size` bins"""
    bins = np.asarray(hashes, dtype=np.uint64) % np.uint64(size)
    if weights is None:
        uniq, counts = np.unique(bins, return_counts=True)
    else:
        uniq, inv = np.unique(bins, return_inverse=True)
        counts = np.bincount(inv, weights=np.asarray(weights, dtype=np.float64), minlength=len(uniq)).astype(np.uint64)
    return uniq, np.minimum(counts, COUNTER_MAX[storage]).astype(np.uint8)


def first_difference(got, want, storage, twice=False, chunk=1 << 27):
    """None if two tables' bytes are equal, else (bin, found, expected) of the first bin that differs; twice: `want` with every
    counter doubled (saturating) is what is expected"""
    assert got.shape == want.shape, 'table lengths differ: {} / {}'.format(got.shape, want.shape)
    per = {'byte': 1, 'nibble': 2, 'bit': 8}[storage]
    for lo in range(0, len(got), chunk):
        a, b = got[lo:lo + chunk], want[lo:lo + chunk]
        if twice:
            b = doubled(b, storage)
        if np.array_equal(a, b):
            continue
        at = int(np.flatnonzero(a != b)[0])
        for j in range(per):
            x, y = int(stored(a, storage, [at * per + j])[0]), int(stored(b, storage, [at * per + j])[0])
            if x != y:
                return (lo + at) * per + j, x, y
        return (lo + at) * per, int(a[at]), int(b[at])
    return None
