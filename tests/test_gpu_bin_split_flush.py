"""Stage B of the partitioned count (k_bin_split, kevlar_amd/csrc/kv_binned.hip) between rounds: every lane decides for its own ring,
then the wave copies the ready bursts four lanes a ring, sixteen rings a pass (rings_flush_quads), and leaves the misfits -- a ring
that overran, a burst that no longer fits the segment -- to rings_flush.  Held to the oracle through the C ABI, every table byte and
n_occupied, on the smallest inputs that reach each path:

  weighted (u32 items, rings of 32 to 4096) and unweighted (u16 items, rings of 64 to 4096) items, from hash lists and from reads;
  tables of 1, 3, 65, 512 and 1153 slices of 2^16 bins: F = 1, 1, 17, 128 and 289 rings per workgroup, so 1, 1, 3, 16 and 37 rings per
  wave -- one ring and one quad, a wave whose last quads have nothing to do, exactly one pass, and three passes with a ragged last one;
  a hash list with a hot slice (a few bins of one slice, as one block) and a warm one (five times its share, spread out) beside a
  uniform background: the hot slice's ring takes more than R items in a round (overrun, then a base that is no multiple of 8: the
  misfit path), both slices' segments fill (the last burst does not fit cap2: overflow and the spill list), and the hot bins
  take far more than 255 additions (saturation).

For a hash list the oracle is h % size in numpy's exact uint64 and a saturating sum per bin (as tests/test_gpu_bigtables.py holds
the hash lists): the CPU oracle's library takes one hash per call.  Reads go through oracle/okhmer.  2^21 hashes a case: with 8
stage-B workgroups per coarse bucket that is 227 items per ring and workgroup at 1153 slices, seven or more bursts each."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 31
N = 1 << 21
KNOBS = ('KV_COUNT_PATH', 'KV_SKM_BUCKET_KMERS')
SLICES = (1, 3, 65, 512, 1153)
WEIGHTS = np.array([1, 2, 3, 127, 128, 255, 256, 1000], dtype=np.int64)


def launches(name):
    from kevlar_amd import _lib
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.load().kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return n.value


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


def size_of(hk, slices):
    """the largest prime that has `slices` slices of 2^16 bins"""
    size = int(hk.primes_below(slices << 16, 1)[0])
    assert (size + 65535) >> 16 == slices
    return size


def uniform_hashes(size, seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 2**64, N, dtype=np.uint64)
    h[:4] = np.array([0, size - 1, size, 2**64 - 1], dtype=np.uint64)         # the first and the last bin are touched
    return h


def skewed_hashes(size, slices, seed):
    """uniform background; 2^19 hashes of three bins of one slice as one block in the middle; 5 x a slice's share spread evenly"""
    rng = np.random.default_rng(seed)
    mult = lambda n: rng.integers(0, (2**64 - 1) // size - 1, n, dtype=np.uint64) * np.uint64(size)
    back = uniform_hashes(size, seed + 1)[:N - (1 << 19)]
    hot_slice, warm_slice = slices // 3, slices // 2
    hot_bins = np.uint64(hot_slice << 16) + np.array([0, 1, 65535], dtype=np.uint64)
    hot = hot_bins[rng.integers(0, 3, 1 << 19)] + mult(1 << 19)
    n_warm = 5 * N // slices
    warm = np.uint64(warm_slice << 16) + rng.integers(0, 65536, n_warm, dtype=np.uint64) + mult(n_warm)
    back[rng.choice(len(back), n_warm, replace=False)] = warm
    h = np.concatenate([back[:len(back) // 2], hot, back[len(back) // 2:]])
    assert len(h) == N and int((hot % np.uint64(size)).max()) < size and int((warm % np.uint64(size)).max()) < size
    return h


def expected_bytes(h, size, w=None):
    """a Counttable's table after the hashes (each w[i] times): every byte, and the bins in use"""
    bins = (h % np.uint64(size)).astype(np.int64)
    sums = np.bincount(bins, weights=None if w is None else w.astype(np.float64), minlength=size)
    table = np.minimum(sums, 255).astype(np.uint8)
    return table, int(np.count_nonzero(table))


def count_list(hk, size, h, w):
    """the list through k_bin_list -> k_bin_split -> k_bin_apply by name; returns the sketch"""
    import torch
    os.environ['KV_COUNT_PATH'] = 'binned'
    dev = hk.Counttable(K, 0, 0, primes=[size])
    if w is None:
        d_h = torch.from_numpy(h.view(np.int64)).cuda()
        assert dev.consume_hashes(d_h.data_ptr(), len(h)) == len(h)
        assert (launches('k_bin_list'), launches('k_bin_split'), launches('k_bin_apply'), launches('k_add_hashes')) == (1, 1, 1, 0)
    else:
        d_pairs = torch.from_numpy(np.stack([h.view(np.int64), w], axis=1)).cuda()
        assert dev.consume_hashes_weighted(d_pairs.data_ptr(), len(h)) == int(w.sum())
        assert (launches('k_bin_list_w'), launches('k_bin_split_w'), launches('k_bin_apply_w'), launches('k_add_hashes_weighted')) == (1, 1, 1, 0)
    return dev


def assert_table(dev, table, occ, what):
    got = np.frombuffer(dev.table_bytes(0), dtype=np.uint8)
    assert got.shape == table.shape, what
    bad = np.flatnonzero(got != table)
    assert len(bad) == 0, '{}: bin {} holds {}, expected {} ({} bins differ)'.format(what, int(bad[0]), int(got[bad[0]]), int(table[bad[0]]), len(bad))
    assert dev.n_occupied() == occ, what


@pytest.mark.parametrize('weighted', [False, True], ids=['u16', 'u32'])
@pytest.mark.parametrize('slices', SLICES)
def test_uniform_hash_list(hk, prof, slices, weighted):
    """every ring of every wave flushes bursts of whole sectors; F = 1, 1, 17, 128, 289"""
    size = size_of(hk, slices)
    h = uniform_hashes(size, 100 + slices)
    w = WEIGHTS[np.arange(N) % len(WEIGHTS)] if weighted else None
    table, occ = expected_bytes(h, size, w)
    assert table[0] and table[size - 1]
    assert_table(count_list(hk, size, h, w), table, occ, '{} slices, {}'.format(slices, 'weighted' if weighted else 'plain'))


@pytest.mark.parametrize('weighted', [False, True], ids=['u16', 'u32'])
@pytest.mark.parametrize('slices', [65, 1153])
def test_hot_and_warm_slice(hk, prof, slices, weighted):
    """ring overrun and the misfit path, segments that fill (overflow, spill list), bins that saturate"""
    size = size_of(hk, slices)
    h = skewed_hashes(size, slices, 200 + slices)
    w = WEIGHTS[np.arange(N) % len(WEIGHTS)] if weighted else None
    table, occ = expected_bytes(h, size, w)
    hot = (slices // 3) << 16
    assert table[hot] == table[hot + 1] == table[hot + 65535] == 255
    per_slice = np.bincount((h % np.uint64(size)).astype(np.int64) >> 16, minlength=slices)
    assert per_slice[slices // 3] >= 1 << 19 and per_slice[slices // 2] >= 5 * (N // slices)
    assert_table(count_list(hk, size, h, w), table, occ, '{} slices, hot and warm, {}'.format(slices, 'weighted' if weighted else 'plain'))


@pytest.fixture(scope='module')
def reads_and_oracle(ok):
    """6000 reads of 100 bases from a 20 kb genome (30 x), and the oracle's four tables of about 3e5 bins after them"""
    rng = np.random.default_rng(11)
    genome = rng.integers(0, 4, size=20000)
    alphabet = np.array(list('ACGT'))
    starts = rng.integers(0, len(genome) - 100, size=6000)
    seqs = [''.join(alphabet[genome[s:s + 100]]) for s in starts]
    ref = ok.Counttable(K, 3e5, 4)
    bases, offs = ok.concat_reads(seqs)
    n = ok.consume_reads(ref, bases, offs, len(seqs))
    assert n == 6000 * (100 - K + 1)
    return seqs, n, [ref.table_bytes(t) for t in range(4)], ref.n_occupied()


@pytest.mark.parametrize('path', ['binned', 'skm'])
def test_reads_through_both_item_forms(hk, prof, reads_and_oracle, path):
    """one item per k-mer (the partition by name: u16 items) and one weighted item per distinct k-mer of a bucket (the super-k-mer
    count: u32 items), every table byte against the oracle"""
    seqs, n, tables, occ = reads_and_oracle
    os.environ['KV_COUNT_PATH'] = path
    os.environ['KV_SKM_BUCKET_KMERS'] = '4096'
    dev = hk.Counttable(K, 3e5, 4)
    assert dev.consume_batch(hk.ReadBatch(seqs)) == n
    if path == 'binned':
        assert (launches('k_bin_split'), launches('k_bin_apply'), launches('k_consume')) == (1, 1, 0)
    else:
        assert (launches('k_skm_count'), launches('k_bin_split_w'), launches('k_bin_apply_w'), launches('k_consume')) == (1, 1, 1, 0)
    for t in range(4):
        assert dev.table_bytes(t) == tables[t], (path, t)
    assert dev.n_occupied() == occ
