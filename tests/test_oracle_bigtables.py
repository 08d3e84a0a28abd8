"""The CPU oracle itself at the table sizes tests/test_gpu_bigtables.py holds the device to: 2^32 - 5, 2^32 + 15 and 6e9 bins, in
bit and nibble storage.  The oracle is the reference of every device comparison there and had never run above 5e8 bins, so it is
pinned here against a restatement in numpy's exact uint64 arithmetic: bins = h % size, counter = min(max, occurrences).  CPU only;
the largest sketch holds 4.3 GB."""
import numpy as np
import pytest

from bigtables_common import COUNTER_MAX, P_README, SWITCH_PRIMES, crafted_hashes, expected_table, is_prime, occupied, oracle_table, \
    stored, storage_of, table_nbytes

K = 31
GEOMETRIES = [[P_README], list(SWITCH_PRIMES[32])]


def test_the_sizes_are_the_primes_next_to_each_switch(ok):
    """the literals of bigtables_common are what the prime search of the oracle finds below each boundary, and the next prime above it"""
    for bits, (below, above) in SWITCH_PRIMES.items():
        assert ok.primes_below(2**bits, 1) == [below]
        assert below < 2**bits < above and is_prime(above)
        assert not any(is_prime(n) for n in range(2**bits + (bits != 31), above))       # (2^31 - 1 is prime, 2^k is not)
    assert ok.primes_below(2e9, 4) == [1999999973, 1999999943, 1999999927, 1999999913]
    assert ok.primes_below(3e9, 1) == [2999999929] and ok.primes_below(6e9, 1) == [5999999989]
    assert ok.primes_below(2.5e8, 3) == [249999991, 249999941, 249999917]


@pytest.fixture(scope='module')
def read_hashes(ok):
    """3000 reads of a synthetic sample, and the hash of each of their k-mers in read order"""
    from kevlar_amd import synth
    seqs = synth.unpack_reads(synth.trio_reads_packed(200_000, 2, 100)['proband'][:3000], 100)
    hashes = [ok.lib.kvo_hash_murmur(s[i:i + K].encode(), K) for s in seqs for i in range(100 - K + 1)]
    return seqs, np.array(hashes, dtype=np.uint64)


@pytest.mark.parametrize('primes', GEOMETRIES, ids=lambda p: '+'.join(str(x) for x in p))
@pytest.mark.parametrize('cls', ['Nodetable', 'SmallCounttable'])
def test_oracle_matches_exact_arithmetic_at_these_sizes(ok, read_hashes, cls, primes, tmp_path):
    seqs, hreads = read_hashes
    rng = np.random.default_rng(21)
    sk = getattr(ok, cls)(K, 0, 0, primes=primes)
    storage = storage_of(sk)
    assert sk.hashsizes() == primes
    bases, offs = ok.concat_reads(seqs)
    assert ok.consume_reads(sk, bases, offs, len(seqs)) == len(hreads)
    crafted = np.concatenate([crafted_hashes(p, rng) for p in primes])
    was_new = np.array([sk.add(int(h)) for h in crafted.tolist()], dtype=bool)
    everything = np.concatenate([hreads, crafted])
    want_get = np.full(len(everything), 255, dtype=np.uint8)
    new_model = np.zeros(len(crafted), dtype=bool)
    for t, size in enumerate(primes):
        view = oracle_table(ok, sk, t)
        assert len(view) == table_nbytes(storage, size)
        uniq, vals = expected_table(everything, size, storage)
        assert int(uniq.max()) == size - 1 and int(uniq.min()) == 0             # the table's last bin (beyond 32 bits where the size is) and its first
        assert vals.max() == COUNTER_MAX[storage]                               # and a counter saturates
        got = stored(view, storage, uniq)
        bad = np.flatnonzero(got != vals)
        assert len(bad) == 0, 'table {} of {} bins: bin {} holds {}, expected {}'.format(t, size, int(uniq[bad[0]]), int(got[bad[0]]), int(vals[bad[0]]))
        assert occupied(view, storage) == len(uniq), 'table {}: a counter outside the touched bins is set'.format(t)
        if t == 0:
            assert sk.n_occupied() == len(uniq)
        want_get = np.minimum(want_get, vals[np.searchsorted(uniq, everything % np.uint64(size))])
        # a hash is new when it finds a zero in ANY table: bins of the crafted hashes not seen before, in order of addition
        bins = crafted % np.uint64(size)
        first = np.zeros(len(crafted), dtype=bool)
        first[np.unique(bins, return_index=True)[1]] = True
        new_model |= first & ~np.isin(bins, hreads % np.uint64(size))
    assert np.array_equal(was_new, new_model)
    sample = np.concatenate([everything[::7], crafted[:10100]])
    want_sample = np.concatenate([want_get[::7], want_get[len(hreads):len(hreads) + 10100]])
    got_sample = np.array([sk.get(int(h)) for h in sample.tolist()], dtype=np.uint8)
    assert np.array_equal(got_sample, want_sample)
    if len(primes) == 1:
        raw = sk.table_bytes(0)                                 # the copy the small tests compare: full length, same bytes
        assert len(raw) == table_nbytes(storage, primes[0])
        assert np.array_equal(np.frombuffer(raw, dtype=np.uint8), oracle_table(ok, sk, 0))
        del raw
    if cls == 'Nodetable':
        path = str(tmp_path / 'big.nt')
        sk.save(path)
        back = ok.Nodetable.load(path)
        assert back.hashsizes() == primes and back.ksize() == K
        for t in range(len(primes)):
            assert np.array_equal(oracle_table(ok, back, t), oracle_table(ok, sk, t))
        assert back.n_occupied() == sk.n_occupied()
        del back
        import os
        os.remove(path)
