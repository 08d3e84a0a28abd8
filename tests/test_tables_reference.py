"""The inputs of tests/test_gpu_tables.py, with the oracle alone: the device test compares hit lists with the oracle's, which proves
something only where the loops it is after change the answer.  Held here, on the CPU: the two parents sit behind the first eight
controls of the 16-sample scan and reject what nobody in front of them does; the strangers around them reject nothing; sixteen
crowded tables, eight of them and one give three different hit lists; every geometry is what its name says, and every scan finds
something.  The figures measured when the module was written stand beside each assertion; the assertions are the inequalities."""
import pytest

import tables_common as tc


def test_geometries_are_what_their_names_say(ok):
    for name, spec in tc.COUNT_GEOMETRIES.items():
        primes = tc.primes_of(ok, spec)
        assert 1 <= len(primes) <= tc.MAX_TABLES and len(set(primes)) == len(primes), name
    assert [len(tc.primes_of(ok, tc.COUNT_GEOMETRIES[n])) for n in ('C1x3e5', 'C2x3e5', 'C3x3e5', 'C5x1e5', 'C8x1e5', 'C16x1e5', 'N7x1e6')] == [1, 2, 3, 5, 8, 16, 7]
    assert all(p < 65536 for p in tc.primes_of(ok, tc.COUNT_GEOMETRIES['C4x4e4']))
    straddle = tc.primes_of(ok, tc.COUNT_GEOMETRIES['C4straddle'])
    assert sum(p < 65536 for p in straddle) == 1 and all(p < 2**31 for p in straddle)
    assert all(2**16 <= p < 2**31 for p in tc.primes_of(ok, tc.COUNT_GEOMETRIES['C4x3e5']))         # the fast4 row
    # all table counts from 1 to 16 that a kernel branches on are somewhere among the sketches of the scans
    counts = {len(tc.primes_of(ok, s)) for scan in (tc.SIXTEEN, tc.TWO_CASES, tc.mixed_scan(1, 1), tc.NIBBLE_CASE_SCAN) for s in scan.cases + scan.ctrls}
    assert {1, 2, 3, 4, 6, 11, 16} <= counts
    assert len(tc.SIXTEEN.cases + tc.SIXTEEN.ctrls) == tc.MAX_SAMPLES == len(tc.TWO_CASES.cases + tc.TWO_CASES.ctrls)
    assert len(tc.SEVENTEEN.cases + tc.SEVENTEEN.ctrls) == tc.MAX_SAMPLES + 1
    assert tc.SIXTEEN.ctrls.index(tc.MOTHER) == 8 and tc.SIXTEEN.ctrls.index(tc.FATHER) == 11       # samples 9 and 12
    assert tc.TWO_CASES.ctrls[-2:] == (tc.MOTHER, tc.FATHER)
    assert len({s.kind for s in tc.SIXTEEN.ctrls}) == 3


def test_counts_are_not_trivial(ok):
    """two batches change the tables twice, a band keeps a part, the skew saturates a counter in every table, and every mask holds back some
    k-mers but not all"""
    for k in tc.KS:
        total = tc.N_READS * (tc.READ_LEN - k + 1)
        (n1, s1), (n2, s2) = tc.oracle_two_batches(ok, tc.COUNT_GEOMETRIES['C3x3e5'], k)
        assert n1 == n2 == total and s1[0] != s2[0] and s2[1] > s1[1] > 0
        (b1, t1), _ = tc.oracle_two_batches(ok, tc.COUNT_GEOMETRIES['C3x3e5'], k, nbands=4, band=3)
        assert 0 < b1 < total / 2 and t1[1] < s1[1]
        for spec, top in ((tc.COUNT_GEOMETRIES['C3x3e5'], 255), (tc.COUNT_GEOMETRIES['S3x3e5'], 15)):
            sk = tc.make(ok, spec, k, ok)
            tc.oracle_count(ok, sk, 'skew')
            assert sk.get('A' * k) == top
        for name in tc.MASK_CASES:
            # consume_masked false skips a k-mer the mask holds more than `threshold` times, true skips one it holds less often: with
            # threshold 0 nothing is below it
            threshold = tc.MASK_CASES[name][1]
            kept = tc.oracle_masked(ok, name, k, False)[0]
            taken = tc.oracle_masked(ok, name, k, True)[0]
            assert 0 < kept < total and kept != taken, name
            assert (taken == total) if threshold == 0 else (0 < taken < total), name


@pytest.mark.parametrize('k', tc.KS)
def test_every_scan_of_the_device_test_finds_something(ok, k):
    seen = []
    for tables in (1, 3, 4, 9, 16):
        for ctrl_max in (1, 0):
            seen.append(tc.oracle_hits(ok, tc.mixed_scan(tables, ctrl_max), k))
            assert len(seen[-1][0]) > 0, (tables, ctrl_max)
        # the bit table can only reject at ctrl_max 0: there it does
        assert len(seen[-1][0]) < len(seen[-2][0])
    for scan in (tc.NIBBLE_CASE_SCAN, tc.SIXTEEN, tc.TWO_CASES, tc.SIXTEEN_TABLES):
        hits = tc.oracle_hits(ok, scan, k)
        assert len(hits[0]) > 0
        ncase = len(scan.cases)
        assert (hits[2][:, :ncase] >= scan.case_min).all() and (hits[2][:, ncase:] <= scan.ctrl_max).all()
    assert len(tc.oracle_hits(ok, tc.TWO_CASES, k, scanned='sibling')[0]) > 0
    # the second case sample takes hits away from the first (its loop is not idle)
    assert len(tc.oracle_hits(ok, tc.TWO_CASES, k)[0]) < len(tc.oracle_hits(ok, tc.SIXTEEN, k)[0])


def test_the_parents_behind_the_first_eight_controls_decide(ok):
    """measured at k = 31: 2162 hits with all 15 controls, 472350 with the first 8, 473025 with none, 2162 with the parents alone"""
    all15, first8, none, parents = (tc.oracle_hits(ok, s, 31) for s in (tc.SIXTEEN, tc.FIRST_EIGHT, tc.NO_CONTROL, tc.PARENTS_ONLY))
    assert len(all15[0]) > 0
    assert len(first8[0]) > 10 * len(all15[0])
    assert len(none[0]) >= len(first8[0])
    # a scan that ignored the strangers would pass, one that ignored the controls behind the eighth would not: the strangers reject nothing
    assert (tc.positions(all15) == tc.positions(parents)).all() and len(all15[0]) == len(parents[0])


def test_sixteen_tables_eight_and_one_give_different_hits(ok):
    """measured at k = 31: 2472 hits with 16 tables on case and mother, 2479 with the first 8 of those primes on both, 43004 with table 0
    of the case alone"""
    sixteen = tc.oracle_hits(ok, tc.SIXTEEN_TABLES, 31)
    eight = tc.oracle_hits(ok, tc.Scan((tc.first_primes(ok, tc.CROWDED_CASE, 8),), (tc.first_primes(ok, tc.CROWDED, 8),), tc.CASE_MIN, tc.CTRL_MAX), 31)
    one = tc.oracle_hits(ok, tc.Scan((tc.first_primes(ok, tc.CROWDED_CASE, 1),), (tc.CROWDED,), tc.CASE_MIN, tc.CTRL_MAX), 31)
    lists = [tc.positions(h).tolist() for h in (sixteen, eight, one)]
    assert all(len(x) > 0 for x in lists)
    assert lists[0] != lists[1] and lists[0] != lists[2] and lists[1] != lists[2]
    # the abundances reported with a hit are the minimum over ALL tables: a reduction over the first four would report something else
    four = tc.oracle_sketch(ok, tc.first_primes(ok, tc.CROWDED, 4), 31)
    full = tc.oracle_sketch(ok, tc.CROWDED, 31)
    kmers = [tc.reads('proband')[int(r)][int(o):int(o) + 31] for r, o in zip(sixteen[0][:400], sixteen[1][:400])]
    assert any(four.get(km) != full.get(km) for km in kmers)
