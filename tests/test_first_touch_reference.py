"""The inputs of tests/test_gpu_first_touch.py, with the oracle alone.  The device test compares kv_unique_new, kv_unique_exact and
kv_abundance_distribution with the oracle's single thread, which proves something only where a wrong first-toucher rule changes the
answer.  Held here, on the CPU: a pure Python model of the rule (tests/first_touch_common.py) gives the oracle's figures for every
case the device test runs; each of five named wrong rules gives other figures in every case that says it catches that rule; the
histogram inputs reach the saturated entry; the boundary batch is what it says; the last bin of a table of every storage is hit.
The figures measured when the module was written stand beside the assertions; the assertions are the inequalities."""
import pytest

import first_touch_common as ft

MODELLED = [c for c in ft.CASES if c.variant != 'dirty']            # the model's inputs hold only A, C, G and T


def test_cases_are_what_they_say(ok):
    ids = [ft.case_id(c) for c in ft.CASES]
    assert len(set(ids)) == len(ids)
    assert set(ft.GEOMETRIES) == {c.geometry for c in ft.GRID} and set(ft.KINDS) == {c.kind for c in ft.GRID}
    for kind in ft.KINDS:
        assert {c.k for c in ft.GRID if c.kind == kind} == set(ft.ks_of(kind))
    assert ft.ks_of('Counttable') == (21, 32, 33, 51) and ft.ks_of('Nodegraph') == (21, 32)
    assert all(p < 100 for p in ft.geometry(ok, 'tiny4')) and len(ft.geometry(ok, 'tiny4')) == 4
    assert len(ft.geometry(ok, 'mid16')) == 16 and all(p < 1500 for p in ft.geometry(ok, 'mid16'))
    assert sum(p < 65536 for p in ft.geometry(ok, 'straddle')) == 1 and ft.geometry(ok, 'single')[0] > 65536
    assert all(p % 2 == 0 for p in ft.geometry(ok, 'even3'))
    assert all(p <= 65543 for name in ft.GEOMETRIES + ('even3',) for p in ft.geometry(ok, name))
    for k in ft.KS:
        assert any(len(s) < k for s in ft.MAIN) and any(len(s) >= k for s in ft.MAIN)
    assert set(''.join(ft.MAIN + ft.PRIOR + ft.MASK_READS + ft.UNIFORM + ft.SECOND)) == set('ACGT')
    assert len(set(ft.MAIN)) < len(ft.MAIN) and set(ft.PRIOR) & set(ft.MAIN) and set(ft.PRIOR) - set(ft.MAIN)
    assert any(ft.revcomp(s) in ft.MAIN for s in ft.MAIN if s != ft.revcomp(s))
    assert {len(s) for s in ft.UNIFORM + ft.UNIFORM_PRIOR} == {ft.UNIFORM_LEN}
    dirty = [c for c in ft.CASES if c.variant == 'dirty']
    for case in dirty:
        text = ''.join(r for batch in ft.batches_of(case)[0] for r in batch)
        assert 'N' in text and any(c in text for c in 'acgt')
        assert ft.oracle_tracked(ok, case).new != ft.oracle_tracked(ok, case._replace(variant='', catches=ft.RULES)).new
    # every option of the count is somewhere: both bands, both mask storages, thresholds 0 and 2, consume_masked both ways
    assert {(c.nbands, c.band) for c in ft.CASES} >= {(0, 0), (4, 2), (9, 8)}
    assert {c.mask for c in ft.CASES} >= {None, ('Nodetable', 0, False), ('Counttable', 0, False), ('Counttable', 2, False), ('Counttable', 2, True)}
    assert {c.variant for c in ft.CASES} == {'', 'dirty', 'packed', 'cleared'}


@pytest.mark.parametrize('case', MODELLED, ids=ft.case_id)
def test_the_model_is_the_oracle_and_the_wrong_rules_are_not(ok, case):
    """Per batch, the growth of the oracle's n_unique_kmers() is the model's number of new k-mers -- with bands, with a mask, on top of
    counted reads -- and every wrong rule the case claims gives another figure.
    Measured at k = 21: Counttable mid16 true (1074, 92, 17), table0 (92, 7, 1), all (0, 0, 0), noprior (3786, 3507, 3671), nobatch
    (2786, 196, 33), wrongbin (1071, 97, 16); straddle true (3712, 2151, 1763), table0 (3365, 1869, 1514), noprior (4135, 3689, 3934),
    wrongbin (3711, 2151, 1763); tiny4 true (18, 12, 9) of (26, 18, 10) distinct k-mers."""
    want = ft.oracle_tracked(ok, case)
    true = ft.model_tracked(ok, case)
    assert true == want.new
    assert sum(want.consumed) > 0
    for rule in case.catches:
        assert ft.model_tracked(ok, case, rule) != want.new, rule
    if case.catches:
        # neither everything nor nothing is new: a rule that ignores the tables, or one that finds them full, shows
        distinct = ft.distinct_in_batches(ok, case)
        assert any(0 < n < d for n, d in zip(true, distinct)), (true, distinct)
        assert {'noprior', 'nobatch'} <= set(case.catches)          # every case with counted reads before it and repeats in it


def test_every_wrong_rule_is_caught_on_either_side_of_2_pow_16():
    for rule in ft.RULES:
        assert any(rule in c.catches and c.geometry in ft.BELOW_2_16 for c in ft.CASES), rule
        assert any(rule in c.catches and c.geometry in ft.ABOVE_2_16 for c in ft.CASES), rule
    # every kind, every k and every option meets a case that catches something
    for kind in ft.KINDS:
        assert {c.k for c in ft.CASES if c.kind == kind and c.catches} == set(ft.ks_of(kind))
    assert all(c.catches for c in ft.CASES if c.mask or c.nbands or c.reads in ('edge', 'uniform'))


@pytest.mark.parametrize('d', ft.DIST_CASES, ids=ft.dist_id)
def test_the_model_is_the_oracle_for_the_abundance_distribution(ok, d):
    """histograms of both calls and the tracking tables at the end; the saturated entry holds k-mers.
    Measured: 7626 and 1946 new k-mers in the two calls over straddle at k = 21, hist[255] = 3; 2129 and 60 over mid16 at k = 33 with
    nibble counts, hist[15] = 2; 167 and 0 with tracking on tiny4 (the tables fill up during the first call)"""
    want = ft.oracle_dist(ok, d)
    hists, seen = ft.model_dist(ok, d)
    assert hists == want.hists
    sizes = ft.geometry(ok, d.tracking_geometry)
    for t, size in enumerate(sizes):
        assert ft.nonzero_bins(d.tracking, want.states[-1][0][t], size) == seen[t], t
    assert sum(want.hists[0]) > 0 and want.states[0] != want.prior_state
    assert all(sum(h[256:]) == 0 for h in want.hists)
    if d.top:
        assert want.hists[0][ft.TOP[d.counts]] > 0
    if d.tracking_geometry != 'tiny4':
        assert sum(want.hists[1]) > 0 and want.states[1] != want.states[0]
    for rule in d.catches:
        assert ft.model_dist(ok, d, rule)[0] != want.hists, rule
    assert 'noprior' in d.catches


def test_the_histogram_cases_cover_the_storages_and_saturate(ok):
    pairs = {(d.counts, d.tracking) for d in ft.DIST_CASES}
    assert pairs >= {('Counttable', 'Nodetable'), ('SmallCounttable', 'Nodetable'), ('Counttable', 'Counttable'), ('Counttable', 'SmallCounttable')}
    assert any(d.counts in ft.GRAPH_KINDS and d.tracking in ft.GRAPH_KINDS for d in ft.DIST_CASES)
    assert any(d.counts_geometry != d.tracking_geometry for d in ft.DIST_CASES)
    assert any(d.top and d.counts == 'Counttable' for d in ft.DIST_CASES) and any(d.top and d.counts == 'SmallCounttable' for d in ft.DIST_CASES)
    for n in (2, 4):
        parts = ft.dist_splits(ft.MAIN, 21, n)
        assert len(parts) == n and [r for part in parts for r in part if len(r) >= 21] == [r for r in ft.MAIN if len(r) >= 21]
    parts = ft.dist_splits(ft.MAIN, 21, 4)
    assert parts[1] == [] and parts[2] and all(len(r) < 21 for r in parts[2])


@pytest.mark.parametrize('case', [c for c in ft.CASES if c.reads == 'edge'], ids=ft.case_id)
def test_the_boundary_batch_is_what_it_says(ok, case):
    """an empty batch, a batch without k-mers, a batch of one k-mer, and a batch of a multiple of 32 k-mers whose first and last are new"""
    batches, _ = ft.batches_of(case)
    k = case.k
    assert batches[0] == [] and batches[1] and all(len(r) < k for r in batches[1])
    assert len(batches[2]) == 1 and len(batches[2][0]) == k
    total = sum(len(r) - k + 1 for r in batches[3] if len(r) >= k)
    assert total % 32 == 0 and total > 64                           # (6816 k-mers at k = 21, 2144 at k = 51)
    new = ft.model_ordinals(ok, case)
    assert new[0] == [] and new[1] == [] and new[2] == [0]
    assert new[3][0] == 0 and new[3][-1] == total - 1               # bit 0 of word 0, bit 31 of the last word
    assert 2 < len(new[3]) < total
    assert ft.oracle_tracked(ok, case).consumed[:3] == (0, 0, 1)


def test_the_last_bin_of_a_table_of_every_storage_is_hit(ok):
    """after the counts, read from table_bytes: a kernel that dropped the last bin (or the odd nibble) of a table would show"""
    seen = set()
    for case in ft.CASES:
        sizes = ft.geometry(ok, case.geometry)
        tables = ft.oracle_tracked(ok, case).state[0]
        if all(ft.nonzero_bins(case.kind, raw, size)[size - 1] for raw, size in zip(tables, sizes)):
            storage = 'byte' if case.kind in ('Counttable', 'Countgraph') else ('nibble' if case.kind == 'SmallCounttable' else 'bit')
            seen |= {(storage, size % 2) for size in sizes}
    assert seen >= {('byte', 1), ('nibble', 1), ('nibble', 0), ('bit', 1)}


@pytest.mark.parametrize('case', ft.EXACT_CASES, ids=ft.case_id)
def test_the_whole_sample_figure_is_the_sum_over_batches_of_a_fresh_sketch(ok, case):
    """what kv_unique_exact must return whatever the sketch holds: n_unique_kmers() of a fresh sketch, which `noprior` over one call of
    all batches gives and the true rule on top of counted reads does not"""
    want = ft.oracle_exact(ok, case)
    fresh = case._replace(variant='cleared')
    assert want == sum(ft.model_tracked(ok, fresh)) > 0
    assert want != sum(ft.oracle_tracked(ok, case).new)             # on top of PRIOR fewer k-mers are new
