"""Host-side checks of `kevlar simlike`.  The yardstick first: the plain-Python restatement of the reference's scoring loops
(tests/simlike_common.py), run on the oracle's sketches, gives what the reference's own test_simlike.py states for every one of
its cases (tests/golden/simlike/recorded.json).  Then the product's host half -- kevlar_amd.simlike.simlike and main -- against the
same expectations, with the device batch answered by the restatement and the sketches loaded by the oracle.  Last, the generators
of the device test: every edge they promise occurs in the jobs they make.  No kernel is launched here."""
import os

import numpy as np
import pytest

import simlike_common as sc
from conftest import SIMLIKE_ALT, SIMLIKE_REF, simlike_minitrio


@pytest.fixture(scope='module')
def rec():
    return sc.recorded()


@pytest.fixture(scope='module')
def kevlar():
    import __graft_entry__
    __graft_entry__.build()
    import kevlar_amd
    import kevlar_amd.simlike  # noqa: F401
    return kevlar_amd


@pytest.fixture(scope='module', autouse=True)
def layout(kevlar):
    """the restatement writes the record the product reads"""
    product_layout = kevlar.simlike
    assert (product_layout.RECORD_WORDS, product_layout.MAX_SAMPLES) == (sc.RECORD_WORDS, sc.MAX_SAMPLES)
    assert (product_layout.REC_NREFR, product_layout.REC_DROPPED, product_layout.REC_FLAGS, product_layout.REC_NKMERS) == \
        (sc.REC_NREFR, sc.REC_DROPPED, sc.REC_FLAGS, sc.REC_NKMERS)
    assert (product_layout.FLAG_PASSENGER, product_layout.FLAG_CASE_ABUND, product_layout.FLAG_CTRL_ABUND, product_layout.FLAG_MISMATCH,
            product_layout.FLAG_NO_REFR) == (sc.PASSENGER, sc.CASE_ABUND, sc.CTRL_ABUND, sc.MISMATCH, sc.NO_REFR)


@pytest.fixture(scope='module')
def minitrio(ok):
    return simlike_minitrio(ok)


@pytest.fixture(scope='module')
def trios(ok):
    cache = {}
    return lambda name: cache.setdefault(name, sc.fixture_trio(ok, name))


def restated(kevlar):
    """the reference's way through a list of calls"""
    return lambda variants, case, controls, refr, **kwargs: sc.restate_simlike(list(variants), case, controls, refr, **kwargs)


def product(kevlar, monkeypatch):
    """kevlar_amd.simlike.simlike with its device batch answered by the restatement"""
    monkeypatch.setattr(kevlar.simlike, 'score_batch', sc.restated_score_batch)
    return lambda variants, case, controls, refr, **kwargs: list(kevlar.simlike.simlike(variants, case, controls, refr, **kwargs))


@pytest.fixture(params=['restatement', 'product'])
def scorer(request, kevlar, monkeypatch):
    return restated(kevlar) if request.param == 'restatement' else product(kevlar, monkeypatch)


# ---- the model's numbers -----------------------------------------------------------------------------------------------------------
def test_abund_log_prob_table(rec):
    """kevlar/tests/test_simlike.py:109-128"""
    assert len(rec['abund_log_prob']) == 17
    for genotype, abundance, kwargs, value in rec['abund_log_prob']:
        assert sc.abund_log_prob(genotype, abundance, **kwargs) == pytest.approx(value)


def test_minitrio_likelihoods(rec, minitrio):
    """kevlar/tests/test_simlike.py:131-143"""
    kid, mom, dad, ref = minitrio
    lists, refrabunds, ndropped = sc.spanning(SIMLIKE_ALT, SIMLIKE_REF, kid, (mom, dad), ref)
    assert ndropped == rec['minitrio']['ndropped']
    assert sc.likelihood_denovo(lists, refrabunds) == pytest.approx(rec['minitrio']['LLDN'])
    assert sc.likelihood_false(lists, refrabunds) == pytest.approx(rec['minitrio']['LLFP'])
    assert sc.likelihood_inherited(lists) == pytest.approx(rec['minitrio']['LLIH'])
    record, likelihoods, _, _ = sc.restate_call(SIMLIKE_ALT, SIMLIKE_REF, kid, (mom, dad), ref)
    assert likelihoods[0] - max(likelihoods[1:]) == pytest.approx(213.796, abs=1e-3)
    assert record[:3] == [28, 28, 28] and record[sc.REC_NREFR:] == [28, 3, 0, 31]


def test_joinlist_and_labels(kevlar):
    """kevlar/tests/test_simlike.py:146-148"""
    assert kevlar.simlike.joinlist([1, 2, 3, 4, 5]) == '1,2,3,4,5'
    assert kevlar.simlike.joinlist([]) == '.'
    assert kevlar.simlike.default_sample_labels(3) == ['Case', 'Control1', 'Control2']
    assert issubclass(kevlar.simlike.KevlarSampleLabelingError, ValueError)


# ---- the reference's cases, through the restatement and through the product's host half ------------------------------------------
def test_bad_windows(rec, scorer, minitrio, kevlar, kevlar_log, request):
    """kevlar/tests/test_simlike.py:151-171"""
    kid, mom, dad, ref = minitrio
    want, log = rec['badwindows'], []
    kwargs = dict(log=log) if 'restatement' in request.node.name else {}
    calls = scorer(sc.read_calls('minitrio/calls-badwindows.vcf'), kid, (mom, dad), ref, samplelabels=('Kid', 'Mom', 'Dad'), **kwargs)
    assert len(calls) == want['ncalls']
    good = [call for call in calls if call.attribute('LIKESCORE') > float('-inf')]
    assert len(good) == want['ngood']
    assert (len(good[0].window), len(good[0].refrwindow)) == (want['window'], want['refrwindow'])
    text = '\n'.join(log) if kwargs else kevlar_log.getvalue()
    for line in want['log']:
        assert line in text
    if not kwargs:
        assert text.count('WARNING: stubbornly refusing to compute likelihood:') == 4


def test_minitrio_call(rec, scorer, minitrio):
    """kevlar/tests/test_simlike.py:174-197"""
    kid, mom, dad, ref = minitrio
    calls = scorer(sc.read_calls('minitrio/calls.vcf'), kid, (mom, dad), ref, samplelabels=('Kid', 'Mom', 'Dad'))
    assert len(calls) == rec['minitrio']['ncalls']
    assert float(calls[0].attribute('LLDN')) == pytest.approx(rec['minitrio']['LLDN'])
    assert calls[0].format('Kid', 'ALTABUND') == rec['minitrio']['kid_altabund']
    assert calls[0].attribute('DROPPED') == 3 and calls[0].filterstr == 'PASS'
    calls = scorer(sc.read_calls('minitrio/calls.vcf'), kid, (mom, dad), ref)
    assert set(calls[0]._sample_data) == set(rec['minitrio']['default_labels'])


def test_fastmode(rec, scorer, trios):
    """kevlar/tests/test_simlike.py:250-270"""
    kid, mom, dad, refr = trios('simlike-fast-mode')
    want = rec['fastmode']
    calls = scorer(sc.read_calls('simlike-fast-mode/cc27.calls.vcf'), kid, [mom, dad], refr, fastmode=True, samplelabels=want['labels'])
    assert len(calls) == want['ncalls']
    assert [call.format('Proband', 'ALTABUND') for call in calls] == want['proband_altabund']
    assert [call.filterstr for call in calls] == want['filters']


@pytest.mark.parametrize('case', range(10))
def test_ctrl_high_abund(case, rec, scorer, trios):
    """kevlar/tests/test_simlike.py:273-297"""
    threshold, status = rec['ctrl_high_abund']['cases'][case]
    kid, mom, dad, refr = trios('ctrl-high-abund')
    calls = scorer(sc.read_calls('ctrl-high-abund/cc57120.calls.vcf'), kid, [mom, dad], refr, samplelabels=['Kid', 'Mom', 'Dad'],
                   ctrlabundhigh=threshold)
    assert len(calls) == rec['ctrl_high_abund']['ncalls']
    for call in calls:
        assert ('ControlAbundance' in call.filterstr) is status


@pytest.mark.parametrize('case', range(10))
def test_case_low_abund(case, rec, scorer, trios):
    """kevlar/tests/test_simlike.py:300-324"""
    casemin, abund, numfilt = rec['case_low_abund']['cases'][case]
    kid, mom, dad, refr = trios('case-low-abund')
    calls = scorer(sc.read_calls('case-low-abund/calls.vcf.gz'), kid, [mom, dad], refr, samplelabels=['Kid', 'Mom', 'Dad'], casemin=casemin,
                   caseabundlow=abund)
    assert len(calls) == rec['case_low_abund']['ncalls']
    assert len([call for call in calls if 'CaseAbundance' in call.filterstr]) == numfilt


def test_min_like_score(rec, scorer, trios):
    """kevlar/tests/test_simlike.py:327-351"""
    kid, mom, dad, refr = trios('ctrl-high-abund')
    for minlikescore, npass, nfail in rec['min_like_score']['cases']:
        calls = scorer(sc.read_calls('ctrl-high-abund/cc57120.calls.vcf'), kid, [mom, dad], refr, samplelabels=['Kid', 'Mom', 'Dad'],
                       minlikescore=minlikescore, **rec['min_like_score']['params'])
        assert len([call for call in calls if call.filterstr == 'PASS']) == npass
        assert len([call for call in calls if call.filterstr != 'PASS']) == nfail


@pytest.mark.parametrize('case', range(2))
def test_drop_outliers(case, rec, scorer, trios):
    """kevlar/tests/test_simlike.py:354-368"""
    dodrop, filterstr = rec['term_high_abund']['drop_outliers'][case]
    kid, mom, dad, refr = trios('term-high-abund')
    calls = scorer(sc.read_calls('term-high-abund/calls.vcf'), kid, [mom, dad], refr, dropoutliers=dodrop, ambigthresh=0,
                   **rec['term_high_abund']['params'])
    assert len(calls) > 0
    for call in calls:
        assert call.filterstr == filterstr


@pytest.mark.parametrize('case', range(5))
def test_ambig_threshold(case, rec, scorer, trios):
    """kevlar/tests/test_simlike.py:371-390"""
    ambigthresh, filterstr = rec['term_high_abund']['ambig'][case]
    kid, mom, dad, refr = trios('term-high-abund')
    calls = scorer(sc.read_calls('term-high-abund/calls.vcf'), kid, [mom, dad], refr, dropoutliers=True, ambigthresh=ambigthresh,
                   **rec['term_high_abund']['params'])
    tested = [call for call in calls if call.attribute('PART') == rec['term_high_abund']['ambig_part']]
    assert len(tested) > 10
    for call in tested:
        assert call.filterstr == filterstr


@pytest.mark.parametrize('partid', ['1085', '1187', '784'])
def test_partscore(partid, rec, scorer, trios):
    """kevlar/tests/test_simlike.py:393-407"""
    assert partid in rec['partscore']['parts']
    kid, mom, dad, refr = trios('partscore')
    calls = scorer(sc.read_calls('partscore/partscore-cc{}.calls.vcf.gz'.format(partid)), kid, [mom, dad], refr, **rec['partscore']['params'])
    assert len(calls) > 0
    for call in calls:
        assert call.filterstr == rec['partscore']['filter']


def test_output_order_and_partitions(kevlar, monkeypatch, trios):
    """best score first, equal scores in the order they came; partitions in the order first seen"""
    kid, mom, dad, refr = trios('term-high-abund')
    kwargs = dict(mu=30.0, sigma=10.0, casemin=5, ctrlmax=1, dropoutliers=True, ambigthresh=0)
    want = sc.restate_simlike(sc.read_calls('term-high-abund/calls.vcf'), kid, [mom, dad], refr, **kwargs)
    got = product(kevlar, monkeypatch)(sc.read_calls('term-high-abund/calls.vcf'), kid, [mom, dad], refr, **kwargs)
    assert [call.vcf for call in got] == [call.vcf for call in want]
    scores = [call.attribute('LIKESCORE') for call in got]
    assert scores == sorted(scores, reverse=True) and len(scores) > 10


def test_mismatch_raises_with_the_two_lengths(kevlar, monkeypatch, ok):
    job = [job for job in sc.edge_jobs(31, with_n=False) if job['label'] == 'outlier-mismatch']
    case, controls, refr = sc.planted_sketches(ok, 31, job)
    from kevlar_amd.vcf import Variant
    call = Variant('chr1', 100, 'A', 'C', ALTWINDOW=job[0]['alt'], REFRWINDOW=job[0]['ref'], PART='1')
    with pytest.raises(AssertionError) as failure:
        product(kevlar, monkeypatch)([call], case, controls, refr, dropoutliers=True)
    assert failure.value.args[0] == (65, 66)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_defaults(kevlar):
    args = kevlar.simlike.parser().parse_args(['--case', 'kid.ct', '--controls', 'mom.ct', 'dad.ct', '--refr', 'refr.sct', 'a.vcf', 'b.vcf'])
    assert vars(args) == dict(case='kid.ct', controls=['mom.ct', 'dad.ct'], refr='refr.sct', ctrl_max=1, case_min=6, mu=30.0, sigma=8.0,
                              epsilon=0.001, ctrl_abund_high=4, case_abund_low=5, min_like_score=0.0, drop_outliers=False, ambig_thresh=10,
                              sample_labels=None, fast_mode=False, out='-', vcf=['a.vcf', 'b.vcf'])
    metavars = {action.dest: action.metavar for action in kevlar.simlike.parser()._actions}
    assert [metavars[dest] for dest in ('case', 'controls', 'refr', 'ctrl_max', 'case_min', 'mu', 'sigma', 'epsilon', 'ctrl_abund_high',
                                        'case_abund_low', 'min_like_score', 'ambig_thresh', 'sample_labels', 'out')] == \
        ['CT', 'CT', 'REFR', 'X', 'Y', 'μ', 'σ', 'ε', 'H', 'L', 'S', 'A', 'LBL', 'OUT']
    short = kevlar.simlike.parser().parse_args(['--case', 'k', '--controls', 'm', '--refr', 'r', '-f', '-o', 'out.vcf', 'a.vcf'])
    assert short.fast_mode is True and short.out == 'out.vcf'


@pytest.mark.parametrize('case', range(2))
def test_cli(case, rec, kevlar, monkeypatch, minitrio, tmp_path, capsys):
    """kevlar/tests/test_simlike.py:200-234: the sketches saved, named on the command line and loaded again"""
    fmtstr, sampleargs = rec['minitrio']['cli'][case]
    paths = [str(tmp_path / name) for name in ('kid.ct', 'mom.ct', 'dad.ct', 'refr.sct')]
    for sketch, path in zip(minitrio, paths):
        sketch.save(path)
    from oracle import okhmer
    monkeypatch.setattr(kevlar.sketch, 'load', lambda path: sc.load_sketch(okhmer, path))
    monkeypatch.setattr(kevlar.simlike, 'score_batch', sc.restated_score_batch)
    args = kevlar.simlike.parser().parse_args(['--case', paths[0], '--controls', paths[1], paths[2]] + sampleargs +
                                              ['--refr', paths[3], sc.golden('minitrio/calls.vcf')])
    kevlar.simlike.main(args)
    out, err = capsys.readouterr()
    assert fmtstr in out
    assert '##source=kevlar::simlike\n' in out
    for text in rec['minitrio']['cli_text']:
        assert text in out
    assert out.count('\n') - sum(1 for line in out.split('\n') if line.startswith('#')) == 1


def test_cli_to_a_file(rec, kevlar, monkeypatch, minitrio, tmp_path):
    loaded = dict(zip(('kid.ct', 'mom.ct', 'dad.ct', 'refr.sct'), minitrio))
    monkeypatch.setattr(kevlar.sketch, 'load', lambda path: loaded[path])
    monkeypatch.setattr(kevlar.simlike, 'score_batch', sc.restated_score_batch)
    out = str(tmp_path / 'scored.vcf')
    kevlar.simlike.main(kevlar.simlike.parser().parse_args(['--case', 'kid.ct', '--controls', 'mom.ct', 'dad.ct', '--refr', 'refr.sct',
                                                          '-o', out, sc.golden('minitrio/calls.vcf')]))
    text = open(out).read()
    assert 'LIKESCORE=213.796' in text and text.endswith('\n')


def test_cli_bad_labels(rec, kevlar):
    """kevlar/tests/test_simlike.py:237-247"""
    want = rec['minitrio']['bad_labels']
    args = kevlar.simlike.parser().parse_args(['--case', 'kid.ct', '--controls', 'mom.ct', 'dad.ct', '--sample-labels'] + want['labels'] +
                                              ['--refr', 'refr.sct', sc.golden('minitrio/calls.vcf')])
    with pytest.raises(kevlar.simlike.KevlarSampleLabelingError, match=want['error']):
        kevlar.simlike.main(args)


def test_module_runs_as_a_command():
    source = open(os.path.join(os.path.dirname(sc.HERE), 'kevlar_amd', 'simlike.py')).read()
    assert "if __name__ == '__main__':\n    main(parser().parse_args())" in source


# ---- score_batch's host side -------------------------------------------------------------------------------------------------------
def test_scored_lists_read_the_layout(kevlar, minitrio):
    kid, mom, dad, ref = minitrio
    windows, refrwindows = [SIMLIKE_ALT, SIMLIKE_ALT[:40], SIMLIKE_ALT], [SIMLIKE_REF, SIMLIKE_REF[:45], SIMLIKE_REF]
    scored = sc.restated_score_batch(windows, refrwindows, kid, (mom, dad), ref)
    for c in range(3):
        lists, refrabunds = kevlar.simlike.scored_lists(scored, c)
        want = sc.spanning(windows[c], refrwindows[c], kid, (mom, dad), ref)
        assert (lists, refrabunds) == (want[0], want[1])
    assert scored.kbase.tolist() == [0, 31, 41, 72]
    assert kevlar.simlike._off(None) == kevlar.simlike._off(False) == kevlar.simlike._off(-3) == kevlar.simlike._off(0) == 0
    assert kevlar.simlike._off(5) == 5


# ---- the generators of the device test ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def edges(ok):
    jobs = sc.edge_jobs(31)
    case, controls, refr = sc.planted_sketches(ok, 31, jobs)
    plain = {job['label']: sc.restate_call(job['alt'], job['ref'], case, controls, refr) for job in jobs}
    drop = {job['label']: sc.restate_call(job['alt'], job['ref'], case, controls, refr, dropoutliers=True) for job in jobs}
    return jobs, plain, drop


def test_edge_jobs_have_the_promised_shapes(edges):
    jobs, plain, drop = edges
    by_label = {job['label']: job for job in jobs}
    assert len(by_label) == len(jobs)
    for nk in (1, 63, 64, 65, 128, 129):
        for label in ('snv-{}', 'indel-{}', 'snv-{}-kept'):
            assert plain[label.format(nk)][0][sc.REC_NKMERS] == nk
        assert plain['snv-{}-kept'.format(nk)][0][0] == nk
        assert plain['indel-{}'.format(nk)][0][sc.REC_FLAGS] & sc.NO_REFR and not plain['snv-{}'.format(nk)][0][sc.REC_FLAGS] & sc.NO_REFR
    assert 0 < plain['snv-129'][0][0] < 129                                     # some dropped, some kept
    assert (len(by_label['long-refr']['alt']), len(by_label['long-refr']['ref'])) == (61, 5000)
    assert plain['all-dropped'][0][0] == 0 and plain['all-dropped'][0][sc.REC_DROPPED] == 40
    assert plain['all-dropped'][0][sc.REC_FLAGS] & sc.PASSENGER
    assert plain['none-dropped'][0][sc.REC_DROPPED] == 0
    assert max(plain['at-255'][2][0]) == 255 and max(plain['at-255'][2][1]) == 255
    assert min(plain['clamped'][2][1]) > 30.0 * max(plain['clamped'][3])       # every count above mu * r
    assert 0 in plain['refr-count-0'][3] and max(plain['refr-count-0'][3]) > 0
    assert 'N' in by_label['n-and-lower-case']['alt'] and by_label['n-and-lower-case']['alt'] != by_label['n-and-lower-case']['alt'].upper()


def test_edge_jobs_trip_the_filters_at_their_thresholds(edges):
    jobs, plain, drop = edges
    flagged = lambda label, bit: bool(plain[label][0][sc.REC_FLAGS] & bit)   # noqa: E731
    for where in ('inside', 'across'):
        assert [flagged('lowrun-{}-{}'.format(length, where), sc.CASE_ABUND) for length in (4, 5, 6)] == [False, True, True]
    lows = [i for i, a in enumerate(plain['lowrun-5-across'][2][0]) if a < 6]
    assert lows[0] < 64 <= lows[-1]                                             # the run lies across the chunk edge
    assert not flagged('lowrun-two-short', sc.CASE_ABUND)
    assert [flagged('ctrlhigh-{}'.format(high), sc.CTRL_ABUND) for high in (4, 5)] == [False, True]
    highs = [i for i, a in enumerate(plain['ctrlhigh-5'][2][2]) if a > 1]
    assert len(highs) == 5 and highs[2] < 64 <= highs[3]


def test_edge_jobs_drop_the_outliers_they_plant(edges):
    jobs, plain, drop = edges
    for where in ('first', 'middle', 'last'):
        label = 'outlier-case-' + where
        assert (plain[label][0][0], drop[label][0][0]) == (140, 139)
        assert 60 in plain[label][2][0] and 60 not in drop[label][2][0]
        assert not drop[label][0][sc.REC_FLAGS] & sc.MISMATCH and drop[label][0][sc.REC_DROPPED] == 1
    assert (plain['outlier-empties'][0][0], drop['outlier-empties'][0][0]) == (2, 0)
    assert drop['outlier-empties'][0][sc.REC_FLAGS] & sc.PASSENGER and drop['outlier-empties'][1] is not None
    for label, lengths in (('outlier-mismatch', [66, 65, 66, 66]), ('outlier-mismatch-indel', [66, 66, 65, 66])):
        assert not plain[label][0][sc.REC_FLAGS] & sc.MISMATCH
        assert drop[label][0][sc.REC_FLAGS] & sc.MISMATCH and drop[label][1] is None
        assert drop[label][0][:3] + [drop[label][0][sc.REC_NREFR]] == lengths
    # nothing but the planted outliers goes: every other job keeps its lists
    for job in jobs:
        if not job['label'].startswith('outlier') and job['label'] not in ('at-255', 'clamped'):
            assert plain[job['label']][0][:3] == drop[job['label']][0][:3], job['label']


def test_seeded_jobs_are_300_mixed_calls(ok):
    jobs = sc.seeded_jobs()
    assert len(jobs) == 300
    assert sum(len(job['alt']) != len(job['ref']) for job in jobs) == 100
    assert {len(job['alt']) - 30 for job in jobs} == {1, 5, 31, 65, 70, 130}
    case, controls, refr = sc.planted_sketches(ok, 31, jobs[:40])
    flags = [sc.restate_call(job['alt'], job['ref'], case, controls, refr)[0][sc.REC_FLAGS] for job in jobs[:40]]
    for bit in (sc.CASE_ABUND, sc.CTRL_ABUND, sc.NO_REFR):
        assert any(flag & bit for flag in flags) and not all(flag & bit for flag in flags)


def test_restated_batch_equals_restated_calls(ok):
    jobs = sc.edge_jobs(13, with_n=False)[:8]
    case, controls, refr = sc.planted_sketches(ok, 13, jobs, refr_kind='Countgraph')
    got = sc.Scored([job['alt'] for job in jobs], [job['ref'] for job in jobs], case, controls, refr)
    assert got.records.shape == (8, 20) and got.likelihoods.shape == (8, 3)
    assert np.all(got.records[:, sc.REC_NKMERS] == np.diff(got.kbase))
