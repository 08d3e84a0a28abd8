"""`kevlar simlike` on the device (kevlar_amd/csrc/kv_simlike.hip through kevlar_amd.simlike): the fused batch against the
plain-Python restatement of tests/simlike_common.py fed by get_kmer_counts of the same device sketches (the per-window path the
oracle tests hold), call for call -- every integer equal, the three doubles within rel = abs = 1e-9 -- and the reference's
fixtures end to end against what its own tests state (tests/golden/simlike/recorded.json)."""
import ctypes

import numpy as np
import pytest

import kevlar_amd.simlike as simlike
from kevlar_amd import _lib

import simlike_common as sc
from conftest import simlike_minitrio

pytestmark = pytest.mark.gpu
TOLERANCE = 1e-9                # rel and abs: both sides are IEEE double and differ in summation order and in lgamma / log alone
PARAM_SETS = (dict(), dict(dropoutliers=True), dict(mu=30.5, sigma=7.3, epsilon=0.004, casemin=5, ctrlmax=2))
worst = {'abs': 0.0, 'rel': 0.0}


@pytest.fixture(scope='module', autouse=True)
def device(hk):
    assert (simlike.RECORD_WORDS, simlike.MAX_SAMPLES) == (sc.RECORD_WORDS, sc.MAX_SAMPLES)
    assert (simlike.FLAG_PASSENGER, simlike.FLAG_CASE_ABUND, simlike.FLAG_CTRL_ABUND, simlike.FLAG_MISMATCH, simlike.FLAG_NO_REFR) == \
        (sc.PASSENGER, sc.CASE_ABUND, sc.CTRL_ABUND, sc.MISMATCH, sc.NO_REFR)
    yield hk
    print('largest deviation of a likelihood from the restatement: abs {abs:.3e}, rel {rel:.3e}'.format(**worst))


@pytest.fixture(scope='module')
def rec():
    return sc.recorded()


class Memo(object):
    """a device sketch that answers a window it has seen from memory (the restatement asks again for every parameter set)"""

    def __init__(self, sketch):
        self.sketch, self.seen = sketch, {}

    def ksize(self):
        return self.sketch.ksize()

    def get_kmer_counts(self, seq):
        if seq not in self.seen:
            self.seen[seq] = self.sketch.get_kmer_counts(seq)
        return self.seen[seq]


def same(got, want):
    """a Scored of the device against one of the restatement"""
    assert got.kbase.tolist() == want.kbase.tolist()
    assert got.records.tolist() == want.records.tolist()
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.refr, want.refr)
    for c in range(len(want.records)):
        for found, expected in zip(got.likelihoods[c], want.likelihoods[c]):
            assert np.isfinite(found)
            worst['abs'] = max(worst['abs'], abs(found - expected))
            worst['rel'] = max(worst['rel'], abs(found - expected) / abs(expected) if expected else 0.0)
            assert found == pytest.approx(expected, rel=TOLERANCE, abs=TOLERANCE), (c, got.likelihoods[c], want.likelihoods[c])


def agree(jobs, case, controls, refr, memo=None, **params):
    windows, refrwindows = [job['alt'] for job in jobs], [job['ref'] for job in jobs]
    got = simlike.score_batch(windows, refrwindows, case, controls, refr, **params)
    memo = memo or [Memo(sketch) for sketch in [case] + list(controls) + [refr]]
    same(got, sc.Scored(windows, refrwindows, memo[0], memo[1:-1], memo[-1], **params))
    return got, memo


# ---- 1. shapes and count patterns -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,refr_kind', [(13, 'Countgraph'), (31, 'SmallCounttable'), (31, 'Counttable'), (31, 'Nodetable'),
                                         (31, 'Countgraph'), (32, 'Countgraph'), (32, 'SmallCounttable'), (33, 'Counttable'),
                                         (51, 'Nodetable'), (128, 'SmallCounttable')])
def test_edges_agree_with_the_restatement(k, refr_kind, hk):
    jobs = sc.edge_jobs(k)
    case, controls, refr = sc.planted_sketches(hk, k, jobs, refr_kind=refr_kind)
    memo = None
    for params in PARAM_SETS:
        got, memo = agree(jobs, case, controls, refr, memo=memo, **params)
        flags = dict(zip([job['label'] for job in jobs], got.records[:, sc.REC_FLAGS].tolist()))
        assert bool(flags['outlier-mismatch'] & sc.MISMATCH) == bool(params.get('dropoutliers'))
    assert any(len(job['ref']) == 5000 for job in jobs)


@pytest.mark.parametrize('nctrl', [2, 3, 15])
def test_two_three_and_fifteen_controls(nctrl, hk):
    jobs = sc.edge_jobs(31, seed=nctrl, nctrl=nctrl)
    case, controls, refr = sc.planted_sketches(hk, 31, jobs, nctrl=nctrl)
    memo = None
    for params in PARAM_SETS[:2]:
        got, memo = agree(jobs, case, controls, refr, memo=memo, **params)
    assert got.nsamples == nctrl + 1 and np.all(got.records[:, nctrl + 1:sc.MAX_SAMPLES] == 0)


def test_samples_of_every_kind_and_both_hash_families(hk):
    """a two-bit case beside murmur controls and a murmur genome: every k-mer is hashed once per family"""
    jobs = sc.edge_jobs(21, seed=5, nctrl=5)
    kinds = ['Countgraph', 'SmallCounttable', 'SmallCountgraph', 'Nodetable', 'Nodegraph', 'Counttable']
    case, controls, refr = sc.planted_sketches(hk, 21, jobs, nctrl=5, sample_kinds=kinds)
    memo = None
    for params in PARAM_SETS[:2]:
        got, memo = agree(jobs, case, controls, refr, memo=memo, **params)


# ---- 2. batches -------------------------------------------------------------------------------------------------------------------
def test_300_calls_in_one_batch_in_sevens_and_one_at_a_time(hk):
    jobs = sc.seeded_jobs()
    case, controls, refr = sc.planted_sketches(hk, 31, jobs)
    whole, memo = agree(jobs, case, controls, refr, dropoutliers=True)
    windows, refrwindows = [job['alt'] for job in jobs], [job['ref'] for job in jobs]
    for step in (7, 1):
        for first in range(0, len(jobs), step):
            part = simlike.score_batch(windows[first:first + step], refrwindows[first:first + step], case, controls, refr, dropoutliers=True)
            assert part.records.tolist() == whole.records[first:first + step].tolist()
            assert part.likelihoods.tolist() == whole.likelihoods[first:first + step].tolist()
            for c in range(len(part.records)):
                assert simlike.scored_lists(part, c) == simlike.scored_lists(whole, first + c)
    # the same cut by window bytes inside score_batch, the parts joined
    joined = simlike.score_batch(windows, refrwindows, case, controls, refr, dropoutliers=True, batch_bytes=1000)
    for field in ('records', 'likelihoods', 'counts', 'refr', 'kbase'):
        assert np.array_equal(getattr(joined, field), getattr(whole, field)), field
    empty = simlike.score_batch([], [], case, controls, refr)
    assert empty.records.shape == (0, sc.RECORD_WORDS) and empty.kbase.tolist() == [0]


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def raw_score(samples, refr, alt, ref, ksize, mu=30.0, sigma=8.0, epsilon=0.001, nsamples=None, null=()):
    """kv_simlike_score as it is, on outputs filled with 0xAB: (return code, the outputs untouched?)"""
    alt_bytes, ref_bytes = ''.join(alt).encode(), ''.join(ref).encode()
    aoff = np.cumsum([0] + [len(w) for w in alt]).astype(np.uint64)
    roff = np.cumsum([0] + [len(w) for w in ref]).astype(np.uint64)
    room = max(1, sum(len(w) for w in alt))
    outs = [np.full(len(alt) * sc.RECORD_WORDS * 4, 0xAB, dtype=np.uint8), np.full(len(alt) * 24, 0xAB, dtype=np.uint8),
            np.full(len(samples) * room, 0xAB, dtype=np.uint8), np.full(room, 0xAB, dtype=np.uint8)]
    ptr = lambda name, array: None if name in null else ctypes.c_void_p(array.ctypes.data)   # noqa: E731
    handles = (ctypes.c_void_p * len(samples))(*[s._h.value for s in samples])
    rc = _lib.load().kv_simlike_score(
        None if 'samples' in null else handles, len(samples) if nsamples is None else nsamples, None if 'refr' in null else refr._h,
        None if 'alt' in null else ctypes.cast(ctypes.c_char_p(alt_bytes), ctypes.c_void_p), ptr('aoff', aoff),
        None if 'ref' in null else ctypes.cast(ctypes.c_char_p(ref_bytes), ctypes.c_void_p), ptr('roff', roff), len(alt), ksize, mu, sigma,
        epsilon, 6, 1, 5, 4, 0, ptr('records', outs[0]), ptr('likelihoods', outs[1]), ptr('counts', outs[2]), ptr('refr_abunds', outs[3]))
    return rc, all(np.all(out == 0xAB) for out in outs)


def test_refusals_leave_the_outputs_alone(hk):
    trio = [hk.Counttable(31, 1e5, 4) for _ in range(3)]
    refr, other_k = hk.SmallCounttable(31, 1e5, 4), hk.Counttable(25, 1e5, 4)
    rng = np.random.default_rng(3)
    alt, ref = [sc.random_seq(rng, 61), sc.random_seq(rng, 40)], [sc.random_seq(rng, 61), sc.random_seq(rng, 44)]
    assert raw_score(trio, refr, alt, ref, 31) == (_lib.KV_OK, False)
    refused = (_lib.KV_ERR_ARG, True)
    for name in ('samples', 'refr', 'alt', 'aoff', 'ref', 'roff', 'records', 'likelihoods', 'counts', 'refr_abunds'):
        assert raw_score(trio, refr, alt, ref, 31, null=(name,)) == refused, name
    assert raw_score(trio[:2], refr, alt, ref, 31) == refused                                  # the model reads abunds[2]
    assert raw_score(trio * 6, refr, alt, ref, 31, nsamples=17) == refused
    assert raw_score(trio * 6, refr, alt, ref, 31, nsamples=16)[0] == _lib.KV_OK
    assert raw_score(trio[:2] + [other_k], refr, alt, ref, 31) == refused
    assert raw_score(trio, other_k, alt, ref, 31) == refused
    assert raw_score(trio, refr, alt, ref, 25) == refused
    assert raw_score(trio, refr, alt + [sc.random_seq(rng, 30)], ref + [sc.random_seq(rng, 61)], 31) == refused
    assert raw_score(trio, refr, alt + [sc.random_seq(rng, 61)], ref + [sc.random_seq(rng, 30)], 31) == refused
    for bad in (dict(epsilon=0.0), dict(epsilon=1.0), dict(epsilon=-0.1), dict(epsilon=float('nan')), dict(sigma=0.0), dict(sigma=-1.0),
                dict(sigma=float('inf')), dict(mu=-1.0), dict(mu=float('nan')), dict(mu=float('inf'))):
        assert raw_score(trio, refr, alt, ref, 31, **bad) == refused, bad
    assert raw_score(trio, refr, alt, ref, 31, mu=0.0)[0] == _lib.KV_OK
    # a graph sketch of k > 32 cannot be made, so none can reach the scorer
    with pytest.raises(ValueError, match='graph sketches need k <= 32'):
        hk.Countgraph(33, 1e5, 4)
    with pytest.raises(_lib.KvArgError, match='shorter than k'):
        simlike.score_batch([sc.random_seq(rng, 30)], [sc.random_seq(rng, 30)], trio[0], trio[1:], refr)


def test_mismatch_raises_the_reference_assertion(hk):
    from kevlar_amd.vcf import Variant
    jobs = [job for job in sc.edge_jobs(31, with_n=False) if job['label'].startswith('outlier-mismatch')]
    case, controls, refr = sc.planted_sketches(hk, 31, jobs)
    for job, lengths in zip(jobs, ((65, 66), (65, 66))):
        call = Variant('chr1', 100, 'A', 'C', ALTWINDOW=job['alt'], REFRWINDOW=job['ref'], PART='1')
        assert len(list(simlike.simlike([call], case, controls, refr))) == 1
        call = Variant('chr1', 100, 'A', 'C', ALTWINDOW=job['alt'], REFRWINDOW=job['ref'], PART='1')
        with pytest.raises(AssertionError) as failure:
            list(simlike.simlike([call], case, controls, refr, dropoutliers=True))
        assert failure.value.args[0] == lengths


# ---- 4. the reference's fixtures, end to end --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trios(hk):
    cache = {}
    return lambda name: cache.setdefault(name, sc.fixture_trio(hk, name))


def score(rel, trio, **kwargs):
    kid, mom, dad, refr = trio
    return list(simlike.simlike(sc.read_calls(rel), kid, [mom, dad], refr, **kwargs))


def test_fixture_fastmode(rec, trios):
    want = rec['fastmode']
    calls = score('simlike-fast-mode/cc27.calls.vcf', trios('simlike-fast-mode'), fastmode=True, samplelabels=want['labels'])
    assert [call.format('Proband', 'ALTABUND') for call in calls] == want['proband_altabund']
    assert [call.filterstr for call in calls] == want['filters']


def test_fixture_abundance_filters(rec, trios):
    for threshold, status in rec['ctrl_high_abund']['cases']:
        calls = score('ctrl-high-abund/cc57120.calls.vcf', trios('ctrl-high-abund'), samplelabels=['Kid', 'Mom', 'Dad'], ctrlabundhigh=threshold)
        assert len(calls) == rec['ctrl_high_abund']['ncalls']
        assert [('ControlAbundance' in call.filterstr) for call in calls] == [status] * len(calls), threshold
    for casemin, abund, numfilt in rec['case_low_abund']['cases']:
        calls = score('case-low-abund/calls.vcf.gz', trios('case-low-abund'), samplelabels=['Kid', 'Mom', 'Dad'], casemin=casemin,
                      caseabundlow=abund)
        assert len(calls) == rec['case_low_abund']['ncalls']
        assert len([call for call in calls if 'CaseAbundance' in call.filterstr]) == numfilt, (casemin, abund)
    for minlikescore, npass, nfail in rec['min_like_score']['cases']:
        calls = score('ctrl-high-abund/cc57120.calls.vcf', trios('ctrl-high-abund'), samplelabels=['Kid', 'Mom', 'Dad'],
                      minlikescore=minlikescore, **rec['min_like_score']['params'])
        assert [len([call for call in calls if call.filterstr == 'PASS']), len([call for call in calls if call.filterstr != 'PASS'])] == \
            [npass, nfail]


def test_fixture_outliers_ambiguity_and_partition_scores(rec, trios):
    want = rec['term_high_abund']
    for dodrop, filterstr in want['drop_outliers']:
        calls = score('term-high-abund/calls.vcf', trios('term-high-abund'), dropoutliers=dodrop, ambigthresh=0, **want['params'])
        assert len(calls) > 10 and {call.filterstr for call in calls} == {filterstr}
    for ambigthresh, filterstr in want['ambig']:
        calls = score('term-high-abund/calls.vcf', trios('term-high-abund'), dropoutliers=True, ambigthresh=ambigthresh, **want['params'])
        tested = [call for call in calls if call.attribute('PART') == want['ambig_part']]
        assert len(tested) > 10 and {call.filterstr for call in tested} == {filterstr}, ambigthresh
    for partid in rec['partscore']['parts']:
        calls = score('partscore/partscore-cc{}.calls.vcf.gz'.format(partid), trios('partscore'), **rec['partscore']['params'])
        assert len(calls) > 0 and {call.filterstr for call in calls} == {rec['partscore']['filter']}


def test_fixture_calls_carry_the_restatement_annotations(trios):
    """every annotation of every call of a fixture, device against restatement, as VCF text"""
    kid, mom, dad, refr = trios('term-high-abund')
    kwargs = dict(mu=30.0, sigma=10.0, casemin=5, ctrlmax=1, dropoutliers=True, ambigthresh=10)
    got = score('term-high-abund/calls.vcf', (kid, mom, dad, refr), **kwargs)
    want = sc.restate_simlike(sc.read_calls('term-high-abund/calls.vcf'), Memo(kid), [Memo(mom), Memo(dad)], Memo(refr), **kwargs)
    assert [call.vcf for call in got] == [call.vcf for call in want]
    assert [call.format('Case', 'ALTABUND') for call in got] == [call.format('Case', 'ALTABUND') for call in want]


def test_minitrio_through_main(rec, hk, kevlar_log, tmp_path, capsys):
    """kevlar/tests/test_simlike.py:151-234 with the sketches counted on the device from the reads"""
    trio = simlike_minitrio(hk)
    kid, mom, dad, ref = trio
    calls = score('minitrio/calls-badwindows.vcf', trio, samplelabels=('Kid', 'Mom', 'Dad'))
    assert len(calls) == rec['badwindows']['ncalls']
    assert len([call for call in calls if call.attribute('LIKESCORE') > float('-inf')]) == rec['badwindows']['ngood']
    for line in rec['badwindows']['log']:
        assert line in kevlar_log.getvalue()
    calls = score('minitrio/calls.vcf', trio, samplelabels=('Kid', 'Mom', 'Dad'))
    assert len(calls) == 1 and calls[0].format('Kid', 'ALTABUND') == rec['minitrio']['kid_altabund']
    for key in ('LLDN', 'LLFP', 'LLIH'):
        assert calls[0].attribute(key) == pytest.approx(rec['minitrio'][key])
    paths = [str(tmp_path / name) for name in ('kid.ct', 'mom.ct', 'dad.ct', 'refr.sct')]
    for sketch, path in zip(trio, paths):
        sketch.save(path)
    for fmtstr, sampleargs in rec['minitrio']['cli']:
        out = str(tmp_path / 'scored.vcf')
        simlike.main(simlike.parser().parse_args(['--case', paths[0], '--controls', paths[1], paths[2]] + sampleargs +
                                                 ['--refr', paths[3], '-o', out, sc.golden('minitrio/calls.vcf')]))
        text = open(out).read()
        assert fmtstr in text
        for fragment in rec['minitrio']['cli_text']:
            assert fragment in text
