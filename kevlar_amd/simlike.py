"""`kevlar simlike`: preliminary calls in, calls scored, filtered and sorted by likelihood out (the reference's kevlar/simlike.py
and kevlar/cli/simlike.py).

For the window spanning a candidate variant the model needs to know how often each of its alternate-allele k-mers was seen in
the case, in every control and in the reference genome.  The reference asks one sketch about one window at a time and does the
rest k-mer by k-mer on the host; here `score_batch` hands every call of a run to one device launch (kv_simlike_score), which
returns each call's abundance lists, filter verdicts and the three log likelihoods, and the host only annotates `Variant`
objects from the records.  The three look-up functions at the top are the earlier per-window path (khmer's get_kmer_counts =
kv_hash_kmers + kv_get_hashes here), which the device batch is tested against.

The command line is this module's: `python -m kevlar_amd.simlike --case kid.ct --controls mom.ct dad.ct --refr refr.sct
calls.vcf`, with the reference's flags; `python -m kevlar_amd simlike ...` takes the same ones (kevlar_amd.cli builds its subcommand
from parser() below)."""
import argparse
from collections import namedtuple
import ctypes
from math import isclose
import sys

import numpy as np

import kevlar_amd
from kevlar_amd.vcf import VariantFilter, VCFWriter, vcfstream


def _window_counts(sketch, sequence):
    return np.asarray(sketch.get_kmer_counts(sequence), dtype=np.int64)


def _near_mean(values, tolerance=20):
    """mask of the entries within `tolerance` of the mean of the vector"""
    return np.abs(values - values.mean()) < tolerance if len(values) else np.zeros(0, dtype=bool)


def discard_nonunique_kmers(altseq, case, controls, refr):
    """Counts of the alternate-allele k-mers that do not occur in the reference genome (those that do carry no
    signal): (case counts, [control counts ...], reference counts of ALL window k-mers)."""
    in_genome = _window_counts(refr, altseq)
    novel = in_genome == 0
    keep = lambda sketch: _window_counts(sketch, altseq)[novel].tolist()   # noqa: E731
    return keep(case), [keep(control) for control in controls], in_genome.tolist()


def discard_outlier_abunds(case_counts, ctrl_counts):
    """Drop, per sample, the counts 20 or more away from that sample's mean."""
    trim = lambda counts: np.asarray(counts, dtype=np.int64)[_near_mean(np.asarray(counts, dtype=np.float64))].tolist()   # noqa: E731
    return trim(case_counts), [trim(counts) for counts in ctrl_counts]


def spanning_kmer_abundances(altseq, refrseq, case, controls, refr, dropoutliers=False):
    """(abundances, refr_abunds, ndropped) for the k-mers spanning a variant: abundances[0] the case counts and
    abundances[1:] the control counts of the alternate-allele k-mers absent from the reference genome; refr_abunds
    the genomic frequency of the matching reference-allele k-mers (substitutions: same window length) or None per
    k-mer (indels); ndropped how many k-mers of the window were discarded."""
    nwindow = len(altseq) - case.ksize() + 1
    in_genome = _window_counts(refr, altseq)
    novel = in_genome == 0
    per_sample = [_window_counts(sketch, altseq)[novel] for sketch in [case] + list(controls)]
    if dropoutliers:
        per_sample = [counts[_near_mean(counts.astype(np.float64))] for counts in per_sample]
    kept = len(per_sample[0])
    if len(altseq) == len(refrseq):
        refr_abunds = _window_counts(refr, refrseq)[novel].tolist()
    else:
        refr_abunds = [None] * kept
    return [counts.tolist() for counts in per_sample], refr_abunds, nwindow - kept


# ---- the device batch -------------------------------------------------------------------------------------------------------
RECORD_WORDS = 20               # KV_SIMLIKE_RECORD_WORDS
MAX_SAMPLES = 16                # KV_MAX_SAMPLES
REC_NREFR, REC_DROPPED, REC_FLAGS, REC_NKMERS = MAX_SAMPLES, MAX_SAMPLES + 1, MAX_SAMPLES + 2, MAX_SAMPLES + 3
FLAG_PASSENGER, FLAG_CASE_ABUND, FLAG_CTRL_ABUND, FLAG_MISMATCH, FLAG_NO_REFR = 1, 2, 4, 8, 16
BATCH_BYTES = 256 << 20         # window bytes handed to the device at a time

# What kv_simlike_score returns for n calls of `nsamples` samples (include/kvsketch.h): records[n, RECORD_WORDS] (uint32),
# likelihoods[n, 3] = LLDN, LLFP, LLIH (float64), counts and refr (uint8, flat) and kbase[n + 1]: call c has nk = kbase[c + 1] -
# kbase[c] k-mers in its alt window, sample s's list starts at counts[nsamples * kbase[c] + s * nk], its refr list at refr[kbase[c]].
Scored = namedtuple('Scored', 'records likelihoods counts refr kbase nsamples')


def scored_lists(scored, c):
    """(abundances, refr_abunds) of call c as the reference's spanning_kmer_abundances returns them"""
    rec, base, ns = scored.records[c], int(scored.kbase[c]), scored.nsamples
    nk = int(scored.kbase[c + 1]) - base
    lists = [scored.counts[ns * base + s * nk:ns * base + s * nk + int(rec[s])].tolist() for s in range(ns)]
    nrefr = int(rec[REC_NREFR])
    refr = [None] * nrefr if rec[REC_FLAGS] & FLAG_NO_REFR else scored.refr[base:base + nrefr].tolist()
    return lists, refr


def _off(value):
    """a threshold given as None, False or anything <= 0 switches its filter off"""
    return int(value) if value and value > 0 else 0


def _score_one_batch(windows, refrwindows, handles, refr, ksize, params):
    from kevlar_amd import _lib
    n, ns = len(windows), len(handles)
    alt, ref = ''.join(windows).encode('latin-1'), ''.join(refrwindows).encode('latin-1')
    aoff = np.zeros(n + 1, dtype=np.uint64)
    roff = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(w) for w in windows], out=aoff[1:])
    np.cumsum([len(w) for w in refrwindows], out=roff[1:])
    nk = np.maximum(np.diff(aoff.astype(np.int64)) - ksize + 1, 0)
    kbase = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nk, out=kbase[1:])
    total = int(kbase[-1])
    records = np.zeros((n, RECORD_WORDS), dtype=np.uint32)
    likelihoods = np.zeros((n, 3), dtype=np.float64)
    counts = np.zeros(ns * total, dtype=np.uint8)
    refr_abunds = np.zeros(total, dtype=np.uint8)
    ptr = lambda array: ctypes.c_void_p(array.ctypes.data)   # noqa: E731
    _lib.check(_lib.load().kv_simlike_score(
        (ctypes.c_void_p * ns)(*[h.value if isinstance(h, ctypes.c_void_p) else h for h in handles]), ns, refr,
        ctypes.cast(ctypes.c_char_p(alt), ctypes.c_void_p), ptr(aoff), ctypes.cast(ctypes.c_char_p(ref), ctypes.c_void_p), ptr(roff), n,
        int(ksize), float(params['mu']), float(params['sigma']), float(params['epsilon']), int(params['casemin']), int(params['ctrlmax']),
        _off(params['caseabundlow']), _off(params['ctrlabundhigh']), 1 if params['dropoutliers'] else 0, ptr(records), ptr(likelihoods),
        ptr(counts), ptr(refr_abunds)))
    return Scored(records, likelihoods, counts, refr_abunds, kbase, ns)


def score_batch(windows, refrwindows, case, controls, refr, mu=30.0, sigma=8.0, epsilon=0.001, casemin=6, ctrlmax=1, caseabundlow=5,
                ctrlabundhigh=4, dropoutliers=False, batch_bytes=BATCH_BYTES):
    """Every (alt window, refr window) pair scored on the device: a `Scored`.  The only function of this module's second half
    that touches the device; inputs of more than `batch_bytes` window bytes go in several launches, whose results are joined."""
    params = dict(mu=mu, sigma=sigma, epsilon=epsilon, casemin=casemin, ctrlmax=ctrlmax, caseabundlow=caseabundlow,
                  ctrlabundhigh=ctrlabundhigh, dropoutliers=dropoutliers)
    if len(windows) != len(refrwindows):
        raise ValueError('{} alt windows but {} refr windows'.format(len(windows), len(refrwindows)))
    samples = [case] + list(controls)
    handles, ksize = [sketch._h for sketch in samples], case.ksize()
    cuts, size = [0], 0
    for c, (window, refrwindow) in enumerate(zip(windows, refrwindows)):
        if size and size + len(window) + len(refrwindow) > batch_bytes:
            cuts.append(c)
            size = 0
        size += len(window) + len(refrwindow)
    cuts.append(len(windows))
    parts = [_score_one_batch(windows[a:b], refrwindows[a:b], handles, refr._h, ksize, params) for a, b in zip(cuts, cuts[1:]) if b > a or a == 0]
    if len(parts) == 1:
        return parts[0]
    starts = np.cumsum([0] + [int(part.kbase[-1]) for part in parts])
    kbase = np.concatenate([parts[0].kbase[:1]] + [part.kbase[1:] + start for part, start in zip(parts, starts)])
    return Scored(np.concatenate([part.records for part in parts]), np.concatenate([part.likelihoods for part in parts]),
                  np.concatenate([part.counts for part in parts]), np.concatenate([part.refr for part in parts]), kbase, len(samples))


# ---- the reference's host half (kevlar/simlike.py:194-275, 303-384) -----------------------------------------------------------
class KevlarSampleLabelingError(ValueError):
    pass


def joinlist(thelist):
    return ','.join(str(value) for value in thelist) if len(thelist) else '.'


def default_sample_labels(nsamples):
    return ['Case'] + ['Control{:d}'.format(i) for i in range(1, nsamples)]


def annotate_abundances(call, abundances, refrabund, samplelabels):
    if len(refrabund) > 0 and None not in refrabund:
        call.annotate('REFRCOPYNUM', joinlist(refrabund))
    for sample, abundlist in zip(samplelabels, abundances):
        call.format(sample, 'ALTABUND', joinlist(abundlist))


def annotate_likescore(call, lldn, llfp, llih):
    """what the reference's calc_likescore writes, from likelihoods computed elsewhere"""
    call.annotate('LLDN', lldn)
    call.annotate('LLFP', llfp)
    call.annotate('LLIH', llih)
    call.annotate('LIKESCORE', lldn - max(llfp, llih))


def process_partition(partitionid, calls, ambigthresh=10):
    """One call per partition: of the passing calls only those with the best score stay unfiltered, and when more than
    `ambigthresh` share it none does."""
    passing = [call for call in calls if call.filterstr == 'PASS']
    if not passing:
        return
    best = max(call.attribute('LIKESCORE') for call in passing)
    winners = []
    for call in calls:
        if call.filterstr == 'PASS' and isclose(call.attribute('LIKESCORE'), best):
            winners.append(call)
        else:
            call.filter(VariantFilter.PartitionScore)
    ambiguous = bool(ambigthresh) and len(winners) > ambigthresh
    for call in winners:
        if ambiguous:
            call.filter(VariantFilter.AmbiguousCall)
        else:
            call.annotate('CALLCLASS', partitionid)


def window_check(call, ksize=31):
    """True when the call has no windows to score (missing, or shorter than k); says why for a call that was passing"""
    altspan, refspan = call.window, call.refrwindow
    complaints = []
    if altspan is None:
        complaints.append('    missing alt allele spanning window')
    if refspan is None:
        complaints.append('    missing refr allele spanning window')
    if altspan and len(altspan) < ksize:
        complaints.append('    alt allele spanning window {:s}, shorter than k size {:d}'.format(altspan, ksize))
    if refspan and len(refspan) < ksize:
        complaints.append('    ref allele spanning window {:s}, shorter than k size {:d}'.format(refspan, ksize))
    if not complaints:
        return False
    if call.filterstr == 'PASS':
        for message in ['WARNING: stubbornly refusing to compute likelihood:'] + complaints:
            kevlar_amd.plog('[kevlar::simlike]', message)
    return True


def simlike(variants, case, controls, refr, mu=30.0, sigma=8.0, epsilon=0.001, casemin=6, ctrlmax=1, caseabundlow=5, ctrlabundhigh=4,
            samplelabels=None, fastmode=False, minlikescore=0.0, dropoutliers=False, ambigthresh=10):
    """The calls of `variants`, scored, one kept per partition, best first.  All calls are read, those with windows to score go to
    the device in one `score_batch`, and the annotations follow in the order the calls came."""
    if samplelabels is None:
        samplelabels = default_sample_labels(len(controls) + 1)
    ksize = case.ksize()
    calls, toscore = [], []
    for call in variants:
        calls.append(call)
        if (fastmode and call.filterstr != 'PASS') or window_check(call, ksize):
            call.annotate('LIKESCORE', float('-inf'))
        else:
            toscore.append(call)
    scored = None
    if toscore:
        scored = score_batch([call.window for call in toscore], [call.refrwindow for call in toscore], case, controls, refr, mu=mu,
                             sigma=sigma, epsilon=epsilon, casemin=casemin, ctrlmax=ctrlmax, caseabundlow=caseabundlow,
                             ctrlabundhigh=ctrlabundhigh, dropoutliers=dropoutliers)
    progress_indicator = kevlar_amd.ProgressIndicator('[kevlar::simlike]     scores for {counter} calls computed')
    for c, call in enumerate(toscore):
        record = scored.records[c]
        flags = int(record[REC_FLAGS])
        call.annotate('DROPPED', int(record[REC_DROPPED]))
        for bit, kind in ((FLAG_PASSENGER, VariantFilter.PassengerVariant), (FLAG_CASE_ABUND, VariantFilter.CaseAbundance),
                          (FLAG_CTRL_ABUND, VariantFilter.ControlAbundance)):
            if flags & bit:
                call.filter(kind)
        if fastmode and call.filterstr != 'PASS':
            call.annotate('LIKESCORE', float('-inf'))
            continue
        if flags & FLAG_MISMATCH:       # the assertions of the reference's likelihood_denovo
            nrefr = int(record[REC_NREFR])
            raise AssertionError((int(record[1]), nrefr) if int(record[1]) != nrefr else (int(record[2]), nrefr))
        annotate_likescore(call, *[float(value) for value in scored.likelihoods[c]])
        annotate_abundances(call, *scored_lists(scored, c), samplelabels)
        progress_indicator.update()

    calls_by_partition = {}
    for call in calls:
        calls_by_partition.setdefault(call.attribute('PART'), []).append(call)
    allcalls = []
    for partition, partcalls in calls_by_partition.items():
        process_partition(partition, partcalls, ambigthresh=ambigthresh)
        allcalls.extend(partcalls)
    allcalls.sort(key=lambda call: call.attribute('LIKESCORE'), reverse=True)
    for call in allcalls:
        if call.attribute('LIKESCORE') < minlikescore:
            call.filter(VariantFilter.LikelihoodFail)
        yield call


def parser():
    """the reference's `kevlar simlike` flags and defaults (kevlar/cli/simlike.py)"""
    parser = argparse.ArgumentParser(prog='python -m kevlar_amd.simlike', add_help=False, description='Sort variants by likelihood score')
    count_args = parser.add_argument_group('K-mer count files', 'The scores rest on the abundance of the alternate allele k-mers in '
                                           'each sample and of the reference allele k-mers in the reference genome.')
    count_args.add_argument('--case', metavar='CT', required=True, help='counttable of the case / proband')
    count_args.add_argument('--controls', nargs='+', metavar='CT', required=True, help='counttables of the controls, one per sample')
    count_args.add_argument('--refr', metavar='REFR', required=True, help='smallcounttable of the reference genome')
    thresh_args = parser.add_argument_group('K-mer count thresholds', 'The thresholds that defined novel k-mers also tell true '
                                            'variants from spurious ones here.')
    thresh_args.add_argument('--ctrl-max', metavar='X', type=int, default=1, help='highest abundance allowed in a control; default is 1')
    thresh_args.add_argument('--case-min', metavar='Y', type=int, default=6, help='lowest abundance wanted in the case; default is 6')
    cov_args = parser.add_argument_group('K-mer coverage', 'The distribution of k-mer abundances in each sample, estimated or observed.')
    cov_args.add_argument('--mu', metavar='μ', type=float, default=30.0, help='mean k-mer abundance; default is 30.0')
    cov_args.add_argument('--sigma', metavar='σ', type=float, default=8.0, help='standard deviation of the k-mer abundance; default is 8.0')
    cov_args.add_argument('--epsilon', metavar='ε', type=float, default=0.001, help='error rate; default is 0.001')
    filt_args = parser.add_argument_group('Heuristic filters', 'These help when calling de novo variants and may need tuning for a '
                                          'data set.')
    filt_args.add_argument('--ctrl-abund-high', metavar='H', type=int, default=4,
                           help='filter a call when a control has more than H spanning k-mers of abundance above --ctrl-max; default is 4, '
                           'H <= 0 switches the filter off')
    filt_args.add_argument('--case-abund-low', metavar='L', type=int, default=5,
                           help='filter a call when the case has L or more consecutive spanning k-mers of abundance below --case-min; default '
                           'is 5, L <= 0 switches the filter off')
    filt_args.add_argument('--min-like-score', metavar='S', type=float, default=0.0, help='filter calls that score below S; default is 0.0')
    filt_args.add_argument('--drop-outliers', action='store_true',
                           help='leave out spanning k-mers whose abundance is far from the average (k-mers the reference genome lacks '
                           'by mistake); more sensitive, and more false calls')
    filt_args.add_argument('--ambig-thresh', metavar='A', type=int, default=10,
                           help='filter the calls of a contig with more than A distinct, equally good calls; default is 10, A = 0 switches '
                           'the filter off')
    misc_args = parser.add_argument_group('Miscellaneous settings')
    misc_args.add_argument('-h', '--help', action='help', help='show this help message and exit')
    misc_args.add_argument('--sample-labels', metavar='LBL', type=str, nargs='+', help='sample labels, the case first')
    misc_args.add_argument('-f', '--fast-mode', action='store_true', help='do no more work on calls that are already filtered')
    misc_args.add_argument('-o', '--out', metavar='OUT', default='-', help='output file; default is terminal (standard output)')
    parser.add_argument('vcf', nargs='+')
    return parser


def main(args):
    nsamples = len(args.controls) + 1
    if args.sample_labels:
        if len(args.sample_labels) != nsamples:
            raise KevlarSampleLabelingError('provided {:d} labels but {:d} samples'.format(len(args.sample_labels), nsamples))
    else:
        args.sample_labels = default_sample_labels(nsamples)

    kevlar_amd.plog('[kevlar::simlike] Loading k-mer counts for each sample')
    case = kevlar_amd.sketch.load(args.case)
    controls = [kevlar_amd.sketch.load(path) for path in args.controls]
    refr = kevlar_amd.sketch.load(args.refr)

    outstream = kevlar_amd.open(args.out, 'w')
    writer = VCFWriter(outstream, source='kevlar::simlike')
    for label in args.sample_labels:
        writer.register_sample(label)
    writer.write_header()

    kevlar_amd.plog('[kevlar::simlike]', 'Computing likelihood scores for preliminary variant calls')
    calculator = simlike(
        vcfstream(args.vcf), case, controls, refr, mu=args.mu, sigma=args.sigma, epsilon=args.epsilon, casemin=args.case_min,
        ctrlmax=args.ctrl_max, caseabundlow=args.case_abund_low, ctrlabundhigh=args.ctrl_abund_high, samplelabels=args.sample_labels,
        fastmode=args.fast_mode, minlikescore=args.min_like_score, dropoutliers=args.drop_outliers, ambigthresh=args.ambig_thresh)
    for call in calculator:
        writer.write(call)
    if outstream is not sys.stdout:
        outstream.close()


if __name__ == '__main__':
    main(parser().parse_args())
