"""What the simlike tests share: a plain-Python restatement of the reference's scoring loops (kevlar/simlike.py:22-191, 278-346),
written from the rules in DESIGN.md section 12 and working on anything with ksize() and get_kmer_counts(); the fixtures under
tests/golden/simlike with the expectations the reference's own tests state (recorded.json); and the generators of the planted
sketches and windows the device test scores."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'simlike')
RECORD_WORDS, MAX_SAMPLES = 20, 16
REC_NREFR, REC_DROPPED, REC_FLAGS, REC_NKMERS = 16, 17, 18, 19
PASSENGER, CASE_ABUND, CTRL_ABUND, MISMATCH, NO_REFR = 1, 2, 4, 8, 16
DEFAULTS = dict(mu=30.0, sigma=8.0, epsilon=0.001, casemin=6, ctrlmax=1, caseabundlow=5, ctrlabundhigh=4, dropoutliers=False)


def golden(rel):
    return os.path.join(GOLDEN, rel)


def recorded():
    with open(golden('recorded.json')) as handle:
        return json.load(handle)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def log_choose(n, k):
    return math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0)


def abund_log_prob(genotype, abundance, refrabund=None, mean=30.0, sd=8.0, error=0.001):
    if genotype == 0:
        if not refrabund:
            refrabund, error = 1, error * 0.01
        n = mean * refrabund
        a = float(abundance)
        if a > n:
            a = n
        return log_choose(math.floor(n), math.floor(a)) + a * math.log(error) + (n - a) * math.log(1.0 - error)
    loc, scale = (mean / 2, sd / 2) if genotype == 1 else (mean, sd)
    z = (abundance - loc) / scale
    return -(z * z) / 2.0 + (-math.log(scale) - 0.5 * math.log(2.0 * math.pi))


def likelihood_denovo(abunds, refrabunds, mean=30.0, sd=8.0, error=0.001):
    total = sum(abund_log_prob(1, a, mean=mean, sd=sd) for a in abunds[0])
    for control in abunds[1:]:
        total += sum(abund_log_prob(0, a, refrabund=r, mean=mean, error=error) for a, r in zip(control, refrabunds))
    return total


def likelihood_false(abunds, refrabunds, mean=30.0, error=0.001):
    return sum(abund_log_prob(0, a, refrabund=r, mean=mean, error=error) for sample in abunds for a, r in zip(sample, refrabunds))


SCENARIOS = [(1, 0, 1), (1, 0, 2), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 2, 0), (1, 2, 1), (2, 1, 1), (2, 1, 2), (2, 2, 1), (2, 2, 2)]


def likelihood_inherited(abunds, mean=30.0, sd=8.0, error=0.001):
    total = 0.0
    for trio in zip(abunds[0], abunds[1], abunds[2]):
        logp = [[abund_log_prob(g, a, mean=mean, sd=sd, error=error) for g in (0, 1, 2)] for a in trio]
        total += max(logp[0][gc] + logp[1][gm] + logp[2][gf] + math.log(1.0 / 15.0) for gc, gm, gf in SCENARIOS)
    return math.log(15.0 / 11.0) + total


def spanning(altseq, refrseq, case, controls, refr, dropoutliers=False):
    """(abundances, refr_abunds, ndropped): kevlar/simlike.py:22-96, an empty list staying empty under dropoutliers"""
    nkmers = len(altseq) - case.ksize() + 1
    genome = list(refr.get_kmer_counts(altseq))
    lists = [[c for c, g in zip(sample.get_kmer_counts(altseq), genome) if g == 0] for sample in [case] + list(controls)]
    if len(altseq) == len(refrseq):
        refrabunds = [c for c, g in zip(refr.get_kmer_counts(refrseq), genome) if g == 0]
    if dropoutliers:
        lists = [[a for a in counts if abs(a - sum(counts) / len(counts)) < 20] for counts in lists]
    if len(altseq) != len(refrseq):
        refrabunds = [None] * len(lists[0])
    return lists, refrabunds, nkmers - len(lists[0])


def filter_flags(lists, casemin, ctrlmax, caseabundlow, ctrlabundhigh):
    flags = 0
    if not any(a >= casemin for a in lists[0]):
        flags |= PASSENGER
    if caseabundlow and caseabundlow > 0:
        run = longest = 0
        for a in lists[0]:
            run = run + 1 if a < casemin else 0
            longest = max(longest, run)
        if longest >= caseabundlow:
            flags |= CASE_ABUND
    if ctrlabundhigh and ctrlabundhigh > 0:
        if any(sum(1 for a in control if a > ctrlmax) > ctrlabundhigh for control in lists[1:]):
            flags |= CTRL_ABUND
    return flags


def restate_call(altseq, refrseq, case, controls, refr, mu=30.0, sigma=8.0, epsilon=0.001, casemin=6, ctrlmax=1, caseabundlow=5,
                 ctrlabundhigh=4, dropoutliers=False):
    """(record, likelihoods or None, lists, refr_abunds) of one call, the record as kv_simlike_score writes it"""
    lists, refrabunds, ndropped = spanning(altseq, refrseq, case, controls, refr, dropoutliers)
    flags = filter_flags(lists, casemin, ctrlmax, caseabundlow, ctrlabundhigh)
    if len(altseq) != len(refrseq):
        flags |= NO_REFR
    likelihoods = None
    if len(lists[1]) != len(refrabunds) or len(lists[2]) != len(refrabunds):
        flags |= MISMATCH
    else:
        likelihoods = (likelihood_denovo(lists, refrabunds, mu, sigma, epsilon), likelihood_false(lists, refrabunds, mu, epsilon),
                       likelihood_inherited(lists, mu, sigma, epsilon))
    record = [len(counts) for counts in lists] + [0] * (MAX_SAMPLES - len(lists))
    record += [len(refrabunds), ndropped, flags, len(altseq) - case.ksize() + 1]
    return record, likelihoods, lists, refrabunds


class Scored(object):
    """the arrays kevlar_amd.simlike.score_batch returns, from the restatement"""

    def __init__(self, windows, refrwindows, case, controls, refr, **params):
        params.pop('batch_bytes', None)
        ns, ksize = len(controls) + 1, case.ksize()
        self.nsamples = ns
        self.kbase = np.zeros(len(windows) + 1, dtype=np.int64)
        np.cumsum([len(window) - ksize + 1 for window in windows], out=self.kbase[1:])
        self.records = np.zeros((len(windows), RECORD_WORDS), dtype=np.uint32)
        self.likelihoods = np.zeros((len(windows), 3), dtype=np.float64)
        self.counts = np.zeros(ns * int(self.kbase[-1]), dtype=np.uint8)
        self.refr = np.zeros(int(self.kbase[-1]), dtype=np.uint8)
        for c, (window, refrwindow) in enumerate(zip(windows, refrwindows)):
            record, likelihoods, lists, refrabunds = restate_call(window, refrwindow, case, controls, refr, **params)
            base, nk = int(self.kbase[c]), int(self.kbase[c + 1] - self.kbase[c])
            self.records[c] = record
            if likelihoods is not None:
                self.likelihoods[c] = likelihoods
            for s, counts in enumerate(lists):
                self.counts[ns * base + s * nk:ns * base + s * nk + len(counts)] = counts
            if None not in refrabunds:
                self.refr[base:base + len(refrabunds)] = refrabunds


def restated_score_batch(windows, refrwindows, case, controls, refr, **params):
    """stands in for kevlar_amd.simlike.score_batch where no device is wanted"""
    from kevlar_amd.simlike import Scored as Product
    got = Scored(windows, refrwindows, case, controls, refr, **params)
    return Product(got.records, got.likelihoods, got.counts, got.refr, got.kbase, got.nsamples)


def restate_simlike(variants, case, controls, refr, mu=30.0, sigma=8.0, epsilon=0.001, casemin=6, ctrlmax=1, caseabundlow=5,
                    ctrlabundhigh=4, samplelabels=None, fastmode=False, minlikescore=0.0, dropoutliers=False, ambigthresh=10,
                    log=None):
    """The reference's annotations (kevlar/simlike.py:303-346) on kevlar_amd.vcf.Variant objects, call by call.  `log` collects
    the lines the reference would print about windows it refuses."""
    from kevlar_amd.vcf import VariantFilter as vf
    labels = samplelabels or ['Case'] + ['Control{}'.format(i) for i in range(1, len(controls) + 1)]
    ksize, minus_inf = case.ksize(), float('-inf')
    partitions = {}
    for call in variants:
        partitions.setdefault(call.attribute('PART'), []).append(call)
        alt, ref = call.window, call.refrwindow
        unusable = alt is None or ref is None or len(alt) < ksize or len(ref) < ksize
        if unusable and call.filterstr == 'PASS' and log is not None:
            log.extend(['missing alt allele spanning window'] * (alt is None) + ['missing refr allele spanning window'] * (ref is None))
            if alt is not None and len(alt) < ksize:
                log.append('alt allele spanning window {}, shorter than k size {}'.format(alt, ksize))
            if ref is not None and len(ref) < ksize:
                log.append('ref allele spanning window {}, shorter than k size {}'.format(ref, ksize))
        if (fastmode and call.filterstr != 'PASS') or unusable:
            call.annotate('LIKESCORE', minus_inf)
            continue
        record, likelihoods, lists, refrabunds = restate_call(alt, ref, case, controls, refr, mu, sigma, epsilon, casemin, ctrlmax,
                                                              caseabundlow, ctrlabundhigh, dropoutliers)
        call.annotate('DROPPED', record[REC_DROPPED])
        for bit, kind in ((PASSENGER, vf.PassengerVariant), (CASE_ABUND, vf.CaseAbundance), (CTRL_ABUND, vf.ControlAbundance)):
            if record[REC_FLAGS] & bit:
                call.filter(kind)
        if fastmode and call.filterstr != 'PASS':
            call.annotate('LIKESCORE', minus_inf)
            continue
        assert likelihoods is not None, (record[1], record[REC_NREFR])
        for key, value in zip(('LLDN', 'LLFP', 'LLIH'), likelihoods):
            call.annotate(key, value)
        call.annotate('LIKESCORE', likelihoods[0] - max(likelihoods[1], likelihoods[2]))
        if refrabunds and None not in refrabunds:
            call.annotate('REFRCOPYNUM', ','.join(str(r) for r in refrabunds))
        for label, counts in zip(labels, lists):
            call.format(label, 'ALTABUND', ','.join(str(a) for a in counts) if counts else '.')
    ordered = []
    for partid, calls in partitions.items():
        passing = [call for call in calls if call.filterstr == 'PASS']
        if passing:
            best = max(call.attribute('LIKESCORE') for call in passing)
            winners = [call for call in passing if math.isclose(call.attribute('LIKESCORE'), best)]
            for call in calls:
                if not any(call is winner for winner in winners):
                    call.filter(vf.PartitionScore)
            for call in winners:
                if ambigthresh and len(winners) > ambigthresh:
                    call.filter(vf.AmbiguousCall)
                else:
                    call.annotate('CALLCLASS', partid)
        ordered.extend(calls)
    ordered.sort(key=lambda call: call.attribute('LIKESCORE'), reverse=True)
    for call in ordered:
        if call.attribute('LIKESCORE') < minlikescore:
            call.filter(vf.LikelihoodFail)
    return ordered


# ---- the fixtures of the reference's tests ---------------------------------------------------------------------------------------
KIND_BY_EXTENSION = {'.ct': 'Counttable', '.sct': 'SmallCounttable', '.nt': 'Nodetable'}


def load_sketch(module, path):
    """a saved sketch as `module` (the oracle, or the product's engine) loads it, the kind taken from the extension"""
    return getattr(module, KIND_BY_EXTENSION[os.path.splitext(path)[1]]).load(path)


FIXTURE_SKETCHES = {
    'case-low-abund': ('case-low-abund/kid.ct', 'case-low-abund/mom.ct', 'case-low-abund/dad.ct', 'case-low-abund/refr.sct'),
    'ctrl-high-abund': ('ctrl-high-abund/cc57120.kid.sct', 'ctrl-high-abund/cc57120.mom.sct', 'ctrl-high-abund/cc57120.dad.sct',
                        'ctrl-high-abund/cc57120.refr.sct'),
    # (the reference scores these against khmer.Nodetable(31, 1, 1), a sketch that holds nothing; so does an empty one of any size)
    'term-high-abund': ('term-high-abund/proband.ct', 'term-high-abund/mother.ct', 'term-high-abund/father.ct', None),
    'partscore': ('partscore/partscore-proband.ct', 'partscore/partscore-mother.ct', 'partscore/partscore-father.ct',
                  'partscore/partscore-refr.sct'),
    'simlike-fast-mode': ('simlike-fast-mode/cc27.kid.ct', 'simlike-fast-mode/cc27.mom.ct', 'simlike-fast-mode/cc27.dad.ct',
                          'simlike-fast-mode/cc27.refr.sct'),
}


def fixture_trio(module, name):
    kid, mom, dad, refr = FIXTURE_SKETCHES[name]
    genome = load_sketch(module, golden(refr)) if refr else module.Nodetable(31, 1e4, 1)
    return load_sketch(module, golden(kid)), load_sketch(module, golden(mom)), load_sketch(module, golden(dad)), genome


def read_calls(rel):
    import kevlar_amd
    return list(kevlar_amd.vcf.VCFReader(kevlar_amd.open(golden(rel), 'r')))


# ---- planted sketches and windows for the device test ----------------------------------------------------------------------------
def random_seq(rng, n):
    return ''.join('ACGT'[b] for b in rng.integers(0, 4, size=n))


def make_job(rng, k, nk, label, indel=False, reflen=None, case=None, ctrls=None, genome=None, refcopy=None, nctrl=2, alt=None):
    """One call: windows and what to plant.  case[i], ctrls[s][i], genome[i] are the counts wanted for the alt window's i-th k-mer
    in the case, control s and the reference genome's sketch, refcopy[i] that of the refr window's i-th k-mer in the latter."""
    alt = alt or random_seq(rng, nk + k - 1)
    ref = random_seq(rng, reflen if reflen else (len(alt) + 3 if indel else len(alt)))
    case = rng.integers(6, 13, size=nk) if case is None else np.asarray(case)
    ctrls = [rng.integers(0, 3, size=nk) if ctrls is None else np.asarray(ctrls[s]) for s in range(nctrl)]
    genome = (rng.random(nk) < 0.1).astype(int) if genome is None else np.asarray(genome)
    plant = []
    for i in range(nk):
        kmer = alt[i:i + k]
        if set(kmer) - set('ACGT'):
            continue
        plant += [(0, kmer, int(case[i]))] + [(1 + s, kmer, int(ctrls[s][i])) for s in range(nctrl)] + [('refr', kmer, int(genome[i]))]
    if not indel:
        refcopy = rng.integers(1, 4, size=nk) if refcopy is None else np.asarray(refcopy)
        plant += [('refr', ref[i:i + k], int(refcopy[i])) for i in range(nk)]
    return dict(label=label, alt=alt, ref=ref, plant=[item for item in plant if item[2] > 0])


def low_run(nk, start, length):
    counts = np.full(nk, 10)
    counts[start:start + length] = 2
    return counts


def edge_jobs(k, seed=20, nctrl=2, with_n=True):
    """The shapes and count patterns DESIGN.md section 12 lists, at k-mer size k, for the default thresholds (casemin 6, ctrlmax 1,
    L = 5, H = 4).  Every job has a label; tests/test_simlike_reference.py checks that each does what its label says."""
    rng = np.random.default_rng(seed + k)
    jobs = []
    add = lambda *args, **kwargs: jobs.append(make_job(rng, k, *args, nctrl=nctrl, **kwargs))   # noqa: E731
    zeros = lambda nk: np.zeros(nk, dtype=int)   # noqa: E731
    for nk in (1, 63, 64, 65, 128, 129):
        add(nk, 'snv-{}'.format(nk))
        add(nk, 'indel-{}'.format(nk), indel=True)
        add(nk, 'snv-{}-kept'.format(nk), genome=zeros(nk))
    add(61 - k + 1 if k <= 61 else 3, 'long-refr', indel=True, reflen=5000)
    add(40, 'all-dropped', genome=np.ones(40, dtype=int))
    add(40, 'none-dropped', genome=zeros(40))
    add(40, 'at-255', genome=zeros(40), case=np.full(40, 255), ctrls=[np.full(40, 255)] * nctrl)
    add(40, 'clamped', genome=zeros(40), ctrls=[np.full(40, 40)] + [rng.integers(0, 3, size=40) for _ in range(nctrl - 1)],
        refcopy=np.ones(40, dtype=int))
    add(40, 'refr-count-0', genome=zeros(40), refcopy=np.arange(40) % 3)
    for length in (4, 5, 6):
        add(100, 'lowrun-{}-inside'.format(length), genome=zeros(100), case=low_run(100, 20, length))
        add(100, 'lowrun-{}-across'.format(length), genome=zeros(100), case=low_run(100, 66 - length, length))
    case = low_run(100, 20, 4)
    case[25:29] = 2
    add(100, 'lowrun-two-short', genome=zeros(100), case=case)
    for high in (4, 5):
        ctrl = zeros(70)
        ctrl[[3, 30, 63, 64, 69][:high]] = 2
        add(70, 'ctrlhigh-{}'.format(high), genome=zeros(70), ctrls=[zeros(70)] * (nctrl - 1) + [ctrl])
    for where, at in (('first', 0), ('middle', 70), ('last', 139)):
        case = np.full(140, 12)
        case[at] = 60
        add(140, 'outlier-case-' + where, genome=zeros(140), case=case, ctrls=[zeros(140)] * nctrl)
    add(2, 'outlier-empties', genome=zeros(2), case=np.array([0, 50]), ctrls=[zeros(2)] * nctrl)
    ctrl = zeros(66)
    ctrl[65] = 80
    add(66, 'outlier-mismatch', genome=zeros(66), ctrls=[ctrl] + [zeros(66)] * (nctrl - 1))
    add(66, 'outlier-mismatch-indel', indel=True, genome=zeros(66), ctrls=[zeros(66)] * (nctrl - 1) + [ctrl])
    if with_n:
        alt = random_seq(rng, 50 + k - 1)
        alt = alt[:7] + 'N' + alt[8:20] + alt[20:30].lower() + alt[30:]
        add(50, 'n-and-lower-case', alt=alt, genome=zeros(50))
    return jobs


def seeded_jobs(k=31, n=300, seed=7, nctrl=2):
    rng = np.random.default_rng(seed)
    jobs = []
    for c in range(n):
        nk = int(rng.choice([1, 5, k, k, k, 2 * k + 3, 70, 130]))
        jobs.append(make_job(rng, k, nk, 'seeded-{}'.format(c), indel=bool(c % 3 == 0), nctrl=nctrl,
                             case=rng.integers(0, 12, size=nk) if c % 5 == 0 else None,
                             ctrls=[rng.integers(0, 5, size=nk) for _ in range(nctrl)] if c % 7 == 0 else None))
    return jobs


def plant(sketch, kmers, counts):
    """add kmers[i] counts[i] times"""
    if not kmers:
        return
    if hasattr(sketch, 'add_hashes'):                  # the product's engine: one device call
        sketch.add_hashes(np.repeat(sketch.hash_kmers(kmers), counts))
    else:
        for kmer, count in zip(kmers, counts):
            for _ in range(count):
                sketch.add(kmer)


FURTHER_KINDS = ('SmallCounttable', 'Nodetable', 'Counttable')


def planted_sketches(module, k, jobs, nctrl=2, refr_kind='SmallCounttable', sample_kinds=None):
    """(case, controls, refr): sketches of 1e5 bins and 4 tables holding what the jobs plant.  By default the trio are Counttables
    (counts to 255) and further controls cycle through FURTHER_KINDS."""
    kinds = sample_kinds or ['Counttable' if s < 3 else FURTHER_KINDS[(s - 3) % 3] for s in range(nctrl + 1)]
    sketches = {s: getattr(module, kinds[s])(k, 1e5, 4) for s in range(nctrl + 1)}
    sketches['refr'] = getattr(module, refr_kind)(k, 1e5, 4)
    for which, sketch in sketches.items():
        items = [(kmer, count) for job in jobs for target, kmer, count in job['plant'] if target == which]
        plant(sketch, [kmer for kmer, count in items], [count for kmer, count in items])
    return sketches[0], [sketches[1 + s] for s in range(nctrl)], sketches['refr']
