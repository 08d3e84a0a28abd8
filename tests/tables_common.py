"""What the tests of table counts and sample counts share (tests/test_gpu_tables.py on the device, tests/test_tables_reference.py
with the oracle alone): one small synthetic family and an unrelated one, the sketch geometries -- 1 to 16 tables (KV_MAX_TABLES), all
three storages, sizes on either side of 2^16 -- and the scans of up to 16 samples (KV_MAX_SAMPLES) built from them, with the oracle's
side of every comparison computed once per process and never changed afterwards.  Not a test module and not a conftest: nothing here
is collected.

A sample is described by a Spec: (kind, what, tables, reads).  `kind` is the class name; `what` is a table size (then `tables` tables of
the primes below it, as khmer picks them) or a tuple of primes; `reads` names a list of reads() below."""
import ctypes
from collections import namedtuple

import numpy as np

GENOME, SEED, N_READS, READ_LEN, ERROR = 40000, 7, 8000, 100, 0.005
STRANGER_SEED, STRANGER_READS, N_STRANGERS = 99, 1500, 13
KS = (31, 51)                               # one- and two-word keys
MAX_TABLES, MAX_SAMPLES = 16, 16            # include/kvsketch.h KV_MAX_TABLES, KV_MAX_SAMPLES
STRADDLE = (65521, 65537, 65539, 65543)     # one table below 2^16 bins (Barrett remainder), three above (the FP64 quotient)
CASE_MIN, CTRL_MAX = 6, 1

Spec = namedtuple('Spec', 'kind what tables reads')

_words, _reads = {}, {}


def _family():
    if _words:
        return
    from kevlar_amd import synth
    trio = synth.make_trio(GENOME, SEED, inherited_per_mb=400, denovo_per_mb=400)
    haps = dict(trio)
    # a second affected child: the proband's first haplotype (half of the de novo variants) beside the father's second
    haps['sibling'] = (trio['proband'][0], trio['father'][1])
    for i, name in enumerate(('proband', 'mother', 'father', 'sibling')):
        _words[name] = synth.sample_reads_packed(haps[name], N_READS, READ_LEN, ERROR, SEED + 1 + i)
    # people who share nothing with the family: whatever their sketches reject is a collision
    other = synth.make_trio(GENOME, STRANGER_SEED, inherited_per_mb=400, denovo_per_mb=400)
    members = ('proband', 'mother', 'father')
    for j in range(N_STRANGERS):
        _words['stranger{}'.format(j)] = synth.sample_reads_packed(other[members[j % 3]], STRANGER_READS, READ_LEN, ERROR, STRANGER_SEED + 1 + j)
    for name, w in _words.items():
        _reads[name] = synth.unpack_reads(w, READ_LEN)
    _reads['skew'] = _reads['proband'][:2000] + ['A' * READ_LEN] * 700      # the skew of test_skm_skew_saturation_and_overflow_paths
    _reads['mother-head'] = _reads['mother'][:3000]


def words(name):
    """the reads of a sample as packed words (uint32 [n, 7]): what the 2-bit kernels take"""
    _family()
    return _words[name]


def reads(name):
    """the same reads as a list of strings"""
    _family()
    return _reads[name]


def primes_of(ok, spec):
    return list(spec.what) if isinstance(spec.what, tuple) else ok.primes_below(spec.what, spec.tables)


def make(mod, spec, k, ok):
    """an empty sketch of `spec` from the device module or the oracle: the same primes on both sides, whatever either would pick"""
    return getattr(mod, spec.kind)(k, 0, 0, primes=primes_of(ok, spec))


_concat = {}


def concat(ok, name):
    if name not in _concat:
        _concat[name] = ok.concat_reads(reads(name))
    return _concat[name]


def oracle_count(ok, sketch, name, nbands=0, band=0, mask=None, threshold=0, consume_masked=False):
    bases, offs = concat(ok, name)
    return ok.consume_reads(sketch, bases, offs, len(reads(name)), nbands, band, mask, threshold, consume_masked)


_counted = {}


def oracle_sketch(ok, spec, k):
    """the oracle's sketch of `spec` with its reads counted: built once, shared, and only read from then on"""
    key = (spec, k)
    if key not in _counted:
        sk = make(ok, spec, k, ok)
        oracle_count(ok, sk, spec.reads)
        _counted[key] = sk
    return _counted[key]


def snapshot(sketch):
    """(bytes of every table, n_occupied)"""
    return [sketch.table_bytes(t) for t in range(len(sketch.hashsizes()))], sketch.n_occupied()


def assert_same_state(dev, want, what=''):
    tables, occupied = want
    assert dev.n_tables() == len(tables)
    for t, raw in enumerate(tables):
        assert dev.table_bytes(t) == raw, '{}: table {} of {} differs from the oracle'.format(what, t, len(tables))
    assert dev.n_occupied() == occupied, what


def launches(name):
    from kevlar_amd import _lib
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.load().kv_prof_get(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return n.value


# ---- section 1: the geometries every count path is held to -----------------------------------------------------------------------
def C(what, tables=0, reads='proband'):
    return Spec('Counttable', what, tables, reads)


def S(what, tables=0, reads='proband'):
    return Spec('SmallCounttable', what, tables, reads)


def N(what, tables=0, reads='proband'):
    return Spec('Nodetable', what, tables, reads)


COUNT_GEOMETRIES = {
    'C4x3e5': C(3e5, 4),            # the control row: the super-k-mer count drains through its 32-bit form (fast4)
    'C4x4e4': C(4e4, 4),            # every table below 2^16 bins
    'C4straddle': C(STRADDLE),      # both remainder forms within one k-mer
    'C1x3e5': C(3e5, 1), 'C2x3e5': C(3e5, 2), 'C3x3e5': C(3e5, 3),
    'S3x3e5': S(3e5, 3),
    'N2x1e6': N(1e6, 2), 'N7x1e6': N(1e6, 7),
    'C5x1e5': C(1e5, 5), 'C8x1e5': C(1e5, 8), 'C16x1e5': C(1e5, 16),
}
BIN_MAX_T = 4                       # kevlar_amd/csrc/kv_bin_plan.h: more tables than this take the atomic kernel whatever is asked for

_count_states = {}


def oracle_two_batches(ok, spec, k, first='proband', second='mother', nbands=0, band=0):
    """what the oracle holds after `first`, and after `second` on top: [(k-mers consumed, snapshot), (k-mers consumed, snapshot)]"""
    key = (spec, k, first, second, nbands, band)
    if key not in _count_states:
        sk = make(ok, spec, k, ok)
        out = []
        for name in (first, second):
            n = oracle_count(ok, sk, name, nbands, band)
            out.append((n, snapshot(sk)))
        _count_states[key] = out
    return _count_states[key]


# (mask, threshold, target): mask and target differ in table count and storage
MASK_CASES = {
    'N1-into-C3': (N(2e5, 1, 'mother-head'), 0, C(3e5, 3)),
    'N2-into-S4': (N(2e5, 2, 'mother-head'), 0, S(3e5, 4)),
    'N7-into-C6': (N(2e5, 7, 'mother-head'), 0, C(1e5, 6)),
    'C5t1-into-S4': (C(2e5, 5, 'mother-head'), 1, S(3e5, 4)),
    'C5t3-into-C3': (C(2e5, 5, 'mother-head'), 3, C(3e5, 3)),
}

_mask_states = {}


def oracle_masked(ok, name, k, consume_masked):
    key = (name, k, consume_masked)
    if key not in _mask_states:
        mask_spec, threshold, target = MASK_CASES[name]
        sk = make(ok, target, k, ok)
        n = oracle_count(ok, sk, 'proband', 0, 0, oracle_sketch(ok, mask_spec, k), threshold, consume_masked)
        _mask_states[key] = (n, snapshot(sk))
    return _mask_states[key]


# ---- section 2: scans -------------------------------------------------------------------------------------------------------------
Scan = namedtuple('Scan', 'cases ctrls case_min ctrl_max')

CROWDED = C(6e4, 16, 'mother')              # 16 tables of 6e4 bins under ~2e5 distinct k-mers: nearly every bin taken, the minimum of 16 still tells
MIXED_CTRLS = (CROWDED, S(3e5, 3, 'father'), N(1e6, 2, 'mother'))


def mixed_scan(case_tables, ctrl_max):
    return Scan((C(3e5, case_tables),), MIXED_CTRLS, CASE_MIN, ctrl_max)


NIBBLE_CASE_SCAN = Scan((S(3e5, 2),), (C(3e5, 4, 'mother'), C(3e5, 3, 'father')), CASE_MIN, CTRL_MAX)

MOTHER, FATHER = C(3e5, 4, 'mother'), S(3e5, 3, 'father')
_STRANGER_SHAPES = [lambda r: C(3e5, 4, r), lambda r: S(3e5, 3, r), lambda r: C(2e5, 6, r), lambda r: N(1e6, 2, r), lambda r: C(1e5, 11, r)]
STRANGERS = tuple(_STRANGER_SHAPES[j % len(_STRANGER_SHAPES)]('stranger{}'.format(j)) for j in range(N_STRANGERS))
PROBAND = C(3e5, 4)
# one case and 15 controls; with the case at place 0 the mother is sample 9 and the father sample 12, both behind the eight controls the
# list scan's predicate (novel_test_wide) unrolls
FIFTEEN_CTRLS = STRANGERS[:8] + (MOTHER,) + STRANGERS[8:10] + (FATHER,) + STRANGERS[10:]
SIXTEEN = Scan((PROBAND,), FIFTEEN_CTRLS, CASE_MIN, CTRL_MAX)
FIRST_EIGHT = Scan((PROBAND,), FIFTEEN_CTRLS[:8], CASE_MIN, CTRL_MAX)
NO_CONTROL = Scan((PROBAND,), (), CASE_MIN, CTRL_MAX)
PARENTS_ONLY = Scan((PROBAND,), (MOTHER, FATHER), CASE_MIN, CTRL_MAX)
TWO_CASES = Scan((PROBAND, C(3e5, 3, 'sibling')), STRANGERS[:12] + (MOTHER, FATHER), CASE_MIN, CTRL_MAX)
SEVENTEEN = Scan((PROBAND,), FIFTEEN_CTRLS + (C(1e5, 2, 'stranger0'),), CASE_MIN, CTRL_MAX)

# the table-count conditions: case and mother with 16 crowded tables each, with the first eight of those primes, and the case with table 0 alone
CROWDED_CASE = C(6e4, 16)
SIXTEEN_TABLES = Scan((CROWDED_CASE,), (CROWDED,), CASE_MIN, CTRL_MAX)


def first_primes(ok, spec, n):
    return Spec(spec.kind, tuple(primes_of(ok, spec)[:n]), 0, spec.reads)


_scan_hits = {}


def oracle_hits(ok, scan, k, scanned=None):
    """(read u32[n], offset u32[n], abundances u8[n, S]) of the reads of the first case (or of `scanned`), in scan order"""
    key = (scan, k, scanned)
    if key not in _scan_hits:
        cases = [oracle_sketch(ok, s, k) for s in scan.cases]
        ctrls = [oracle_sketch(ok, s, k) for s in scan.ctrls]
        name = scanned or scan.cases[0].reads
        bases, offs = concat(ok, name)
        r, o, a = ok.novel_scan_mt(cases, ctrls, bases, offs, len(reads(name)), k, scan.case_min, scan.ctrl_max, 4)
        _scan_hits[key] = (r, o.astype(np.uint32), a)
    return _scan_hits[key]


def positions(hits):
    """the (read, offset) pairs of a hit list, as one sorted uint64 array: what two scans over different samples can be compared by"""
    return np.sort(hits[0].astype(np.uint64) << np.uint64(32) | hits[1].astype(np.uint64))


def hits_difference(got, want):
    """None if two hit lists (read, offset, abundances) are equal, else what differs first"""
    if len(got[0]) != len(want[0]) or not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
        return '{} hits, the oracle has {}: other (read, offset) positions'.format(len(got[0]), len(want[0]))
    if not np.array_equal(got[2], want[2]):
        i = int(np.flatnonzero((got[2] != want[2]).any(axis=1))[0])
        return 'hit {} (read {}, offset {}): abundances {}, the oracle has {}'.format(i, int(got[0][i]), int(got[1][i]), got[2][i].tolist(), want[2][i].tolist())
    return None
