"""Host-side checks of contig-to-cutout alignment: the plain-Python restatement of the rule (tests/align_common.py) against what
the reference's compiled align() returned (tests/golden/align/recorded.json), CIGAR formatting, the launch planner, argument
validation, and align_partitions' ordering with the device call stubbed out.  No kernel is launched here."""
import ctypes
import io

import numpy as np
import pytest

import align_common as ac


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kevlar_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def records():
    return ac.recorded()


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_test_pair(records):
    assert ac.restated_align(ac.LITERAL_TARGET, ac.LITERAL_QUERY) == ac.LITERAL_RESULT
    assert (records['literal']['cigar'], records['literal']['score']) == ac.LITERAL_RESULT


def test_restatement_reproduces_the_recorded_fixture_alignments(records):
    """every fixture pair on both strands under the default scoring, and the pairs of the cigar and pico fixtures under the
    other three: about 4 M cells, what the restatement does in a few seconds"""
    assert records['scorings'] == [list(s) for s in ac.SCORINGS]
    pairs = ac.fixture_pairs()
    assert len(records['pairs']) == len(pairs) * 2 * len(ac.SCORINGS)
    checked = 0
    for key, target, query in pairs:
        small = key.startswith(('cigar-', 'pico-'))
        for scoring in ac.SCORINGS if small else ac.SCORINGS[:1]:
            for strand, seq in ((1, query), (-1, ac.rc(query))):
                cigar, score = ac.restated_align(target, seq, *scoring)
                assert [cigar, score] == records['pairs'][ac.record_key(key, strand, scoring)], (key, strand, scoring)
                checked += 1
    assert checked >= 2 * len(pairs)


def test_recorded_winners_are_the_cigars_the_reference_tests_record(records):
    assert records['test_call'] == {'pico-7': '10D83M190D75M20I1M', 'pico-2': '10D89M153I75M20I'}
    for name, cigar in records['test_call'].items():
        winners = [ac.restated_both_strands(target, query)[1] for key, target, query in ac.fixture_pairs() if key.startswith(name + ':')]
        assert cigar in winners


def test_large_pairs_come_from_the_generators(records):
    assert [(r['kind'], r['seed'], r['strand']) for r in records['large']] == [(k, s, st) for k, s in ac.LARGE for st in (1, -1)]
    for rec in records['large']:
        target, query = ac.large_pair(rec['kind'], rec['seed'])
        assert (len(target), len(query)) == (rec['tlen'], rec['qlen'])
    assert records['large'][0]['tlen'] == 10000 and records['large'][0]['qlen'] == 3000 and '30D' in records['large'][0]['cigar']
    assert records['large'][2]['qlen'] > records['large'][2]['tlen']


def test_restatement_ties_and_strands():
    # a palindromic query scores the same on both strands: the forward strand is kept
    half = 'ACGGTCA'
    query = half + ac.rc(half)
    assert ac.rc(query) == query
    assert ac.restated_both_strands('TT' + query + 'GG', query)[2] == 1
    score, cigar, strand = ac.restated_both_strands('TTGACCATTGACGGACGT', ac.rc('GACCATTGACGG'))
    assert strand == -1 and cigar == '2D12M4D' and score == 12 - 10


# ---- CIGAR strings ---------------------------------------------------------------------------------------------------------------
def test_cigar_string_from_runs():
    from kevlar_amd.alignment import cigar_string
    assert cigar_string([]) == ''
    assert cigar_string([10 << 4 | 2, 91 << 4, 69 << 4 | 2, 79 << 4, 20 << 4 | 1]) == '10D91M69D79M20I'
    assert cigar_string(np.array([(1 << 22) << 4 | 1, 1 << 4], dtype=np.uint32)) == '4194304I1M'


# ---- the planner -----------------------------------------------------------------------------------------------------------------
def test_z_bytes_follow_the_strip_width(lib):
    from kevlar_amd import alignment
    w = ac.ALIGN_STRIP
    assert alignment.ALIGN_STRIP == w
    assert alignment.z_bytes(1, 1) == 64 * w
    assert alignment.z_bytes(1, w) == 64 * w and alignment.z_bytes(1, w + 1) == 2 * 64 * w
    assert alignment.z_bytes(10000, 3000) == 12 * 10063 * w
    for tlen, qlen in ((100, 100), (7, 2 * w + 1), (4000, w - 1)):
        assert alignment.z_bytes(tlen, qlen) >= tlen * qlen


def test_planner_orders_largest_first_and_cuts_at_the_budget(lib):
    from kevlar_amd import _lib, alignment
    tlens = [10, 500, 10, 3000, 500, 1]
    qlens = [10, 300, 10, 600, 300, 1]
    zb = [alignment.z_bytes(t, q) for t, q in zip(tlens, qlens)]
    order, ends = alignment.plan_launches(tlens, qlens, sum(zb))
    assert order == [3, 1, 4, 0, 2, 5]                      # by cells, equal ones in the order given
    assert ends == [6]
    order, ends = alignment.plan_launches(tlens, qlens, zb[3])
    assert order == [3, 1, 4, 0, 2, 5]
    launches = [order[a:b] for a, b in zip([0] + ends[:-1], ends)]
    assert launches[0] == [3] and len(launches) >= 2
    assert all(sum(zb[k] for k in launch) <= zb[3] for launch in launches)
    # greedy in that order: a launch ends exactly where the next job would not fit
    for launch, following in zip(launches, launches[1:]):
        assert sum(zb[k] for k in launch) + zb[following[0]] > zb[3]
    assert alignment.plan_launches([], [], 1 << 20) == ([], [])
    with pytest.raises(_lib.KvCapacityError):
        alignment.plan_launches(tlens, qlens, zb[3] - 1)
    with pytest.raises(_lib.KvArgError):
        alignment.plan_launches([5, 0], [5, 5], 1 << 30)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _call_batch(lib, targets, queries, jobs, scoring=(1, 2, 5, 0), budget=1 << 30):
    from kevlar_amd.alignment import _text
    tbases, toff = _text(targets)
    qbases, qoff = _text(queries)
    jobs = np.ascontiguousarray(jobs, dtype=np.uint32).reshape(-1, 3)
    n = len(jobs)
    scores, offs, counts, runs = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32), np.zeros(16, np.uint32)
    need = ctypes.c_uint64(0)
    return lib.kv_align_batch(tbases.ctypes.data, toff.ctypes.data, len(targets), qbases.ctypes.data, qoff.ctypes.data, len(queries),
                              jobs.ctypes.data, n, scoring[0], scoring[1], scoring[2], scoring[3], budget, scores.ctypes.data,
                              offs.ctypes.data, counts.ctypes.data, runs.ctypes.data, 16, ctypes.byref(need))


def test_library_refuses_bad_arguments_before_it_touches_the_device(lib):
    """(this machine may have no device at all: every refusal below comes from host code)"""
    from kevlar_amd import _lib
    assert _call_batch(lib, ['ACGT'], [''], [(0, 0, 0)]) == _lib.KV_ERR_ARG
    assert b'empty' in lib.kv_last_error()
    assert _call_batch(lib, ['', 'ACGT'], ['ACGT'], [(0, 0, 1)]) == _lib.KV_ERR_ARG
    assert _call_batch(lib, ['ACGT'], ['ACGT'], [(1, 0, 0)]) == _lib.KV_ERR_ARG
    assert _call_batch(lib, ['ACGT'], ['ACGT'], [(0, 1, 0)]) == _lib.KV_ERR_ARG
    assert _call_batch(lib, ['ACGT'], ['ACGT'], [(0, 0, 2)]) == _lib.KV_ERR_ARG
    for scoring in ((128, 2, 5, 0), (-1, 2, 5, 0), (1, 128, 5, 0), (1, -128, 5, 0), (1, 2, 128, 0), (1, 2, -1, 0), (1, 2, 5, 128), (1, 2, 5, -1)):
        assert _call_batch(lib, ['ACGT'], ['ACGT'], [(0, 0, 0)], scoring) == _lib.KV_ERR_ARG, scoring
    assert _call_batch(lib, ['ACGT' * 100], ['ACGT' * 100], [(0, 0, 0)], budget=1000) == _lib.KV_ERR_CAPACITY
    assert _call_batch(lib, ['ACGT'], ['ACGT'], []) == _lib.KV_OK                    # nothing to do, nothing launched


def test_wrapper_refuses_bad_arguments(lib):
    from kevlar_amd import _lib, alignment
    with pytest.raises(_lib.KvArgError):
        alignment.contig_align('ACGT', '')
    with pytest.raises(_lib.KvArgError):
        alignment.contig_align('', 'ACGT')
    with pytest.raises(_lib.KvArgError):
        alignment.contig_align('ACGT', 'ACGT', match=128)
    with pytest.raises(_lib.KvArgError):
        alignment.contig_align('ACGT', 'ACGT', gapextend=-1)
    with pytest.raises(_lib.KvArgError):
        alignment.align_batch(['ACGT'], ['ACGT'], [(0, 1)])
    assert alignment.check_scoring(1, -2, 5, 0) == alignment.check_scoring(1, 2, 5, 0) == (1, 2, 5, 0)
    assert alignment.align_batch(['ACGT'], ['ACGT'], []) == []


def test_public_names():
    import kevlar_amd
    from kevlar_amd import alignment
    assert kevlar_amd.align is alignment.contig_align
    assert callable(alignment.align_both_strands) and callable(alignment.align_batch) and callable(alignment.align_partitions)


# ---- align_partitions, device call stubbed ------------------------------------------------------------------------------------
def test_align_partitions_order_and_nocall(monkeypatch, lib):
    import kevlar_amd
    from kevlar_amd import alignment
    from kevlar_amd.reference import ReferenceCutout

    calls = []

    def stub(targets, queries, jobs, scoring, z_budget, capacity):
        calls.append((list(targets), list(queries), list(jobs), scoring))
        # forward score: the query's length; reverse: 1 more for queries that start with 'T'
        return [(len(queries[q]) + (1 if rev and queries[q].startswith('T') else 0), '{}M{}'.format(t, 'r' if rev else 'f')) for t, q, rev in jobs]

    monkeypatch.setattr(alignment, '_device_batch', stub)
    contigs = {
        '1': [kevlar_amd.Record(name='c1a', sequence='ACGTA'), kevlar_amd.Record(name='c1b', sequence='TTGACCATT'),
              kevlar_amd.Record(name='c1c', sequence='GGGGG')],
        '2': [kevlar_amd.Record(name='c2a', sequence='ACG')],
        '3': [kevlar_amd.Record(name='c3a', sequence='ACGT')],             # no cutouts: left out
    }
    cutouts = {
        '2': [ReferenceCutout('chr2_100-104', 'ACGT')],
        '1': [ReferenceCutout('chrB_5-9', 'TTTT'), ReferenceCutout('chrA_100-20100', 'ACGT' * 5000), ReferenceCutout('chrA_10-16', 'GATTAC')],
        '9': [ReferenceCutout('chr9_0-4', 'AAAA')],
    }
    got = list(alignment.align_partitions(contigs, cutouts, maxtargetlen=10000))
    assert len(calls) == 1                                   # all partitions in one batch
    targets, queries, jobs, scoring = calls[0]
    assert scoring == (1, 2, 5, 0)
    # partitions as the contigs give them; contigs longest first (equal lengths in the order given); cutouts by defline
    assert [(p, c.name, t.defline) for p, c, t, score, cigar, strand in got] == [
        ('1', 'c1b', 'chrA_10-16'), ('1', 'c1b', 'chrA_100-20100'), ('1', 'c1b', 'chrB_5-9'),
        ('1', 'c1a', 'chrA_10-16'), ('1', 'c1a', 'chrA_100-20100'), ('1', 'c1a', 'chrB_5-9'),
        ('1', 'c1c', 'chrA_10-16'), ('1', 'c1c', 'chrA_100-20100'), ('1', 'c1c', 'chrB_5-9'),
        ('2', 'c2a', 'chr2_100-104')]
    # the cutout whose interval is longer than maxtargetlen is not aligned: the reference's nocall
    assert [(score, cigar, strand) for p, c, t, score, cigar, strand in got if t.defline == 'chrA_100-20100'] == [(0, None, 1)] * 3
    assert all(len(targets[t]) < 20000 for t, q, rev in jobs)
    assert len(jobs) == 2 * 7 and [rev for t, q, rev in jobs] == [0, 1] * 7
    # the strand rule: reverse only when strictly greater
    by_name = {(c.name, t.defline): (score, cigar, strand) for p, c, t, score, cigar, strand in got}
    assert by_name[('c1b', 'chrA_10-16')][0] == 10 and by_name[('c1b', 'chrA_10-16')][2] == -1 and by_name[('c1b', 'chrA_10-16')][1].endswith('r')
    assert by_name[('c1a', 'chrB_5-9')][0] == 5 and by_name[('c1a', 'chrB_5-9')][2] == 1 and by_name[('c1a', 'chrB_5-9')][1].endswith('f')
    # every job names the sequences of its own pair
    for (p, c, t, score, cigar, strand) in got:
        if cigar is not None:
            assert any(targets[tj] == t.sequence and queries[qj] == c.sequence for tj, qj, rev in jobs)
    # maxtargetlen = 0 switches the limit off, as in the reference
    calls.clear()
    got = list(alignment.align_partitions(contigs, cutouts, maxtargetlen=0))
    assert all(cigar is not None for p, c, t, score, cigar, strand in got) and len(calls[0][2]) == 2 * 10


def test_align_partitions_takes_what_the_readers_yield(monkeypatch, lib):
    import kevlar_amd
    from kevlar_amd import alignment

    monkeypatch.setattr(alignment, '_device_batch', lambda targets, queries, jobs, *rest: [(0, '1M')] * len(jobs))
    contig_text = '>contig1 kvcc=7\nACGTACGT\n>contig2 kvcc=7\nACGTACGTAA\n>contig3 kvcc=8\nTTTT\n'
    parts = list(kevlar_amd.parse_partitioned_reads(kevlar_amd.parse_augmented_fastx(io.StringIO(contig_text))))
    cutouts = {}
    for cutout in kevlar_amd.reference.load_refr_cutouts(io.StringIO('>chr1_10-14 kvcc=7\nACGT\n>chr1_30-34 kvcc=8\nTTTT\n')):
        cutouts.setdefault(cutout.defline.split('kvcc=')[1], []).append(cutout)
    got = list(alignment.align_partitions(parts, cutouts))
    assert [(p, c.name.split()[0], t.defline.split()[0]) for p, c, t, score, cigar, strand in got] == [
        ('7', 'contig2', 'chr1_10-14'), ('7', 'contig1', 'chr1_10-14'), ('8', 'contig3', 'chr1_30-34')]
