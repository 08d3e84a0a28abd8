"""CPU check of the host rules of the alignment and the call scan (kevlar_amd/csrc/kv_seq_jobs.h, kv_align_plan.h, kv_call_plan.h):
what a batch of sequences and jobs must satisfy, the order, the launches and every job's place in a launch's working memory, and
the descriptor of a job's runs -- the tokenizer's positions, the candidate of the end check and the class and the scanned blocks
for both of its answers -- against tokenize, endcheck and classify of tests/call_common.py.

The headers compile for the host; tests/harness/align_call_plan_host.cpp wraps them in a C ABI.  No GPU involved."""
import ctypes
import os
import random
import subprocess

import pytest

import call_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kevlar_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'harness', 'align_call_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libalign_call_plan_host.so')
HEADERS = [os.path.join(CSRC, name) for name in ('kv_require.h', 'kv_seq_jobs.h', 'kv_align_plan.h', 'kv_call_plan.h')]
KV_OK, KV_ERR_ARG, KV_ERR_CAPACITY = 0, -1, -6
MAX_LEN = 1 << 22
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
OP = {'M': 0, 'I': 1, 'D': 2}
NO_BLOCK = (0,) * 6


class CallBlock(ctypes.Structure):
    _fields_ = [(name, U32) for name in ('len', 'tpos', 'qpos', 'seam', 'tgap', 'qgap')]


class CallShape(ctypes.Structure):
    _fields_ = [(name, U32) for name in ('cls', 'indel_op', 'indel_len', 'indel_qpos')] + [('scan', CallBlock * 2)]


class CallJob(ctypes.Structure):
    _fields_ = ([(name, U64) for name in ('toff', 'qoff', 'ik_begin', 'ik_end')]
                + [(name, U32) for name in ('tlen', 'qlen', 'rev', 'index', 'fold_len', 'fold_t', 'fold_q', 'pad')] + [('shape', CallShape * 2)])


@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_last_error.restype = ctypes.c_char_p
    L.h_z_bytes.restype = U64
    L.h_z_bytes.argtypes = [U64, U64]
    L.h_constants.argtypes = [ctypes.c_void_p]
    L.h_seq_jobs.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p]
    L.h_align_layout.argtypes = [ctypes.c_void_p, U64, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.h_call_plan.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, U64,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def array(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def offsets_of(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def test_harness_and_test_share_their_constants(lib):
    out = (U64 * 9)()
    lib.h_constants(out)
    assert [int(v) for v in out] == [MAX_LEN, 64, 256, 6, 56, ctypes.sizeof(CallJob), cc.CLASS_CODE[None], cc.CLASS_CODE['snv'], cc.CLASS_CODE['indel']]
    assert ctypes.sizeof(CallJob) == 192 and CallJob.shape.offset == 64 and CallJob.fold_len.offset == 48


# ---------------------------------------------------------------- the job table
def seq_jobs(lib, noun, tlens, qlens, jobs, toffsets=None, qoffsets=None, n_jobs=None):
    """(return code, message, rows of (toff, qoff, tlen, qlen, target, query, rev)) of kv_seq_jobs"""
    toffsets = offsets_of(tlens) if toffsets is None else toffsets
    qoffsets = offsets_of(qlens) if qoffsets is None else qoffsets
    out = (U64 * (7 * max(len(jobs), 1)))()
    rc = lib.h_seq_jobs(b'entry', noun.encode(), array(U64, toffsets), len(toffsets) - 1, array(U64, qoffsets), len(qoffsets) - 1,
                        array(U32, [v for job in jobs for v in job]), len(jobs) if n_jobs is None else n_jobs, out)
    return rc, lib.h_last_error().decode(), [tuple(int(v) for v in out[7 * k:7 * k + 7]) for k in range(len(jobs))]


def call_plan(lib, targets, queries, jobs, runlists, annotations, run_offsets=None, ik_offsets=None, **entry_level):
    """the arguments of call_common.raw_scan through the headers alone: (return code, the rule that refused, descriptors)"""
    counts = [len(runs) for runs in runlists]
    run_offsets = offsets_of(counts)[:-1] if run_offsets is None else run_offsets
    runs = [run for runs in runlists for run in runs]
    ik_offsets = offsets_of([len(notes) for notes in annotations]) if ik_offsets is None else ik_offsets
    ikmers = [v for notes in annotations for pair in notes for v in pair]
    descs, stage = (CallJob * max(len(jobs), 1))(), ctypes.c_int(-1)
    rc = lib.h_call_plan(array(U64, offsets_of([len(t) for t in targets])), len(targets), array(U64, offsets_of([len(q) for q in queries])), len(queries),
                         array(U32, [v for job in jobs for v in job]), len(jobs), array(U64, run_offsets), array(U32, counts), array(U32, runs), len(runs),
                         array(U64, ik_offsets), array(U32, ikmers + [0, 0]), descs, ctypes.byref(stage))
    return rc, stage.value, descs


JOB_TABLE, IKMERS, RUNS = 1, 2, 3
ENTRY_LEVEL = {'ksize-0', 'negative-mindist'}           # kv_call_scan's own two checks: no sequence, index, strand flag or run in them


def rule_of(name):
    if name.startswith('ikmer'):
        return IKMERS
    return RUNS if 'run' in name else JOB_TABLE


def test_call_argument_errors_are_refused_by_the_headers_alone(lib):
    rc, stage, descs = call_plan(lib, **cc.GOOD_CALL)
    assert (rc, stage) == (KV_OK, 0) and (descs[0].tlen, descs[0].qlen, descs[0].shape[0].cls) == (10, 10, 1)
    seen = set()
    for name, change in cc.ARGUMENT_ERRORS:
        if name in ENTRY_LEVEL:
            continue
        rc, stage, _ = call_plan(lib, **dict(cc.GOOD_CALL, **change))
        assert (rc, stage) == (KV_ERR_ARG, rule_of(name)), (name, lib.h_last_error())
        seen.add(stage)
        if stage == JOB_TABLE:
            args = dict(cc.GOOD_CALL, **change)
            rc, message, _ = seq_jobs(lib, 'call', [len(t) for t in args['targets']], [len(q) for q in args['queries']], args['jobs'])
            assert rc == KV_ERR_ARG and message.startswith('call job 0 '), name
    assert seen == {JOB_TABLE, IKMERS, RUNS}
    assert len(cc.ARGUMENT_ERRORS) - len(ENTRY_LEVEL) == 19 and ENTRY_LEVEL < {name for name, _ in cc.ARGUMENT_ERRORS}


def test_alignment_argument_errors_are_refused_by_the_header_alone(lib):
    """the sequence, index and strand cases of test_align_reference.py::test_library_refuses_bad_arguments_before_it_touches_the_device"""
    for targets, queries, job, words in ((['ACGT'], [''], (0, 0, 0), 'alignment job 0 has an empty sequence'),
                                         (['', 'ACGT'], ['ACGT'], (0, 0, 1), 'alignment job 0 has an empty sequence'),
                                         (['ACGT'], ['ACGT'], (1, 0, 0), 'alignment job 0 names target 1 of 1, query 0 of 1, strand flag 0'),
                                         (['ACGT'], ['ACGT'], (0, 1, 0), 'alignment job 0 names target 0 of 1, query 1 of 1, strand flag 0'),
                                         (['ACGT'], ['ACGT'], (0, 0, 2), 'alignment job 0 names target 0 of 1, query 0 of 1, strand flag 2')):
        rc, message, _ = seq_jobs(lib, 'alignment', [len(t) for t in targets], [len(q) for q in queries], [job])
        assert (rc, message) == (KV_ERR_ARG, words)
    assert seq_jobs(lib, 'alignment', [4], [4], [])[0] == KV_OK
    # what both entries checked in front of their jobs
    assert seq_jobs(lib, 'alignment', None, [4], [(0, 0, 0)], toffsets=[0, 5, 3])[:2] == (KV_ERR_ARG, 'entry: target offsets must not decrease')
    assert seq_jobs(lib, 'call', [4], None, [(0, 0, 0)], qoffsets=[9, 5])[:2] == (KV_ERR_ARG, 'entry: query offsets must not decrease')
    assert seq_jobs(lib, 'call', [4], [4], [(0, 0, 0)], n_jobs=0x7FFFFFFF)[:2] == (KV_ERR_ARG, 'entry: 2147483647 jobs')
    out = (U64 * 7)()
    for toffsets, qoffsets, jobs in ((None, array(U64, [0, 4]), array(U32, [0, 0, 0])), (array(U64, [0, 4]), None, array(U32, [0, 0, 0])),
                                     (array(U64, [0, 4]), array(U64, [0, 4]), None)):
        assert lib.h_seq_jobs(b'entry', b'call', toffsets, 1, qoffsets, 1, jobs, 1, out) == KV_ERR_ARG
        assert lib.h_last_error() == b'entry: null argument'


def test_a_good_batch_yields_the_offsets_and_lengths_of_its_strings(lib):
    rng = random.Random(21)
    for noun in ('alignment', 'call'):
        targets = [cc.random_bases(rng, rng.randint(1, 90)) for _ in range(rng.randint(1, 12))] + ['']
        queries = [''] + [cc.random_bases(rng, rng.randint(1, 90)) for _ in range(rng.randint(1, 12))]
        jobs = [(rng.randrange(len(targets) - 1), rng.randrange(1, len(queries)), rng.randrange(2)) for _ in range(100)]
        rc, _, rows = seq_jobs(lib, noun, [len(t) for t in targets], [len(q) for q in queries], jobs)
        assert rc == KV_OK
        ttext, qtext = ''.join(targets), ''.join(queries)
        for (t, q, rev), (toff, qoff, tlen, qlen, target, query, flag) in zip(jobs, rows):
            assert (target, query, flag) == (t, q, rev)
            assert ttext[toff:toff + tlen] == targets[t] and qtext[qoff:qoff + qlen] == queries[q] and (tlen, qlen) == (len(targets[t]), len(queries[q]))


def test_the_length_limit_is_inclusive(lib):
    """offset arrays alone: no text is needed"""
    for noun in ('alignment', 'call'):
        rc, _, rows = seq_jobs(lib, noun, [7, MAX_LEN], [MAX_LEN, 3], [(1, 0, 1), (0, 1, 0)])
        assert rc == KV_OK and rows == [(7, 0, MAX_LEN, MAX_LEN, 1, 0, 1), (0, MAX_LEN, 7, 3, 0, 1, 0)]
        for tlens, qlens in (([7, MAX_LEN + 1], [MAX_LEN, 3]), ([7, MAX_LEN], [MAX_LEN + 1, 3])):
            rc, message, _ = seq_jobs(lib, noun, tlens, qlens, [(0, 1, 0), (1, 0, 1)])
            assert rc == KV_ERR_ARG and message == '{} job 1: sequences of {} and {} bases (at most {})'.format(noun, tlens[1], qlens[0], MAX_LEN)


# ---------------------------------------------------------------- the alignment's plan and layout
def z_bytes(tlen, qlen):
    """the direction bytes of a job: strips of 256 columns, tlen + 63 steps each, 256 bytes a step"""
    return -(-qlen // 256) * (tlen + 63) * 256


def align_layout(lib, rows, budget):
    """rows: (toff, qoff, tlen, qlen, rev) per job -> (return code, launch ends, descriptors in launch order, scalars)"""
    n = len(rows)
    ends, descs, scalars = (U64 * n)(), (U64 * (9 * n))(), (U64 * 5)()
    rc = lib.h_align_layout(array(U64, [v for row in rows for v in row]), n, budget, ends, descs, scalars)
    if rc != KV_OK:
        return rc, None, None, None
    names = ('index', 'toff', 'qoff', 'tlen', 'qlen', 'rev', 'zoff', 'bndoff', 'tmpoff')
    return (rc, [int(v) for v in ends[:int(scalars[0])]], [dict(zip(names, (int(v) for v in descs[9 * k:9 * k + 9]))) for k in range(n)],
            dict(zip(('launches', 'z_max', 'bnd_max', 'tmp_max', 'cells'), (int(v) for v in scalars))))


def disjoint_inside(intervals, bound):
    at = 0
    for begin, length in sorted(intervals):
        if begin < at:
            return False
        at = begin + length
    return at <= bound


def check_layout(lib, rows, budget):
    rc, ends, descs, scalars = align_layout(lib, rows, budget)
    assert rc == KV_OK
    order = [d['index'] for d in descs]
    n = len(rows)
    cells = [row[2] * row[3] for row in rows]
    # a permutation, largest first, equal ones in input order: the stable sort's answer is unique
    assert order == sorted(range(n), key=lambda k: (-cells[k], k))
    assert scalars['cells'] == sum(cells) and scalars['launches'] == len(ends) and ends[-1] == n and ends == sorted(set(ends))
    at = 0
    for launch, end in enumerate(ends):
        mine = descs[at:end]
        for d in mine:
            assert (d['toff'], d['qoff'], d['tlen'], d['qlen'], d['rev']) == tuple(rows[d['index']])
            assert d['zoff'] % 256 == 0
        used = sum(z_bytes(d['tlen'], d['qlen']) for d in mine)
        assert used <= budget
        assert disjoint_inside([(d['zoff'], z_bytes(d['tlen'], d['qlen'])) for d in mine], min(scalars['z_max'], budget))
        assert disjoint_inside([(d['bndoff'], 2 * d['tlen']) for d in mine], scalars['bnd_max'])
        assert disjoint_inside([(d['tmpoff'], d['tlen'] + d['qlen']) for d in mine], scalars['tmp_max'])
        if end < n:         # a launch is cut only where the next job would pass the budget
            assert used + z_bytes(descs[end]['tlen'], descs[end]['qlen']) > budget
        at = end
    return scalars


def test_z_bytes_at_the_strip_edges(lib):
    for tlen in (1, 63, 64, 65, 2000, MAX_LEN):
        for qlen in (1, 255, 256, 257, 512, 513, 2000, MAX_LEN):
            assert lib.h_z_bytes(tlen, qlen) == z_bytes(tlen, qlen) >= tlen * qlen


def budgets_of(rows):
    need = [z_bytes(row[2], row[3]) for row in rows]
    biggest, total = max(need), sum(need)
    return sorted({biggest, biggest + 1, biggest + (total - biggest) // 3, (biggest + total) // 2, max(total - 1, biggest), total, total + 1, 1 << 40})


def test_layout_of_seeded_batches(lib):
    rng = random.Random(22)
    launches = set()
    for n in [1, 2, 3, 7, 64, 200] + [rng.randint(1, 200) for _ in range(14)]:
        rows = [(rng.randrange(1 << 40), rng.randrange(1 << 40), rng.choice([rng.randint(1, 2000), rng.randint(1, 300), 64, 256]),
                 rng.choice([rng.randint(1, 2000), rng.randint(1, 300), 256, 257]), rng.randrange(2)) for _ in range(n)]
        for budget in budgets_of(rows):
            launches.add(check_layout(lib, rows, budget)['launches'])
        assert align_layout(lib, rows, budgets_of(rows)[0] - 1)[0] == KV_ERR_CAPACITY
        assert check_layout(lib, rows, 1 << 40)['launches'] == 1
    assert {1, 2, 3} <= launches and max(launches) > 20


def test_layout_at_the_strip_edges(lib):
    rows = [(1000 * k, 77 * k, tlen, qlen, k % 2) for k, (qlen, tlen) in enumerate((q, t) for q in (1, 255, 256, 257, 512, 513) for t in (1, 63, 64, 65))]
    for batch in (rows, rows[::-1], rows + rows):
        for budget in budgets_of(batch):
            check_layout(lib, batch, budget)
    # jobs of equal cells keep their order, whatever their shapes
    same = [(0, 0, 64, 256, 0), (0, 0, 256, 64, 1), (0, 0, 128, 128, 0), (0, 0, 256, 64, 0), (0, 0, 16384, 1, 1)]
    assert [d['index'] for d in align_layout(lib, same, 1 << 40)[2]] == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------- the call plan
def restate_plan(runs):
    """runs: [(kind, length)] -> what call_plan_job owes, by tokenize, endcheck and classify of call_common.py: the end check's
    candidate (fold_len, fold_t, fold_q) and the two shapes, each (class, indel op, indel length, indel qpos, block, block) with a
    block as (len, tpos, qpos, seam, tgap, qgap)"""
    cigar = ''.join('{}{}'.format(length, kind) for kind, length in runs)
    tlen, qlen = sum(n for kind, n in runs if kind in 'MD'), sum(n for kind, n in runs if kind in 'MI')
    # all bases alike: wherever the end check can fold, it does
    blocks = cc.tokenize('A' * qlen, 'A' * tlen, cigar)
    placed, tpos, qpos = [], 0, 0
    for length, kind, tseq, qseq in blocks:
        placed.append(dict(kind=kind, len=length, tpos=tpos, qpos=qpos))
        tpos, qpos = tpos + len(tseq or ''), qpos + len(qseq or '')
    assert (tpos, qpos) == (tlen, qlen) and [(b['kind'], b['len']) for b in placed] == list(runs)

    def shape(blocks, merged_at=None, merged=None):
        vartype = cc.classify(''.join('{}{}'.format(b['len'], b['kind']) for b in blocks))
        if vartype is None:
            return (0, 0, 0, 0, NO_BLOCK, NO_BLOCK)

        def scanned(at):
            at %= len(blocks)
            b = blocks[at]
            return merged if at == merged_at else (b['len'], b['tpos'], b['qpos'], b['len'], 0, 0)
        first = 0 if blocks[0]['kind'] == 'M' else 1            # Mapping._flanks of call_common.py
        if vartype == 'snv':
            return (1, 0, 0, 0, scanned(first), NO_BLOCK)
        gap = blocks[first + 1]
        return (2, OP[gap['kind']], gap['len'], gap['qpos'], scanned(first), scanned(-1 if blocks[-1]['kind'] == 'M' else -2))

    unfolded = shape(placed)
    if not cc.endcheck(blocks):
        assert len(placed) < 3 or placed[-1]['kind'] != 'M' or placed[-3]['kind'] != 'M'
        return tlen, qlen, (0, 0, 0), unfolded, unfolded
    third, middle, last = placed[-3:]
    assert third['kind'] == last['kind'] == 'M'
    # kevlar/cigar.py:52-61: the middle block's and the last block's bases in the sequence the middle block lies in (the target for
    # a D, else the query) against the last block's bases in the other one
    fold = (last['len'], middle['tpos'], last['qpos']) if middle['kind'] == 'D' else (last['len'], last['tpos'], middle['qpos'])
    merged = (third['len'] + last['len'], third['tpos'], third['qpos'], third['len'], last['tpos'] - (third['tpos'] + third['len']),
              last['qpos'] - (third['qpos'] + third['len']))
    after = placed[:-3] + [dict(third, len=merged[0]), middle]
    assert [(b['kind'], b['len']) for b in after] == [(kind, length) for length, kind, _, _ in blocks]      # the list endcheck left
    return tlen, qlen, fold, unfolded, shape(after, len(after) - 2, merged)


def shape_tuple(s):
    return (s.cls, s.indel_op, s.indel_len, s.indel_qpos) + tuple(tuple(getattr(b, f) for f in ('len', 'tpos', 'qpos', 'seam', 'tgap', 'qgap')) for b in s.scan)


def check_plan(lib, runs, reverse):
    """one job among other sequences, runs and k-mers, so that every offset is not 0"""
    tlen, qlen, fold, unfolded, folded = restate_plan(runs)
    packed = [length << 4 | OP[kind] for kind, length in runs]
    rc, stage, descs = call_plan(lib, ['T' * 3, 'T' * tlen], ['Q' * 5, 'Q' * qlen, 'Q'], [(0, 0, 0), (1, 1, int(reverse))], [[cc.M(3), cc.I(2)], packed],
                                 [[(0, 1)] * 2, [(0, 1)] * 4, []])
    assert (rc, stage) == (KV_OK, 0), lib.h_last_error()
    d = descs[1]
    assert (d.toff, d.qoff, d.ik_begin, d.ik_end, d.tlen, d.qlen, d.rev, d.index, d.pad) == (3, 5, 2, 6, tlen, qlen, int(reverse), 1, 0)
    assert (d.fold_len, d.fold_t, d.fold_q) == fold, runs
    assert shape_tuple(d.shape[0]) == unfolded and shape_tuple(d.shape[1]) == folded, runs
    return fold[0] != 0, unfolded[0], folded[0]


def test_call_plan_of_every_cigar_shape(lib):
    seen = set()
    for spec, cls, fold, folded in cc.CIGAR_SHAPES:
        runs = [(block[0], block[1]) for block in spec]
        for reverse in (False, True):
            can_fold, unfolded_cls, folded_cls = check_plan(lib, runs, reverse)
            # the table says what the device must answer when the bases decide as `fold` has them built
            assert (folded_cls if folded else unfolded_cls) == cc.CLASS_CODE[cls], runs
            assert can_fold or not folded
            kinds = ''.join(kind for kind, _ in runs)
            if kinds[-3:] in ('MIM', 'MDM'):
                assert can_fold
            else:
                assert can_fold == (kinds[-3:] == 'MMM')        # endcheck asks of the middle block only whether it is a D
            seen.add((can_fold, unfolded_cls, folded_cls))
    assert {(False, 0, 0), (False, 1, 1), (False, 2, 2), (True, 2, 1), (True, 0, 2), (True, 0, 0)} <= seen


def test_call_plan_of_seeded_run_lists(lib):
    rng = random.Random(23)
    seen, made = set(), 0
    while made < 2000:
        runs = [(rng.choice('MMID'), rng.randint(1, 40)) for _ in range(rng.randint(1, 9))]
        if not any(kind in 'MD' for kind, _ in runs) or not any(kind in 'MI' for kind, _ in runs):
            continue                                                        # (a job has no empty sequence)
        made += 1
        can_fold, unfolded_cls, folded_cls = check_plan(lib, runs, made % 2)
        seen.add((len(runs), can_fold))
        seen.add(('classes', unfolded_cls, folded_cls))
    assert {(n, can_fold) for n in range(3, 10) for can_fold in (False, True)} <= seen and (1, False) in seen and (2, False) in seen
    assert {('classes', 1, 1), ('classes', 2, 2), ('classes', 2, 1), ('classes', 0, 2), ('classes', 0, 0)} <= seen
