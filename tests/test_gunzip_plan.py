"""CPU check of the host rules of the parallel gzip decoder (kevlar_amd/csrc/kv_gunzip_plan.h): the segment's extent, the starts,
the cuts, the jobs and their room, the chain walk and the CRC ranges, against the plain-Python restatement and the simulated
decoder of tests/gunzip_plan_common.py.  The walk is also taken down the arms no real gzip stream reaches on demand: 201
repairs, a repair of a repair, the room of a GZ_FULL retry, a stretch that passes two member trailers, a landing on nobody's start.

The header compiles for the host; tests/harness/gunzip_plan_host.cpp wraps it in a C ABI.  No GPU involved."""
import ctypes
import os
import random
import subprocess

import pytest

import gunzip_plan_common as gp

ROOT = gp.ROOT
SRC = os.path.join(ROOT, 'tests', 'harness', 'gunzip_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libgunzip_plan_host.so')
C = gp.C
NONE = gp.NONE
U64 = ctypes.c_uint64
JOB_FIELDS = ('start_bit', 'target_idx', 'out_off', 'header_bit', 'out_cap')
RESULT_FIELDS = ('end_bit', 'n_out', 'status', 'members', 'isize_sum', 'trailer_at', 'trailer_crc')
CHAIN_SCALARS = ('text', 'end_rel', 'isize_seg', 'repairs', 'ended', 'crc_lost', 'fail', 'fail_bit')


class GzJob(ctypes.Structure):
    _fields_ = [('start_bit', U64), ('target_idx', U64), ('out_off', U64), ('header_bit', U64), ('out_cap', ctypes.c_uint32), ('pad', ctypes.c_uint32)]


class GzResult(ctypes.Structure):
    _fields_ = [('end_bit', U64), ('n_out', ctypes.c_uint32), ('status', ctypes.c_uint16), ('members', ctypes.c_uint16), ('isize_sum', ctypes.c_uint32),
                ('trailer_at', ctypes.c_uint32), ('trailer_crc', ctypes.c_uint32), ('pad', ctypes.c_uint32)]


DECODE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(GzJob), ctypes.POINTER(GzResult))


@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in (SRC, gp.HDR)):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_gz_starts.restype = ctypes.c_int
    for name in ('h_gz_guesses', 'h_gz_merge', 'h_gz_crc_ranges'):
        getattr(L, name).restype = U64
    L.h_gz_room.restype = ctypes.c_uint32
    ext = [U64, U64, U64, ctypes.c_double, ctypes.c_uint32]
    L.h_gz_constants.argtypes = [ctypes.c_void_p]
    L.h_gz_extent.argtypes = ext + [ctypes.c_void_p]
    L.h_gz_starts.argtypes = ext + [ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_void_p]
    L.h_gz_guesses.argtypes = ext + [ctypes.c_void_p, U64, ctypes.c_int, U64, U64, ctypes.c_void_p, U64]
    L.h_gz_merge.argtypes = [ctypes.c_void_p, U64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_void_p]
    L.h_gz_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_int, U64, ctypes.c_double, ctypes.c_void_p, U64, ctypes.c_void_p]
    L.h_gz_room.argtypes = [ctypes.c_double, U64]
    L.h_gz_walk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_int, U64, ctypes.c_double, DECODE, ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p]
    L.h_gz_crc_ranges.argtypes = [U64, ctypes.c_void_p, U64, ctypes.c_uint32, ctypes.c_void_p, U64]
    return L


def u64s(values):
    return (U64 * max(len(values), 1))(*values)


def c_extent(lib, args):
    out = (U64 * 9)()
    lib.h_gz_extent(*args, out)
    return dict(zip(gp.EXTENT_FIELDS, (int(v) for v in out)))


def c_starts(lib, args, cand):
    cap = len(cand) + 1
    starts, headers, scalars = (U64 * cap)(), (U64 * cap)(), (U64 * 3)()
    ok = lib.h_gz_starts(*args, u64s(cand), len(cand), starts, headers, cap, scalars)
    n = int(scalars[0])
    assert n <= cap and list(starts[:n]) == list(headers[:n])
    return bool(ok), [int(v) for v in starts[:n]], bool(scalars[1]), int(scalars[2])


def c_guesses(lib, args, starts, have_terminal, wanted, max_guesses):
    cap = 8 * len(starts) + 8
    out = (U64 * (2 * cap))()
    n = lib.h_gz_guesses(*args, u64s(starts), len(starts), int(have_terminal), wanted, max_guesses, out, cap)
    assert n <= cap
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def c_merge(lib, starts, have_terminal, guesses, found):
    cap = len(starts) + len(guesses)
    s_out, h_out, n_out = (U64 * cap)(), (U64 * cap)(), U64()
    flat = [v for g in guesses for v in g]
    taken = lib.h_gz_merge(u64s(starts), len(starts), int(have_terminal), u64s(flat), u64s(found), len(guesses), s_out, h_out, cap, ctypes.byref(n_out))
    n = n_out.value
    assert n <= cap
    return [int(v) for v in s_out[:n]], [int(v) for v in h_out[:n]], int(taken)


def c_plan(lib, starts, headers, have_terminal, n_bytes, ratio):
    cap = len(starts)
    jobs, scalars = (GzJob * cap)(), (U64 * 4)()
    lib.h_gz_plan(u64s(starts), u64s(headers), len(starts), int(have_terminal), n_bytes, ratio, jobs, cap, scalars)
    n = int(scalars[0])
    assert n <= cap and all(jobs[j].pad == 0 for j in range(n))
    return {'jobs': [{f: int(getattr(jobs[j], f)) for f in JOB_FIELDS} for j in range(n)], 'total_cap': int(scalars[1]), 'repair_room': int(scalars[2]),
            'exact': int(scalars[3])}


def c_walk(lib, starts, headers, have_terminal, n_bytes, ratio, decode):
    """gz_walk_chain over a Python decoder, in the shape of gp.walk_chain()"""
    def answer(job, result):
        got = decode({f: int(getattr(job[0], f)) for f in JOB_FIELDS})
        for f in RESULT_FIELDS:
            setattr(result[0], f, got[f])
        result[0].pad = 0
        return 0
    cap = len(starts) + C['GZ_MAX_REPAIRS'] + 2
    v, ends, scalars = (U64 * (3 * cap))(), (U64 * (2 * cap))(), (U64 * 11)()
    lib.h_gz_walk(u64s(starts), u64s(headers), len(starts), int(have_terminal), n_bytes, ratio, DECODE(answer), v, cap, ends, cap, scalars)
    nv, ne = int(scalars[0]), int(scalars[1])
    assert nv <= cap and ne <= cap and int(scalars[10]) == 0
    out = dict(zip(CHAIN_SCALARS, (int(x) for x in scalars[2:10])))
    out['v'] = [tuple(int(x) for x in v[3 * i:3 * i + 3]) for i in range(nv)]
    out['ends'] = [tuple(int(x) for x in ends[2 * i:2 * i + 2]) for i in range(ne)]
    return out


def test_harness_and_test_share_their_constants(lib):
    out = (U64 * 12)()
    lib.h_gz_constants(out)
    assert [int(v) for v in out] == [C['GZ_FIND_KEEP'], C['GZ_MARGIN'], C['GZ_MAX_REPAIRS'], C['GZ_MAX_CAP'], gp.LANDED, gp.END, gp.BAD, gp.FULL, gp.SHORT,
                                     ctypes.sizeof(GzJob), 16, ctypes.sizeof(GzResult)]
    assert (C['GZ_FIND_KEEP'], C['GZ_MARGIN'], C['GZ_MAX_REPAIRS'], C['GZ_MAX_CAP'], C['KV_CRC_SLICE']) == (4, 4 << 20, 200, 0x7ffffff0, 16384)
    for ratio in (1.0, 3.2, 4.0, 25.6, 40.0):
        for bits in (0, 7, 8, 4096 * 8, 10 ** 7, 1 << 31, 1 << 40):
            assert lib.h_gz_room(ratio, bits) == gp.room(ratio, bits)
    assert gp.room(1.0, 0) == 8 + 16384 and gp.room(4.0, 800) == 1010 + 16384 and gp.room(40.0, 800) == 64 * 101 + 16384
    assert gp.room(4.0, 1 << 40) == C['GZ_MAX_CAP']


# ---------------------------------------------------------------- extent, starts, cuts, jobs
CHUNKS = (1024, 16384, 65536)
RATIOS = (1.0, 4.0, 40.0)
BOUNDARY = 256 * 8 * 37                                    # a bit on a 256-byte boundary
FILE_ENDS = ('in_segment', 'in_margin', 'beyond')


def file_size_of(kind, pos_bit, want_text, ratio, chunk):
    """a file that ends inside the segment, inside the margin behind it, or beyond the margin"""
    whole = gp.extent(pos_bit, 1 << 60, want_text, ratio, chunk)
    return {'in_segment': whole['seg_end'] - chunk // 3, 'in_margin': whole['seg_end'] + C['GZ_MARGIN'] // 2, 'beyond': whole['seg_end'] + 3 * C['GZ_MARGIN']}[kind]


def test_extent_is_the_rule(lib):
    seen = set()
    for chunk in CHUNKS:
        for pos_bit in range(BOUNDARY - 9, BOUNDARY + 10):                 # every bit phase on either side of the boundary
            for ratio in RATIOS:
                for want_text in (0, 100000, 3000000):
                    for kind in FILE_ENDS:
                        args = (pos_bit, file_size_of(kind, pos_bit, want_text, ratio, chunk), want_text, ratio, chunk)
                        got = c_extent(lib, args)
                        assert got == gp.extent(*args), args
                        assert got['first_byte'] % 256 == 0 and 0 <= got['start_rel'] < 256 * 8
                        assert got['first_byte'] * 8 + got['start_rel'] == pos_bit
                        assert got['seg_end'] <= got['upto'] <= args[1] and got['upto'] - got['seg_end'] <= C['GZ_MARGIN']
                        assert got['n_chunks'] * chunk >= got['n_bytes'] > (got['n_chunks'] - 1) * chunk
                        assert (got['to_file_end'], got['is_file_end']) == {'in_segment': (1, 1), 'in_margin': (0, 1), 'beyond': (0, 0)}[kind]
                        if kind == 'beyond':
                            assert got['seg_end'] % chunk == 0 and got['seg_end'] - got['first_byte'] >= 4 * chunk
                        seen.add((got['to_file_end'], got['is_file_end'], got['start_rel'] % 8))
    assert len(seen) == 3 * 8


def candidate_lists(x, rng):
    """name -> what k_gz_find could have kept: GZ_FIND_KEEP per chunk, ~0 where it kept none"""
    keep, n = C['GZ_FIND_KEEP'], x['n_chunks'] * C['GZ_FIND_KEEP']
    chunk_bits = 8 * (-(-x['n_bytes'] // x['n_chunks']))

    def placed(bits):
        out = [NONE] * n
        used = {}
        for b in sorted(b for b in bits if b < x['n_bytes'] * 8):          # (k_gz_find reports places inside the buffer)
            c = min(b // chunk_bits, x['n_chunks'] - 1)
            if used.get(c, 0) < keep:
                out[c * keep + used.get(c, 0)] = b
                used[c] = used.get(c, 0) + 1
        return out
    inside = x['start_rel'] + (x['seg_end_rel'] - x['start_rel']) // 2
    many = sorted(rng.sample(range(1, x['n_bytes'] * 8), min(40, x['n_bytes'])))
    return {'none': [], 'all_absent': [NONE] * n, 'one': placed([inside]), 'equal_to_start': placed([x['start_rel'], inside]),
            'at_segment_end': placed([inside, x['seg_end_rel']]), 'behind_segment_end': placed([inside, x['seg_end_rel'] + 1, x['seg_end_rel'] + 999]),
            'many': placed(many)}


def found_for(guesses, starts, stop_rel, rng):
    """answers k_gz_sync could give: near the guess, none, at or in front of the header, behind the next start, behind the end, twice the same"""
    found = []
    for i, (header, guess) in enumerate(guesses):
        later = [s for s in starts if s > header]
        pick = rng.randrange(8)
        found.append({0: NONE, 1: header, 2: header - 1 if header else 0, 3: later[0] if later else guess + 5, 4: later[0] + 9 if later else guess + 7,
                      5: stop_rel if stop_rel != NONE else guess + 11}.get(pick, guess + rng.randrange(40)))
        if pick == 7 and i:
            found[-1] = found[-2]
    return found


def check_plan(plan, starts, headers, have_terminal, n_bytes):
    assert all(a < b for a, b in zip(starts, starts[1:])) and all(h <= s for h, s in zip(headers, starts))
    jobs = plan['jobs']
    assert len(jobs) == (len(starts) - 1 if have_terminal else len(starts)) >= 1
    at = 0
    for j, job in enumerate(jobs):
        assert (job['start_bit'], job['header_bit'], job['target_idx']) == (starts[j], headers[j], j + 1)
        assert job['out_off'] == at and 16384 < job['out_cap'] <= C['GZ_MAX_CAP']          # ranges back to back: disjoint, inside total_cap
        at += gp.round_up(job['out_cap'], 64)
    assert at == plan['total_cap'] and plan['repair_room'] == max(256 << 20, at // 4)
    assert plan['exact'] == int(any(h != s for h, s in zip(headers, starts)))


@pytest.mark.parametrize('kind', FILE_ENDS)
@pytest.mark.parametrize('chunk', CHUNKS)
def test_starts_cuts_and_jobs_are_the_rule(lib, chunk, kind):
    rng = random.Random(chunk + len(kind))
    seen = set()
    for pos_bit in (BOUNDARY - 1, BOUNDARY, BOUNDARY + 3):
        for ratio in RATIOS:
            want_text = 200000
            args = (pos_bit, file_size_of(kind, pos_bit, want_text, ratio, chunk), want_text, ratio, chunk)
            x = gp.extent(*args)
            for name, cand in candidate_lists(x, rng).items():
                want = gp.starts_of(x, cand)
                got = c_starts(lib, args, cand)
                assert got == want, (args, name)
                ok, starts, have_terminal, stop_rel = got
                assert starts[0] == x['start_rel'] and all(a < b for a, b in zip(starts, starts[1:]))
                assert have_terminal == (not x['to_file_end'] and starts[-1] >= x['seg_end_rel'] and len(starts) > 1)
                assert ok == bool(have_terminal or x['is_file_end'])
                if name == 'at_segment_end' and not x['to_file_end']:
                    assert have_terminal and stop_rel == x['seg_end_rel']
                seen.add((name, ok, have_terminal))
                if not ok:
                    continue
                for wanted, max_guesses in ((32 * 256, len(cand) * 7 + 8), (64, len(cand) * 7 + 8), (8, 3), (1, 8)):
                    guesses = c_guesses(lib, args, starts, have_terminal, wanted, max_guesses)
                    assert guesses == gp.cut_guesses(x, starts, have_terminal, wanted, max_guesses), (args, name, wanted)
                    assert len(guesses) <= max_guesses and all(sum(1 for g in guesses if g[0] == s) <= 7 for s in starts)
                    assert all(h in starts and h < g for h, g in guesses)
                    if len(starts) * 4 >= wanted * 3:
                        assert not guesses
                    found = found_for(guesses, starts, stop_rel, rng)
                    merged = c_merge(lib, starts, have_terminal, guesses, found)
                    assert merged == gp.merge_cuts(starts, have_terminal, guesses, found), (args, name, wanted)
                    m_starts, m_headers, taken = merged
                    assert m_starts[0] == x['start_rel'] and set(starts) <= set(m_starts) and len(m_starts) <= len(starts) + taken
                    assert (m_starts[-1] == stop_rel) == have_terminal or not have_terminal
                    plan = c_plan(lib, m_starts, m_headers, have_terminal, x['n_bytes'], ratio)
                    assert plan == gp.plan_jobs(m_starts, m_headers, have_terminal, x['n_bytes'], ratio)
                    check_plan(plan, m_starts, m_headers, have_terminal, x['n_bytes'])
                    seen.add(('cut', bool(guesses), bool(taken), bool(plan['exact'])))
    assert ('none', kind != 'beyond', False) in seen and ('all_absent', kind != 'beyond', False) in seen
    assert ('at_segment_end', True, kind != 'in_segment') in seen and ('cut', True, True, True) in seen and ('cut', False, False, False) in seen


# ---------------------------------------------------------------- the chain walk against a simulated stream
STEP = 9001                                                # bits between two block starts of the simulated stream
BLOCKS = [2000 + STEP * k for k in range(30)]
N_BYTES = (BLOCKS[-1] + STEP) // 8 + 1
RATIO = 4.0                                                # room for 10 symbols per compressed byte + 16384: 27 K symbols a block


def stream(name):
    """name -> (SimStream, starts, headers, have_terminal).  Every stream has false block starts, a true and a false cut, and a
    cut on a true symbol boundary that is listed as a block start (the wrong kind)."""
    jumps, members, poison = [], [], None
    true = {b: b for b in BLOCKS}
    true.update({BLOCKS[4] + 3000: BLOCKS[4], BLOCKS[4] + 6000: BLOCKS[4], BLOCKS[9] + 2500: BLOCKS[9], BLOCKS[12] + 4000: BLOCKS[12]})
    listed = {b: b for b in BLOCKS[:28]}
    del listed[BLOCKS[7]], listed[BLOCKS[8]]                                        # blocks the search missed: one stretch runs through them
    listed.update({BLOCKS[2] + 1234: BLOCKS[2] + 1234, BLOCKS[5] + 77: BLOCKS[5] + 77, BLOCKS[5] + 4000: BLOCKS[5] + 4000})       # false block starts
    listed.update({BLOCKS[4] + 3000: BLOCKS[4], BLOCKS[4] + 6000: BLOCKS[4]})       # true cuts
    listed[BLOCKS[9] + 5000] = BLOCKS[9]                                            # a false cut
    listed[BLOCKS[12] + 4000] = BLOCKS[12] + 4000                                   # a true symbol boundary, but not a block start
    listed[BLOCKS[14] + 100] = BLOCKS[13]                                           # a cut that names another block
    have_terminal, end_bit = True, BLOCKS[-1] + STEP - 50
    if name == 'to_the_end':
        have_terminal = False
        listed.update({BLOCKS[28]: BLOCKS[28], BLOCKS[29]: BLOCKS[29]})
    elif name == 'false_terminal':
        listed[BLOCKS[28] - 500] = BLOCKS[28] - 500                                 # the decoder lands on the block boundary behind it
        del listed[BLOCKS[27]]
    elif name == 'full':
        jumps = [(BLOCKS[3] + 10, 400000), (BLOCKS[16] + 10, 1200000), (BLOCKS[4] + 4000, 50000)]      # one retry; a retry of a retry; a cut stretch
    elif name == 'members':
        have_terminal = False
        listed.update({BLOCKS[28]: BLOCKS[28], BLOCKS[29]: BLOCKS[29]})
        members = [(BLOCKS[6] - 300, 0xdeadbeef, 1111), (BLOCKS[11] - 300, 0x01020304, 0xfffffff0), (BLOCKS[20] - 300, 5, 6), (end_bit, 7, 8)]
    elif name == 'two_members_in_a_stretch':
        members = [(BLOCKS[8] - 300, 11, 100), (BLOCKS[8] - 200, 12, 200), (BLOCKS[8] - 100, 13, 0xffffffff)]
    elif name == 'full_then_members':
        jumps = [(BLOCKS[7] + 10, 600000)]
        members = [(BLOCKS[8] - 300, 21, 31)]
    elif name in ('bad', 'short'):
        poison = (BLOCKS[10] + 321, gp.BAD if name == 'bad' else gp.SHORT)
    elif name in ('bad_in_a_dropped_stretch',):
        poison = (BLOCKS[2] + 2000, gp.BAD)                                         # the true stretch from BLOCKS[2] meets it as well
    else:
        assert name == 'plain'

    def text_at(bit):
        return bit * 5 // 8 + sum(size for at, size in jumps if bit >= at)
    starts = sorted(listed)
    return gp.SimStream(true, text_at, end_bit, members, poison), starts, [listed[s] for s in starts], have_terminal


STREAMS = ('plain', 'to_the_end', 'false_terminal', 'full', 'members', 'two_members_in_a_stretch', 'full_then_members')


def both_walks(lib, name):
    out = []
    for walk in (lambda *a: c_walk(lib, *a), gp.walk_chain):
        sim, starts, headers, have_terminal = stream(name)
        stop_rel = starts[-1] if have_terminal else NONE
        out.append((walk(starts, headers, have_terminal, N_BYTES, RATIO, sim.decoder(starts, headers, stop_rel)), sim))
    (got, sim), (want, sim_py) = out
    assert got == want and sim.log == sim_py.log
    return got, sim, starts, headers, have_terminal


@pytest.mark.parametrize('name', STREAMS)
def test_walk_on_a_simulated_stream(lib, name):
    got, sim, starts, headers, have_terminal = both_walks(lib, name)
    plan = gp.plan_jobs(starts, headers, have_terminal, N_BYTES, RATIO)
    n_first, total_cap = len(plan['jobs']), plan['total_cap']
    assert 24 <= n_first <= 40 and got['fail'] == gp.WALK_OK
    assert [job for job, _ in sim.log[:n_first]] == plan['jobs'] and len(sim.log) == n_first + got['repairs']
    # the accepted stretches tile the text, each begins where the one before ended, none began at a false start
    final = {}
    for job, result in sim.log:
        if result['status'] != gp.FULL:
            final[job['out_off']] = (job, result)              # (a retry writes over the room of the retry that failed)
    accepted = [final[off] for off, _, _ in got['v']]
    at, bit = 0, starts[0]
    for (off, n, base), (job, result) in zip(got['v'], accepted):
        assert (base, n) == (at, result['n_out']) and job['start_bit'] == bit and sim.true.get(bit) == job['header_bit']
        at, bit = at + n, result['end_bit']
    assert at == got['text'] == sim.text_at(got['end_rel']) - sim.text_at(starts[0]) and bit == got['end_rel']
    stop_rel = starts[-1] if have_terminal else NONE
    assert got['ended'] == int(not have_terminal) and (got['end_rel'] == sim.end_bit if got['ended'] else got['end_rel'] >= stop_rel and sim.true[got['end_rel']] == got['end_rel'])
    # what was decoded and is not in the text: the stretches from false starts, and every attempt that ran out of room
    false_jobs = sum(1 for job, _ in sim.log if sim.true.get(job['start_bit']) != job['header_bit'])
    full = [i for i, (_, result) in enumerate(sim.log) if result['status'] == gp.FULL]
    assert n_first + got['repairs'] - len(got['v']) == false_jobs + len(full) and false_jobs >= 6 and got['repairs'] == len(full)
    # a retry has 32 times the room, behind the first launch's; the room of a retry that failed is used again; nothing accepted overlaps
    for i in full:
        job = sim.log[i][0]
        retry = next(j for j, _ in sim.log[max(i + 1, n_first):] if j['start_bit'] == job['start_bit'])
        assert retry == dict(job, out_cap=min(job['out_cap'] * 32, C['GZ_MAX_CAP']), out_off=retry['out_off']) and retry['out_off'] >= total_cap
        if i >= n_first:
            assert retry['out_off'] == job['out_off']
    ranges = sorted((job['out_off'], job['out_off'] + gp.round_up(job['out_cap'], 64)) for job, _ in accepted)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] <= total_cap + plan['repair_room']
    for job, _ in sim.log[n_first:]:
        lo, hi = job['out_off'], job['out_off'] + gp.round_up(job['out_cap'], 64)
        assert all(hi <= a or b <= lo for (other, _) in accepted for a, b in [(other['out_off'], other['out_off'] + gp.round_up(other['out_cap'], 64))]
                   if other['start_bit'] != job['start_bit'])
    # member ends as (text offset, CRC-32), the ISIZE sum, and the CRC chain given up where a stretch passed two trailers
    first_of_stretch, lost = [], False
    for job, result in accepted:
        inside = [m for m in sim.member_ends if job['start_bit'] < m[0] <= result['end_bit']]
        if inside:
            first_of_stretch.append((sim.text_at(inside[0][0]) - sim.text_at(starts[0]), inside[0][1]))
        lost = lost or len(inside) > 1
    assert got['ends'] == first_of_stretch and got['crc_lost'] == int(lost)
    assert got['isize_seg'] == sum(m[2] for m in sim.member_ends if m[0] <= got['end_rel']) & 0xffffffff
    expect = {'full': (4, False, 0), 'members': (0, False, 4), 'two_members_in_a_stretch': (0, True, 1), 'full_then_members': (1, False, 1)}.get(name, (0, False, 0))
    assert (got['repairs'], bool(got['crc_lost']), len(got['ends'])) == expect


@pytest.mark.parametrize('name', ['bad', 'short', 'bad_in_a_dropped_stretch'])
def test_walk_reports_what_a_decoder_met(lib, name):
    got, sim, starts, headers, _ = both_walks(lib, name)
    at, status = sim.poison
    assert (got['fail'], got['fail_bit']) == (gp.WALK_BAD if status == gp.BAD else gp.WALK_SHORT, at)
    last = max(s for s, h in zip(starts, headers) if s <= at and sim.true.get(s) == h)       # where the stretch that met it began
    assert got['ended'] == 0 and got['v'] and got['text'] == sim.text_at(last) - sim.text_at(starts[0])


def scripted(answers, log):
    """a decoder that answers job after job from a list (the last answer again when the list is spent)"""
    def decode(job):
        answer = answers[min(len(log), len(answers) - 1)]
        answer = answer(job) if callable(answer) else answer
        log.append(job)
        return dict({'n_out': 0, 'members': 0, 'isize_sum': 0, 'trailer_at': 0, 'trailer_crc': 0}, **answer)
    return decode


def walk_both_scripted(lib, starts, headers, have_terminal, n_bytes, answers):
    logs = [], []
    got = c_walk(lib, starts, headers, have_terminal, n_bytes, RATIO, scripted(answers, logs[0]))
    assert got == gp.walk_chain(starts, headers, have_terminal, n_bytes, RATIO, scripted(answers, logs[1])) and logs[0] == logs[1]
    return got, logs[0]


def test_walk_gives_up_after_200_repairs(lib):
    """every repair lands on a block nobody began at, 1000 bits on: the 201st is one too many"""
    starts = [100, 10 ** 6]
    for n_landings, fail in ((200, gp.WALK_OK), (201, gp.WALK_REPAIRS)):
        answers = [(lambda job: {'status': gp.LANDED, 'end_bit': job['start_bit'] + 1000, 'n_out': 10})] * n_landings + [{'status': gp.LANDED, 'end_bit': 10 ** 6}]
        got, log = walk_both_scripted(lib, starts, starts, True, 200000, answers)
        assert (got['fail'], got['repairs']) == (fail, min(n_landings, 201)) and len(log) == min(n_landings, 200) + 1
        # every landing was accepted before the stretch behind it was asked for
        assert len(got['v']) == n_landings + (fail == gp.WALK_OK) and got['text'] == 10 * n_landings
        if fail:
            assert got['fail_bit'] == log[-1]['start_bit'] == 100 + 1000 * 200


def test_walk_gives_up_when_the_repair_room_is_spent(lib):
    """GZ_FULL again and again: 32 times the room each time, until that is more than the repairs' room"""
    starts = [100, 80000]
    got, log = walk_both_scripted(lib, starts, starts, True, 20000, [{'status': gp.FULL, 'end_bit': 0}])
    cap = gp.room(RATIO, 80000 - 100)
    total_cap = gp.round_up(cap, 64)
    assert [(j['out_cap'], j['out_off']) for j in log] == [(cap, 0), (32 * cap, total_cap), (1024 * cap, total_cap)]
    assert gp.round_up(1024 * cap, 64) <= 256 << 20 < 32768 * cap
    assert (got['fail'], got['fail_bit'], got['repairs'], got['v']) == (gp.WALK_REPAIRS, 100, 3, [])


def test_walk_gives_up_on_a_stretch_that_has_all_the_room_there_is(lib):
    n_bytes = 300 << 20
    got, log = walk_both_scripted(lib, [100], [100], False, n_bytes, [{'status': gp.FULL, 'end_bit': 0}])
    assert [j['out_cap'] for j in log] == [C['GZ_MAX_CAP']]
    assert (got['fail'], got['fail_bit'], got['repairs']) == (gp.WALK_REPAIRS, 100, 1)


def test_walk_repairs_a_landing_on_nobodys_start(lib):
    """GZ_LANDED in front of stop_rel on a bit that is no start: the stretch counts, and a stretch of its own begins there -- a block
    start (header_bit == start_bit) whose target is the first start behind it"""
    starts, headers = [100, 5000, 9000, 20000, 31000, 50000], [100, 5000, 5000, 20000, 31000, 50000]
    answers = [{'status': gp.LANDED, 'end_bit': 5000, 'n_out': 7}, {'status': gp.LANDED, 'end_bit': 12345, 'n_out': 8}, {'status': gp.LANDED, 'end_bit': 20000, 'n_out': 1},
               {'status': gp.LANDED, 'end_bit': 31000, 'n_out': 9}, {'status': gp.LANDED, 'end_bit': 50000, 'n_out': 10},
               lambda job: {'status': gp.LANDED, 'end_bit': 31000, 'n_out': 11}]
    got, log = walk_both_scripted(lib, starts, headers, True, 10000, answers)
    plan = gp.plan_jobs(starts, headers, True, 10000, RATIO)
    repair = log[5]
    assert repair == {'start_bit': 12345, 'header_bit': 12345, 'target_idx': 3, 'out_off': plan['total_cap'], 'out_cap': gp.room(RATIO, 20000 - 12345)}
    assert (got['fail'], got['repairs'], got['end_rel'], got['text']) == (gp.WALK_OK, 1, 50000, 7 + 8 + 11 + 10)
    assert [v[0] for v in got['v']] == [0, plan['jobs'][1]['out_off'], plan['total_cap'], plan['jobs'][4]['out_off']]


# ---------------------------------------------------------------- CRC ranges
S = C['KV_CRC_SLICE']
TEXTS = (0, 1, S - 1, S, S + 1, 3 * S, 5 * S + 17)


def end_lists(text):
    return {'none': [], 'at_the_end': [text], 'in_the_middle': [text // 2], 'empty_member': [text // 2, text // 2], 'empty_at_0': [0, text // 2],
            'empty_at_0_only': [0], 'empty_at_the_end': [text, text], 'many': sorted({0, text // 3, text // 2, S, text} & set(range(text + 1))) + [text]}


@pytest.mark.parametrize('text', TEXTS)
def test_crc_ranges(lib, text):
    for name, ends in end_lists(text).items():
        cap = text // S + 2 * len(ends) + 4
        out = (U64 * (3 * cap))()
        n = lib.h_gz_crc_ranges(text, u64s(ends), len(ends), S, out, cap)
        assert n <= cap
        got = [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(n)]
        assert got == gp.crc_ranges(text, ends, S), (text, name)
        at, closed = 0, 0
        for start, length, closes in got:
            assert start == at and length <= S
            at += length
            if closes:
                assert closes == closed + 1 and ends[closes - 1] == at          # the ends 1..n once each, in order, where they are
                closed = closes
            else:
                assert length > 0
            if length == 0:
                assert closes and (closes >= 2 and ends[closes - 2] == at or at == 0)      # an empty member: an empty range closes it
        assert at == text and closed == len(ends), (text, name)
        assert sum(1 for r in got if r[1] == 0) == sum(1 for i, e in enumerate(ends) if e == (ends[i - 1] if i else 0))
