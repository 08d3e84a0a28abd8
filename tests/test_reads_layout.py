"""CPU check of the layout planner of a read batch (kevlar_amd/csrc/kv_reads_layout.h): word offsets, tile table and
every scalar against a plain-Python restatement of the rule (tests/reads_layout_common.py).  A uniform batch planned without
tables has only its scalars to compare; that the arithmetic layout equals the rule's tables is shown on the Python restatement,
and the device writer of that layout (k_uniform_layout) is held to the oracle by tests/test_gpu_reads_build.py.

The header compiles for the host; tests/harness/reads_layout_host.cpp wraps it in a C ABI.  No GPU involved."""
import ctypes
import os
import subprocess

import pytest

import reads_layout_common as rl

ROOT = rl.ROOT
SRC = os.path.join(ROOT, 'tests', 'harness', 'reads_layout_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libreads_layout_host.so')
SCALARS = ('n_words', 'n_bases', 'max_len', 'tile_max_bases', 'n_tiles', 'uni_len', 'uni_per_tile')
C = rl.constants()
CASES = rl.cases(C)


@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in (SRC, rl.HDR, rl.API)):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_reads_plan.restype = ctypes.c_uint64
    L.h_reads_plan.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.h_reads_per_tile.restype = ctypes.c_uint32
    L.h_reads_per_tile.argtypes = [ctypes.c_uint32]
    return L


def run_plan(lib, lens, uniform_tables):
    """the planner's answer in the shape of rl.plan(); woff / tiles are None when the plan left them out"""
    n = len(lens)
    tile_cap = n + sum(x // C['KV_SEG_BASES'] + 1 for x in lens) + 1
    arr = (ctypes.c_uint32 * max(n, 1))(*lens)
    scalars = (ctypes.c_uint64 * 8)()
    woff = (ctypes.c_uint64 * (n + 1))()
    n_woff = ctypes.c_uint64()
    tiles = (ctypes.c_uint32 * (4 * tile_cap))()
    n_desc = lib.h_reads_plan(arr, n, int(uniform_tables), scalars, woff, n + 1, ctypes.byref(n_woff), tiles, tile_cap)
    assert n_desc <= tile_cap
    got = dict(zip(SCALARS, (int(v) for v in scalars)))
    assert int(scalars[7]) == (n_woff.value == 0)         # closed_form says that the tables were left out, and nothing else does
    got['woff'] = [int(v) for v in woff[:n_woff.value]] if n_woff.value else None
    got['tiles'] = [tuple(int(v) for v in tiles[4 * t:4 * t + 4]) for t in range(n_desc)] if n_desc else None
    assert (got['woff'] is None) == (got['tiles'] is None)
    return got


def test_harness_and_test_share_their_constants(lib):
    out = (ctypes.c_uint64 * 7)()
    lib.h_layout_constants(out)
    assert [int(v) for v in out] == [C['KV_TILE_LDS_BYTES'], C['KV_TILE_MAX_READS'], C['KV_READ_PAD'], C['KV_SEG_BASES'], C['KV_MAX_K'], 16, 8]
    # a segment tile stages up to KV_SEG_BASES + KV_MAX_K - 1 bases: they have to fit the budget the whole-read tiles fit
    assert rl.need(C, C['KV_SEG_BASES'] + C['KV_MAX_K'] - 1) <= rl.budget(C)


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_is_the_rule(lib, name):
    lens = CASES[name]
    want = rl.plan(C, lens)
    got = run_plan(lib, lens, True)
    assert got == want
    # tiles cover every read with bases exactly once, in order
    covered = []
    for first, count, seg_start, seg in got['tiles']:
        if seg:
            assert count == 1 and seg_start % C['KV_SEG_BASES'] == 0 and seg_start < lens[first]
            if seg_start == 0:
                covered.append(first)
        else:
            covered.extend(range(first, first + count))
    assert covered == list(range(len(lens)))
    # without tables on request: the same scalars; the tables are left out exactly when the batch is uniform
    short = run_plan(lib, lens, False)
    assert {k: short[k] for k in SCALARS} == {k: want[k] for k in SCALARS}
    if want['uni_len']:
        assert short['woff'] is None and short['tiles'] is None
        woff, tiles, per_tile = rl.closed_form(C, lens[0], len(lens))
        assert (woff, tiles, per_tile) == (want['woff'], want['tiles'], want['uni_per_tile'])     # Python's closed form against Python's loop
        assert lib.h_reads_per_tile(lens[0]) == per_tile
    else:
        assert (short['woff'], short['tiles']) == (want['woff'], want['tiles'])


def test_the_cases_sit_on_the_boundaries():
    """what the names in rl.cases() promise, whatever the constants are"""
    full, budget = C['KV_TILE_MAX_READS'], rl.budget(C)
    uniform = {name: rl.plan(C, lens)['uni_len'] != 0 for name, lens in CASES.items()}
    assert [n for n in sorted(uniform) if not uniform[n]] == sorted(['empty', 'one_empty_read', 'three_empty_reads', 'mixed', 'two_segments_just',
                                                                    'two_segments_full', 'three_segments', 'long_between_short', 'equal_but_segmented'])
    assert [rl.plan(C, CASES['std_x{}'.format(n)])['n_tiles'] for n in (1, full, full + 1, 2 * full + 1)] == [1, 1, 2, 3]
    assert rl.plan(C, CASES['budget_limited'])['uni_per_tile'] == budget // rl.need(C, CASES['budget_limited'][0]) < full
    assert rl.plan(C, CASES['budget_limited'])['n_tiles'] == 2
    assert rl.plan(C, CASES['longest_one_tile'])['tiles'] == [(0, 1, 0, 0)]
    assert [rl.plan(C, CASES[n])['n_tiles'] for n in ('two_segments_just', 'two_segments_full', 'three_segments')] == [2, 2, 3]
    assert [t[3] for t in rl.plan(C, CASES['long_between_short'])['tiles']] == [0, 1, 1, 1, 0]
    assert all(t[3] == 1 for t in rl.plan(C, CASES['equal_but_segmented'])['tiles'])
