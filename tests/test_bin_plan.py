"""CPU check of the planner of the partitioned count (kevlar_amd/csrc/kv_bin_plan.h): the shape a sketch's table sizes give against
every geometry of the case table (tests/bin_instances_common.py), the sizes a batch adds -- writers, quota, capacities, the carve,
fast4 -- against a plain restatement of the rules, and at every point the conditions the kernels of kv_binned.hip rely on.

The header compiles for the host; tests/harness/bin_plan_host.cpp wraps it in a C ABI.  No GPU involved."""
import ctypes
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bin_instances_common import GEOMETRIES, SMALL, WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_bin_plan.h')
SRC = os.path.join(ROOT, 'tests', 'harness', 'bin_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libbin_plan_host.so')
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
CONSTANTS = ('BIN_C', 'BIN_MAX_T', 'BIN_MAX_F', 'BIN_SLICE_BITS', 'BIN_W_SHIFT', 'BIN_W_MAX', 'BIN_RING_MIN', 'BIN_RING_MAX', 'BIN_B_THREADS', 'BIN_B_BUDGET',
             'BIN_C_THREADS', 'BIN_MAX_SEG', 'BIN_LIST_ROUNDS', 'BIN2_TILES')
CUS = 256


def constants():
    """the #defines the rules are made of, read from the header"""
    text = open(HDR).read()
    return {name: int(re.search(r'#define\s+{}\s+(\d+)u?\b'.format(name), text).group(1)) for name in CONSTANTS}


K = constants()
SLICE = 1 << K['BIN_SLICE_BITS']

# (id, table sizes, (maxsl, cmax, F, C, ringB, threadsA) of u16 items, ringB of weighted items): every row of the case table
SHAPES = [(gid, primes, plan, ring_w) for gid, _, primes, plan, ring_w, _ in GEOMETRIES] + [('SMALL', SMALL['primes'], SMALL['plan'], SMALL['ring_w']),
                                                                                           ('WIDE', WIDE['primes'], WIDE['plan'], WIDE['ring_w'])]
# four tables: what fast4 turns on -- all of 2^16 <= size < 2^31, one below 2^16, one of exactly 2^31 bins
FOUR = [('four-small', SMALL['primes'] + [917467, 917459]), ('four-wide', WIDE['primes'] + [1073741783, 1073741741]), ('four-tiny', SMALL['primes'] + [917467, 65521]),
        ('four-2^31', SMALL['primes'] + [917467, 1 << 31])]


@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    headers = [HDR, os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_fastmod.h')]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + headers):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_bin_constants.argtypes = [ctypes.c_void_p]
    L.h_bin_shape.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.h_bin_sizes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, U64, ctypes.c_int, ctypes.c_int, U64, U32, ctypes.c_int, ctypes.c_void_p]
    L.h_bin_split_lds.argtypes = [U32, U32, U64, ctypes.c_void_p]
    return L


SHAPE_FIELDS = ('maxsl', 'cmax', 'F', 'C', 'recipF', 'ringB', 'threadsA', 'pmin', 'pmax', 'T')
SIZES_FIELDS = ('nwgA', 'nwgB', 'quotaA', 'cap1', 'cap2', 'spill_cap', 'b_buf1', 'b_buf2', 'b_cnt1', 'b_cnt2', 'b_spill', 'b_ctr', 'b_total', 'fast4')
CARVE = SIZES_FIELDS[6:12]


def shape_of(lib, sizes, weighted):
    out, nslices = (U64 * len(SHAPE_FIELDS))(), (U64 * K['BIN_MAX_T'])()
    lib.h_bin_shape((U64 * len(sizes))(*sizes), len(sizes), int(weighted), out, nslices)
    return dict(zip(SHAPE_FIELDS, (int(v) for v in out)), nslices=[int(v) for v in nslices[:len(sizes)]])


def sizes_of(lib, sizes, weighted, n_items, nbands, use_mask, work_units, nwgA_fixed, cus=CUS):
    out = (U64 * len(SIZES_FIELDS))()
    lib.h_bin_sizes((U64 * len(sizes))(*sizes), len(sizes), int(weighted), n_items, nbands, int(use_mask), work_units, nwgA_fixed, cus, out)
    return dict(zip(SIZES_FIELDS, (int(v) for v in out)))


def split_lds_of(lib, F, ringB, item_bytes):
    out = (U64 * 4)()
    lib.h_bin_split_lds(F, ringB, item_bytes, out)
    return dict(zip(('cnt', 'base', 'ready', 'total'), (int(v) for v in out)))


def round_up(v, m):
    return (v + m - 1) // m * m


def restate_sizes(sizes, sh, weighted, n_items, nbands, use_mask, work_units, nwgA_fixed, cus):
    """the sizes rules of kv_bin_plan.h in plain Python (its floats are the same doubles), on the shape of the case table"""
    T, F, C, pmin = len(sizes), sh['F'], sh['C'], min(sizes)
    expected = float(n_items // nbands + 1 if nbands > 0 and not use_mask else n_items)
    ns = T * C
    nwgA = nwgA_fixed if nwgA_fixed else min(max(work_units, 1), (3 if sh['cmax'] <= 32 else 1) * cus)
    avg = (max(work_units, 1) + nwgA - 1) // nwgA
    per_bucket = expected * min(1.0, float(F) * float(SLICE) / float(pmin))
    per_slice = expected * min(1.0, float(SLICE) / float(pmin))
    most = min(nwgA, K['BIN_MAX_SEG'])
    nwgB = int(max(1.0, min(float(most), float(math.ceil(per_bucket / 524288.0)))))
    nwgB = max(nwgB, min(most, (nwgA + 31) // 32))
    m1, m2 = per_bucket / nwgA, per_slice / nwgB
    z = dict(nwgA=nwgA, nwgB=nwgB, quotaA=min(avg + avg // 2 + 1, 0xffffffff),
             cap1=round_up(int(m1 * 1.5 + 8.0 * math.sqrt(m1)) + 2048, 64), cap2=round_up(int(m2 * 1.05 + 8.0 * math.sqrt(m2)) + 64, 64),
             spill_cap=max(1 << 22, int(expected * T / 8)))
    z.update(b_buf1=round_up(ns * nwgA * z['cap1'] * 4, 256), b_buf2=round_up(ns * F * nwgB * z['cap2'] * (4 if weighted else 2), 256),
             b_cnt1=round_up(ns * nwgA * 4, 256), b_cnt2=round_up(ns * F * nwgB * 4, 256), b_spill=round_up(z['spill_cap'] * 8, 256), b_ctr=256)
    z['b_total'] = sum(z[name] for name in CARVE)
    z['fast4'] = int(T == 4 and ns * nwgA * z['cap1'] < 1 << 32 and all(65536 <= size < 1 << 31 for size in sizes))
    return z


def test_harness_and_test_share_their_constants(lib):
    out = (U64 * len(CONSTANTS))()
    lib.h_bin_constants(out)
    assert [int(v) for v in out] == [K[name] for name in CONSTANTS]
    # what the rules and the kernels take for granted of them
    assert K['BIN_SLICE_BITS'] == 16 and K['BIN_MAX_F'] << K['BIN_SLICE_BITS'] == 1 << K['BIN_W_SHIFT'] and K['BIN_W_MAX'] == 1 << (32 - K['BIN_W_SHIFT'])
    assert K['BIN_MAX_F'] <= K['BIN_B_THREADS'] and K['BIN_MAX_SEG'] <= K['BIN_C_THREADS'] and K['BIN_RING_MIN'] * K['BIN_MAX_F'] * 2 <= 65536


def test_the_shape_is_what_the_case_table_says(lib):
    assert len(SHAPES) == 26
    for gid, primes, plan, ring_w in SHAPES:
        for weighted in (False, True):
            sh = shape_of(lib, primes, weighted)
            want = plan[:4] + (ring_w if weighted else plan[4],) + plan[5:]
            assert tuple(sh[name] for name in ('maxsl', 'cmax', 'F', 'C', 'ringB', 'threadsA')) == want, (gid, weighted)
            assert (sh['T'], sh['pmin'], sh['pmax']) == (len(primes), min(primes), max(primes)), gid
            assert sh['nslices'] == [(p + SLICE - 1) // SLICE for p in primes] and sh['maxsl'] == max(sh['nslices']), gid


def check_shape(sh, weighted, where):
    """what the kernels rely on of a shape"""
    F, C, ringB = sh['F'], sh['C'], sh['ringB']
    assert 1 <= F <= K['BIN_MAX_F'] <= K['BIN_B_THREADS'], where                # stage B: one lane per slice stream
    assert 1 <= C <= sh['cmax'] <= K['BIN_C'] and (C - 1) * F < sh['maxsl'] <= C * F, where
    assert ringB & (ringB - 1) == 0 and (32 if weighted else K['BIN_RING_MIN']) <= ringB <= K['BIN_RING_MAX'], where
    if F == 1:
        assert sh['recipF'] == 0, where                                        # the kernels take the slice as the bucket
    else:
        slices = np.arange(C * F, dtype=np.uint64)
        assert np.array_equal((slices * np.uint64(sh['recipF'])) >> np.uint64(32), slices // np.uint64(F)), where       # __umulhi(slice, recipF)
    assert (sh['threadsA'], sh['cmax'] <= 32) in ((512, True), (1024, False)), where


def check_sizes(sh, z, weighted, work_units, nwgA_fixed, where):
    """what the kernels rely on of a plan's sizes"""
    assert z['cap1'] % 64 == 0 and z['cap2'] % 64 == 0 and z['cap1'] >= 2048 and z['cap2'] >= 64, where
    assert 1 <= z['nwgB'] <= min(z['nwgA'], K['BIN_MAX_SEG']) and z['nwgB'] <= K['BIN_C_THREADS'], where
    assert z['nwgA'] == nwgA_fixed or (nwgA_fixed == 0 and 1 <= z['nwgA'] <= max(work_units, 1)), where
    assert z['quotaA'] * z['nwgA'] >= work_units, where
    # the carve: every region begins on a multiple of 256 bytes, holds what is stored in it, and the regions are the whole arena
    ns, at = sh['T'] * sh['C'], 0
    for name in CARVE:
        assert at % 256 == 0 and z[name] % 256 == 0, (where, name)
        at += z[name]
    assert at == z['b_total'], where
    assert z['b_buf1'] >= ns * z['nwgA'] * z['cap1'] * 4 and z['b_buf2'] >= ns * sh['F'] * z['nwgB'] * z['cap2'] * (4 if weighted else 2), where
    assert z['b_cnt1'] >= ns * z['nwgA'] * 4 and z['b_cnt2'] >= ns * sh['F'] * z['nwgB'] * 4 and z['b_spill'] >= z['spill_cap'] * 8 and z['b_ctr'] >= 5 * 8, where


def check_split_lds(lib, sh, weighted, where):
    item = 4 if weighted else 2
    F, ringB = sh['F'], sh['ringB']
    lay = split_lds_of(lib, F, ringB, item)
    assert lay['cnt'] % 16 == 0 and F * ringB * item <= lay['cnt'] < F * ringB * item + 16, where
    assert (lay['base'], lay['ready'], lay['total']) == (lay['cnt'] + 4 * F, lay['cnt'] + 8 * F, lay['cnt'] + 8 * F + K['BIN_B_THREADS']), where
    # what kv_bin_finish passes to the launch: the rings rounded up to 16 bytes, two counters a ring, a byte a thread
    assert lay['total'] == round_up(F * ringB * item, 16) + F * 2 * 4 + K['BIN_B_THREADS'], where


def test_the_sizes_are_what_the_rules_say_and_what_the_kernels_rely_on(lib):
    points = 0
    for gid, primes, plan, ring_w in SHAPES + [(name, sizes, None, None) for name, sizes in FOUR]:
        for weighted in (False, True):
            sh = shape_of(lib, primes, weighted)
            check_shape(sh, weighted, (gid, weighted))
            check_split_lds(lib, sh, weighted, (gid, weighted))
            cmax_cus = (3 if sh['cmax'] <= 32 else 1) * CUS
            for work_units, nbands, use_mask, nwgA_fixed, n_items in itertools.product((1, CUS - 1, 3 * CUS, 3 * CUS + 1, 100000), (0, 4), (False, True), (0, 7, 600),
                                                                                       (1, 1 << 22, 1 << 30)):
                where = (gid, weighted, work_units, nbands, use_mask, nwgA_fixed, n_items)
                z = sizes_of(lib, primes, weighted, n_items, nbands, use_mask, work_units, nwgA_fixed)
                assert z == restate_sizes(primes, sh, weighted, n_items, nbands, use_mask, work_units, nwgA_fixed, CUS), where
                check_sizes(sh, z, weighted, work_units, nwgA_fixed, where)
                if not nwgA_fixed:
                    assert z['nwgA'] == min(work_units, cmax_cus), where
                points += 1
    assert points == (26 + len(FOUR)) * 2 * 5 * 2 * 2 * 3 * 3


def test_fast4_takes_four_tables_below_2_31_bins_and_32_bit_slots(lib):
    verdict = {name: {n: sizes_of(lib, sizes, True, n, 0, False, 3 * CUS, 600)['fast4'] for n in (1 << 22, 1 << 30)} for name, sizes in FOUR}
    assert verdict['four-small'] == {1 << 22: 1, 1 << 30: 0}            # 2^30 items: more than 2^32 coarse-item slots
    assert verdict['four-wide'][1 << 22] == 1
    assert verdict['four-tiny'] == {1 << 22: 0, 1 << 30: 0} and verdict['four-2^31'] == {1 << 22: 0, 1 << 30: 0}
    assert all(sizes_of(lib, primes, True, 1 << 22, 0, False, 3 * CUS, 600)['fast4'] == 0 for _, primes, _, _ in SHAPES)     # two tables


def test_multiply_high_divides_by_every_f(lib):
    """recipF = floor(2^32 / F) + 1 gives slice / F for every slice a coarse item can name, whatever the table sizes"""
    slices = np.arange(K['BIN_C'] * K['BIN_MAX_F'], dtype=np.uint64)
    for F in range(2, K['BIN_MAX_F'] + 1):
        recip = (1 << 32) // F + 1
        assert recip < 1 << 32 and np.array_equal((slices * np.uint64(recip)) >> np.uint64(32), slices // np.uint64(F)), F
