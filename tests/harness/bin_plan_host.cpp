// Host-side harness for kevlar_amd/csrc/kv_bin_plan.h (compiled as plain C++ by tests/test_bin_plan.py): the shape, the sizes and
// stage B's LDS layout of the partitioned count behind a C ABI, so that Python can hold them to the case table and to a
// restatement of the rules.
#include <stdint.h>
#include <string.h>
#include "../../kevlar_amd/csrc/kv_bin_plan.h"

extern "C" {
// out[0 .. 13]: the constants in the order of tests/test_bin_plan.py's CONSTANTS
void h_bin_constants(uint64_t *out)
{
    const uint64_t c[14] = {BIN_C, BIN_MAX_T, BIN_MAX_F, BIN_SLICE_BITS, BIN_W_SHIFT, BIN_W_MAX, BIN_RING_MIN, BIN_RING_MAX, BIN_B_THREADS, BIN_B_BUDGET,
                            BIN_C_THREADS, BIN_MAX_SEG, BIN_LIST_ROUNDS, BIN2_TILES};
    memcpy(out, c, sizeof(c));
}

// out[0 .. 9]: maxsl, cmax, F, C, recipF, ringB, threadsA, pmin, pmax, T; nslices[0 .. T)
void h_bin_shape(const uint64_t *size, int T, int weighted, uint64_t *out, uint64_t *nslices)
{
    const BinShape sh = bin_shape(size, T, weighted != 0);
    const uint64_t v[10] = {sh.maxsl, (uint64_t)sh.cmax, (uint64_t)sh.F, (uint64_t)sh.C, sh.recipF, sh.ringB, sh.threadsA, sh.pmin, sh.pmax, (uint64_t)sh.T};
    memcpy(out, v, sizeof(v));
    for (int t = 0; t < T && t < BIN_MAX_T; ++t) nslices[t] = sh.nslices[t];
}

// out[0 .. 13]: nwgA, nwgB, quotaA, cap1, cap2, spill_cap, the six byte sizes in carve order, their total, fast4
void h_bin_sizes(const uint64_t *size, int T, int weighted, uint64_t n_items_max, int nbands, int use_mask, uint64_t work_units, uint32_t nwgA_fixed, int cus,
                 uint64_t *out)
{
    const BinSizes z = bin_sizes(bin_shape(size, T, weighted != 0), n_items_max, nbands, use_mask != 0, work_units, nwgA_fixed, weighted != 0, cus);
    const uint64_t v[14] = {z.nwgA, z.nwgB, z.quotaA, z.cap1, z.cap2, z.spill_cap, z.b_buf1, z.b_buf2, z.b_cnt1, z.b_cnt2, z.b_spill, z.b_ctr, z.b_total,
                            (uint64_t)z.fast4};
    memcpy(out, v, sizeof(v));
}

// out[0 .. 3]: the offsets of cnt, base and ready, and the total
void h_bin_split_lds(uint32_t F, uint32_t ringB, uint64_t item_bytes, uint64_t *out)
{
    const BinSplitLds l = bin_split_lds(F, ringB, (size_t)item_bytes);
    const uint64_t v[4] = {l.cnt, l.base, l.ready, l.total};
    memcpy(out, v, sizeof(v));
}
}
