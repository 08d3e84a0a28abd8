// kv_bin_plan.h -- the planner's arithmetic of the partitioned count (kv_binned.hip), free of HIP: its constants, the geometry a
// sketch's table sizes give (bin_shape), what a batch adds -- writers, quota, capacities, the carve of the staging arena, fast4
// (bin_sizes) -- and stage B's dynamic-LDS layout (bin_split_lds).  Plain C++17: tests/harness/bin_plan_host.cpp compiles it for the
// host, tests/test_bin_plan.py holds it to the case table of tests/bin_instances_common.py and to what the kernels rely on.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "kv_fastmod.h"

#define BIN_C 64            // most coarse buckets per table
#define BIN_MAX_T 4         // tables handled by the partitioned path
#define BIN_MAX_F 512       // slices per coarse bucket (9 bits of a coarse item)

// A coarse item (stage A -> stage B) is one u32.  Unweighted (one item per k-mer):
//   bits  0..15  offset of the bin inside its 65536-bin slice        bits 16..24  slice inside the coarse bucket (< F <= 512)
// Weighted (one item per distinct k-mer of a batch; saturating adds commute, so a k-mer seen c times is one item of
// weight c instead of c items): the same layout plus bits 25..31 = weight - 1.
// A fine item (stage B -> stage C) is the u16 offset, or for weighted items offset | weight << 16.
#define BIN_W_SHIFT 25
#define BIN_W_MAX 128u
#define BIN_SLICE_BITS 16

#define BIN_RING_MIN 64
#define BIN_RING_MAX 4096   // a round appends at most 4096 items to one stream
#define BIN_B_THREADS 512   // 8 waves: one lane per slice stream for F <= 512
#define BIN_B_BUDGET 16384  // LDS ring entries per stage-B workgroup
#define BIN_C_THREADS 1024
#define BIN_MAX_SEG 512     // stage-B writers per slice (nwgB)
#define BIN_LIST_ROUNDS 16  // list elements per thread and ticket of k_bin_list
#define BIN2_TILES 8u       // tiles' worth of reads per ticket of k_bin_hash_2bit

static inline uint64_t bin_round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// what the table sizes alone decide
struct BinShape {
    int T; uint64_t pmin, pmax;      // tables; the smallest and the largest
    uint32_t nslices[BIN_MAX_T], maxsl;      // slices of every table and the most of any
    int cmax, F, C;                  // bucket budget, slices per coarse bucket, coarse buckets in use
    uint32_t recipF;                 // floor(2^32 / F) + 1: slice / F by multiply-high (0 with F == 1: kernels take the slice as is)
    uint32_t ringB;                  // stage B's ring entries per slice stream
    uint32_t threadsA;               // stage A's workgroup size
};

static inline BinShape bin_shape(const uint64_t *size, int T, bool weighted)
{
    BinShape sh = {};
    sh.T = T; sh.pmin = UINT64_MAX; sh.maxsl = 1;
    for (int t = 0; t < T && t < BIN_MAX_T; ++t) {
        sh.pmin = std::min(sh.pmin, size[t]);
        sh.pmax = std::max(sh.pmax, size[t]);
        sh.nslices[t] = (uint32_t)((size[t] + (1ull << BIN_SLICE_BITS) - 1) >> BIN_SLICE_BITS);
        sh.maxsl = std::max(sh.maxsl, sh.nslices[t]);
    }
    // Coarse buckets per table: as few as keep stage B's fan-out F at <= 384 slices per bucket (its u16 rings then fit three
    // workgroups per CU), between 4 and 32 with 512-thread stage-A workgroups; 64 buckets / 1024 threads beyond 2^30 bins.  Fewer
    // buckets = fewer distinct lines per stage-A store instruction (that stage is bound by L2 write requests): measured per 525 M k-mers
    // into 5e8-bin tables, A/B/C = 10.5/5.0/4.0 ms with 32 buckets, 8.7/4.9/4.0 with 20, 8.3/6.1/4.0 with 16 (F = 478: rings too big).
    sh.cmax = sh.maxsl <= 32u * BIN_MAX_F ? (int)std::min<uint32_t>(32u, std::max<uint32_t>(4u, (sh.maxsl + 383u) / 384u)) : BIN_C;
    sh.F = (int)((sh.maxsl + (uint32_t)sh.cmax - 1) / (uint32_t)sh.cmax);
    sh.C = (int)((sh.maxsl + (uint32_t)sh.F - 1) / (uint32_t)sh.F);
    sh.recipF = sh.F == 1 ? 0u : (uint32_t)((1ull << 32) / (uint64_t)sh.F + 1);
    sh.ringB = weighted ? 32u : BIN_RING_MIN;                // budget in entries: u32 rings get half the entries per byte
    while (sh.ringB * 2 <= BIN_RING_MAX && (uint64_t)sh.ringB * 2 * sh.F <= BIN_B_BUDGET) sh.ringB *= 2;
    if (weighted) while (sh.ringB > 32u && (uint64_t)sh.ringB * sh.F * 4 > 2u * BIN_B_BUDGET) sh.ringB /= 2;
    sh.threadsA = sh.cmax <= 32 ? 512u : 1024u;
    return sh;
}

// what a batch adds: writers, quota, capacities, and the carve of the staging arena in the order of its regions.  bin_sizes takes
// work_units: the stage-A front end's units of work; nwgA_fixed != 0 pins the number of stage-A writers; cus: the device's compute units
struct BinSizes {
    uint32_t nwgA, nwgB;             // writers per coarse bucket (stage-A workgroups) / per slice (stage-B workgroups of the bucket)
    uint32_t quotaA;                 // work units one stage-A workgroup may take
    uint64_t cap1, cap2, spill_cap;  // items per private segment of stage A / stage B, entries of the spill list
    uint64_t b_buf1, b_buf2, b_cnt1, b_cnt2, b_spill, b_ctr, b_total;    // bytes, each a multiple of 256
    int fast4;                       // BinGeom::fast4 (kv_binned.h)
};

static inline BinSizes bin_sizes(const BinShape &sh, uint64_t n_items_max, int nbands, bool use_mask, uint64_t work_units, uint32_t nwgA_fixed,
                                 bool weighted, int cus)
{
    BinSizes z = {};
    const double expected = (double)(nbands > 0 && !use_mask ? n_items_max / (uint64_t)nbands + 1 : n_items_max);
    const uint64_t ns = (uint64_t)sh.T * sh.C;
    // writers: stage A = persistent workgroups (tiles dealt round-robin, so their loads are equal
    // to within one tile); stage B = nwgB workgroups per coarse bucket, ~256 k items each
    z.nwgA = nwgA_fixed ? nwgA_fixed : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(work_units, 1), (sh.cmax <= 32 ? 3u : 1u) * (uint32_t)cus);
    const uint64_t avg = (std::max<uint64_t>(work_units, 1) + z.nwgA - 1) / z.nwgA;
    z.quotaA = (uint32_t)std::min<uint64_t>(avg + avg / 2 + 1, 0xffffffffull);   // matches the 1.5x slack of cap1
    const double slice_bins = (double)(1u << BIN_SLICE_BITS);
    const double per_bucket = expected * std::min(1.0, (double)sh.F * slice_bins / (double)sh.pmin);
    const double per_slice = expected * std::min(1.0, slice_bins / (double)sh.pmin);
    const uint32_t most = std::min<uint32_t>(z.nwgA, BIN_MAX_SEG);
    z.nwgB = (uint32_t)std::max(1.0, std::min((double)most, std::ceil(per_bucket / 524288.0)));
    // a stage-B workgroup drains its segments one after the other, a dependent round trip or two each: with few items per
    // segment (a shard of a multi-GPU run, a small batch) that chain is the stage's whole time -- at most 32 segments each
    z.nwgB = std::max<uint32_t>(z.nwgB, std::min<uint32_t>(most, (z.nwgA + 31u) / 32u));
    const double m1 = per_bucket / z.nwgA, m2 = per_slice / z.nwgB;
    z.cap1 = bin_round_up((uint64_t)(m1 * 1.5 + 8.0 * std::sqrt(m1)) + 2048, 64);   // tiles are dealt dynamically: shares are uneven
    z.cap2 = bin_round_up((uint64_t)(m2 * 1.05 + 8.0 * std::sqrt(m2)) + 64, 64);
    z.spill_cap = std::max<uint64_t>(1u << 22, (uint64_t)(expected * sh.T / 8));
    z.b_buf1 = bin_round_up(ns * z.nwgA * z.cap1 * 4, 256), z.b_buf2 = bin_round_up(ns * sh.F * z.nwgB * z.cap2 * (weighted ? 4 : 2), 256);
    z.b_cnt1 = bin_round_up(ns * z.nwgA * 4, 256), z.b_cnt2 = bin_round_up(ns * sh.F * z.nwgB * 4, 256);
    z.b_spill = bin_round_up(z.spill_cap * 8, 256), z.b_ctr = 256;
    z.b_total = z.b_buf1 + z.b_buf2 + z.b_cnt1 + z.b_cnt2 + z.b_spill + z.b_ctr;
    // four tables of 2^16 <= size < 2^31 bins and less than 2^32 coarse-item slots in all
    z.fast4 = sh.T == 4 && ns * z.nwgA * z.cap1 < (1ull << 32) && kv_fastmod_fp(sh.pmin) && sh.pmax < (1ull << 31) ? 1 : 0;
    return z;
}

// Stage B's dynamic LDS, byte offsets: F rings of ringB items, the rings' append and flushed counters, a byte per thread (ready lists)
struct BinSplitLds { size_t cnt, base, ready, total; };
KVF_HD BinSplitLds bin_split_lds(uint32_t F, uint32_t ringB, size_t item_bytes)
{
    BinSplitLds l;
    l.cnt = ((size_t)F * ringB * item_bytes + 15) & ~(size_t)15;
    l.base = l.cnt + (size_t)F * 4;
    l.ready = l.base + (size_t)F * 4;
    l.total = l.ready + BIN_B_THREADS;
    return l;
}
