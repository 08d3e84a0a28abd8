// kv_binned.h -- geometry and host entry points of the partitioned count (kv_binned.hip), shared with the
// super-k-mer front end (kv_skm.hip), which feeds the same coarse buckets with (bin, count) items.
#pragma once
#include "kv_internal.h"
#include "kv_bin_plan.h"   // the constants, the item layout and the planner's arithmetic

struct BinGeom {
    int T, F, C;                     // tables, slices per coarse bucket, coarse buckets in use (<= BIN_C)
    int sbits;                       // log2 of the bins per slice (BIN_SLICE_BITS)
    uint32_t ringB;                  // LDS ring entries per stream in stage B (a power of two)
    uint32_t recipF;                 // floor(2^32 / F) + 1: slice / F by multiply-high
    uint32_t nslices[BIN_MAX_T];
    uint32_t tile_lds;               // bytes of dynamic LDS stage A stages a tile of reads in
    uint32_t nwgA, nwgB;             // writers per coarse bucket (stage-A workgroups) / per slice (stage-B workgroups of the bucket)
    uint32_t quotaA;                 // work units (tiles / list chunks) one stage-A workgroup may take: bounds its segments' fill
    uint64_t cap1, cap2, spill_cap;  // items per PRIVATE segment: every writer owns its own region of every stream,
                                     // so appending needs no global atomic (and no round trip) at all
    uint32_t *gbuf1;                 // [T*C][nwgA][cap1] coarse items
    uint16_t *gbuf2;                 // [T*C*F][nwgB][cap2] fine items (u16, or u32 when weighted)
    uint32_t *gcnt1, *gcnt2;         // [T*C][nwgA] / [T*C*F][nwgB] items written per segment
    unsigned long long *spill;       // bin | table << 32 | (increment - 1) << 40
    unsigned long long *ctr;         // [0] spill count, [1] overflow flag, [2] k-mers added, [3] occupancy delta, [4] work ticket
    uint64_t tsize[BIN_MAX_T];       // table sizes and base pointers by value: stage C starts without a round trip to the descriptor
    uint8_t *ttab[BIN_MAX_T];
    int zero_tables;                 // the tables are all zero by decree (kv_sketch::lazy_zero): stage C writes every slice without loading it
    // fast4: four tables of 2^16 <= size < 2^31 bins each and less than 2^32 coarse-item slots in all: the super-k-mer count's drain then
    // takes h % size with the FP64 quotient and 32-bit remainders (the remainder's sign is bit 31) and appends its four items with 32-bit
    // index arithmetic; tmagic[t] = kv_fastmod_magic(size[t]) by value (no trip to the sketch's descriptor per k-mer)
    int fast4;
    uint64_t tmagic[BIN_MAX_T];
};

// host-side description of one partitioned count in flight
struct BinPlan {
    BinGeom g;
    int cmax;                // bucket budget the geometry was chosen for (<= 32: 512-thread stage A, else 1024)
    uint32_t threadsA;
    uint32_t maxsl;          // most slices of any table
    bool weighted;
};

#ifdef __HIPCC__
__device__ __forceinline__ void spill_item(const BinGeom &g, int t, uint64_t bin, uint32_t weight = 1u)
{
    const unsigned long long pos = atomicAdd(&g.ctr[0], 1ull);
    if (pos < g.spill_cap) g.spill[pos] = ((unsigned long long)(weight - 1u) << 40) | ((unsigned long long)t << 32) | bin;
    else g.ctr[1] = 1;
}
// the same for a whole wave at once: every lane calls, `live` lanes append their T items (one per table); ONE atomic on the
// shared counter per call.  (The counter is one address for the whole device: it takes ~90 updates per microsecond however
// they are issued -- an atomic per item, or per table, made the 9 M loose items of a k = 51 sample cost 2 ms.)
__device__ __forceinline__ void spill_items_wave(const BinGeom &g, const uint64_t *bins, uint32_t weight, bool live)
{
    const unsigned long long vote = __ballot(live);
    if (!vote) return;
    const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)vote) - 1;
    const unsigned long long T = (unsigned long long)g.T;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&g.ctr[0], (unsigned long long)__popcll(vote) * T);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, leader), hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), leader);
    base = (unsigned long long)lo | ((unsigned long long)hi << 32);
    if (live) {
        const unsigned long long first = base + (unsigned long long)__popcll(vote & ((1ull << lane) - 1ull)) * T;
#pragma unroll
        for (int t = 0; t < BIN_MAX_T; ++t) {
            if (t >= g.T) break;
            if (first + t < g.spill_cap) g.spill[first + t] = ((unsigned long long)(weight - 1u) << 40) | ((unsigned long long)t << 32) | bins[t];
            else g.ctr[1] = 1;
        }
    }
}
#endif

// A kernel instance together with its name: KV_INST-style macros (SKM_INST in kv_skm.hip, BIN_INST in kv_binned.hip) hand
// kv_inst a function pointer and the text of that very expression, so the name cannot drift from the kernel.  A launch takes its
// pointer from a function that notes the name in its stream's KvLaunched, and an entry point reports that list (blanks removed,
// comma separated; a comma between angle brackets belongs to a name).
template <typename F> struct KvInst { F *fn; const char *name; };
template <typename F> KvInst<F> kv_inst(F *fn, const char *name) { return KvInst<F>{fn, name}; }
struct KvLaunched {
    std::mutex mu;
    std::string names;
    void begin() { std::lock_guard<std::mutex> lk(mu); names.clear(); }
    void note(const char *name)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!names.empty()) names += ',';
        for (const char *c = name; *c; ++c) if (*c != ' ') names += *c;
    }
    // the list and its terminating zero into out[cap]; false when they do not fit
    bool report(char *out, uint64_t cap)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!out || names.size() + 1 > cap) return false;
        memcpy(out, names.c_str(), names.size() + 1);
        return true;
    }
};

bool kv_bin_two_bit(const kv_sketch *s, const kv_reads *reads);      // stage A can hash this batch from its 2-bit form (k_bin_hash_2bit)

// Geometry + scratch for a count of at most `n_items_max` k-mers into `s` on the calling thread's stream.
// work_units / threads: the stage-A front end's units of work and workgroup size (0 threads: pick by geometry);
// nwgA_fixed != 0 pins the number of stage-A writers (the super-k-mer front end brings its own grid).
// Every partitioned count begins here (kv_consume_binned's first step, and the super-k-mer count's before its S3): the stream's
// list of launched k_bin_* instances is emptied, and the plan is kept for kv_bin_last_plan.
int kv_bin_plan(kv_sketch *s, uint64_t n_items_max, int nbands, bool use_mask, uint64_t work_units, uint32_t lds_front,
                uint32_t nwgA_fixed, bool weighted, BinPlan *plan);
// stages B, C, spill + bookkeeping (n_occupied, n_unique estimate); synchronises the stream.
// n_added_fixed: the caller knows the number of k-mers added (hash lists), else it is read from ctr[2].
int kv_bin_finish(kv_sketch *s, BinPlan &plan, bool added_from_ctr, uint64_t n_added_fixed, uint64_t *n_added);
