// kv_assemble.hip -- per-partition unitigs for `kevlar assemble`, thousands of partitions in one call.
// The rule, per partition, with K odd and a threshold min_count:
//   (1) keys: the canonical 2-bit key of every window of K bases of every read (the encoding and order of kv_localize.hip); equal
//       (partition, key) pairs are grouped in ONE open-addressing table for the batch whose slots hold (hash tag, id of the first
//       window that claimed the pair) -- a match is the full key and the claiming window's partition, never the hash -- and counted;
//   (2) degrees: a key with count >= min_count is solid; its four successors and four predecessors are looked up once and kept as an
//       8-bit mask, so a walk step is one probe and one mask;
//   (3) heads: an oriented node whose incoming edge is not simple (|succ(w)| = 1 and |pred(v)| = 1 make w -> v simple) starts a unitig;
//       heads are counted per chunk of ASM_THREADS windows, the chunks' counts go through the one prefix sum and every chunk
//       writes its heads, in window order, behind its base;
//   (4) walk, twice: a lane per head follows simple edges and learns the length; of a unitig S and its reverse complement the one
//       whose first K-mer is smaller is kept (they differ there unless S is its own reverse complement, and then both are one head);
//       a prefix sum over the kept lengths gives exact offsets and the second walk writes the bases.
// A walk from a head cannot loop (entering a cycle takes a node with two predecessors); the guard of 2 * windows + 2 steps per
// partition only bounds a walk over damaged memory.  A component of simple edges alone is a cycle without a head: no output, counted.
// Cleaning (rules 3a to 3c, kv_assemble_clean_batch with a limit above 0) runs rounds in front of (3): every round computes degrees
// and heads of the LIVE keys, a lane per head measures its unitig (k_asm_measure), a lane per head decides whether it is a tip or
// a beaten bubble arm from those records alone (k_asm_decide), and a LATER launch marks the keys of the flagged unitigs dead
// (k_asm_kill): nothing that walks or probes liveness runs beside the marking, so a round's answer does not depend on scheduling.
// Liveness is a word of its own: the counts stay what the reads gave.
#include <algorithm>
#include <vector>

#include "kv_device.h"
#include "kv_roll2bit_device.h"
#include "kv_asm_plan.h"

namespace {

#define ASM_EMPTY32 0xFFFFFFFFu
#define ASM_EMPTY64 0xFFFFFFFFFFFFFFFFull
#define ASM_SOLID 0x100u                    // info: bits 0-3 successors by base, 4-7 predecessors by base, of the key as stored
#define ASM_HEAD0 0x200u                    // the key as stored starts a unitig
#define ASM_HEAD1 0x400u                    // its reverse complement does
#define ASM_DEFAULT_BUDGET (4ull << 30)

struct AsmDev {
    const uint8_t *bases;
    const uint64_t *roff, *wpre, *cpre;     // per read: first base, windows in front, runs in front
    const uint32_t *rpart;                  // per read: partition, counted from the launch's first
    const uint32_t *guard;                  // per partition: most steps of a walk
    uint64_t n_reads, n_windows, n_runs;
    int K;
    uint32_t min_count;
    uint64_t *keys;
    uint32_t *grp, *wpart, *cnt, *info;
    uint32_t *ccount;                       // per chunk of ASM_THREADS windows: heads
    const uint64_t *hbase;                  // per chunk: heads in front
    unsigned long long *table;
    uint64_t capmask;
    unsigned long long *ctr;                // [0] valid windows [1] distinct [2] solid [3] unitigs [4] live keys on a unitig
                                            // [5] tips removed [6] their keys [7] arms removed [8] their keys [9] = [6] + [8]
    uint32_t *pcount;                       // per partition: unitigs
    uint64_t n_heads;
    uint32_t *heads, *klen, *kflag;         // per head: 2 * window + strand; bases if kept, else 0; kept
    const uint64_t *ubase, *uidx;           // per head: first output byte, output index
    uint8_t *out;
    uint64_t *uoff;
    uint32_t *upart;
    uint64_t out_base;
    uint32_t part0;
    // cleaning; dead is null without it
    uint32_t *dead;                         // per window: 1 once the key it owns was removed
    uint32_t *hinv;                         // per 2 * window + strand of a head: its index in heads
    uint32_t count_pass;                    // k_asm_degree adds to ctr[1] and ctr[2]: the first degree pass of a launch only
    uint32_t tip_nodes, bubble_nodes;
    uint32_t *rm, *rpq, *rlast, *rpcode, *rqcode, *rflag;   // per head: nodes; P | Q << 4 (masks by base); last node, the one node of P,
    uint64_t *rsum;                                         // the one node of Q as 2 * window + strand or ASM_EMPTY32; verdict; sum of counts
};
#define ASM_CTR_BYTES 128
#define ASM_FLAG_TIP 1u
#define ASM_FLAG_ARM 2u
#define ASM_FLAG_MARKS 4u                   // of a unitig's two heads the one that counts it and marks its keys

template <int W>
__device__ __forceinline__ uint64_t asm_hash(const uint64_t *key, uint32_t part)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ ((uint64_t)part * 0xd6e8feb86659fd93ull);
#pragma unroll
    for (int w = 0; w < W; ++w) h = fmix64(h ^ key[w]) + 0x632be59bd9b4e019ull * (uint64_t)(w + 1);
    return h;
}

// the canonical key of the rolled window; 1 when it is the reverse complement's (K is odd: the two never tie)
template <int W>
__device__ __forceinline__ uint32_t asm_canonical(const LocRoll<W> &roll, uint64_t *key)
{
    bool f_less = true, decided = false;
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (!decided && roll.f[w] != roll.r[w]) { f_less = roll.f[w] < roll.r[w]; decided = true; }
#pragma unroll
    for (int w = 0; w < W; ++w) key[w] = f_less ? roll.f[w] : roll.r[w];
    return f_less ? 0u : 1u;
}

template <int W>
__device__ __forceinline__ void asm_flip(LocRoll<W> &roll)
{
#pragma unroll
    for (int w = 0; w < W; ++w) { const uint64_t t = roll.f[w]; roll.f[w] = roll.r[w]; roll.r[w] = t; }
}

// a base in front of the window instead of behind it: the reverse complement takes the complement behind
template <int W>
__device__ __forceinline__ void asm_push_front(LocRoll<W> &roll, uint32_t c, int topbits)
{
    asm_flip(roll);
    roll.push(3u - c, topbits);
    asm_flip(roll);
}

// base j of a key of K bases (0: the first, most significant)
template <int W>
__device__ __forceinline__ uint32_t asm_base(const uint64_t *key, int K, int j)
{
    const int bit = 2 * (K - 1 - j);
    return (uint32_t)(key[W - 1 - (bit >> 6)] >> (bit & 63)) & 3u;
}

// the window whose forward key is `key`, as strand 0, or its reverse complement, as strand 1
template <int W>
__device__ __forceinline__ void asm_load(LocRoll<W> &roll, const uint64_t *key, int K, int topbits, uint32_t strand)
{
    roll.clear();
    for (int j = 0; j < K; ++j) roll.push(asm_base<W>(key, K, j), topbits);
    if (strand) asm_flip(roll);
}

// the mask of a key as the node of the other strand sees it: its successors are the complements of the predecessors, backwards
__device__ __forceinline__ uint32_t asm_rev4(uint32_t x) { return ((x & 1u) << 3) | ((x & 2u) << 1) | ((x & 4u) >> 1) | ((x & 8u) >> 3); }
__device__ __forceinline__ uint32_t asm_orient(uint32_t info, uint32_t strand)
{
    const uint32_t m = info & 0xFFu;
    return strand ? (asm_rev4(m >> 4) | (asm_rev4(m & 15u) << 4)) : m;
}

// the window that claimed (part, key), or ASM_EMPTY32
template <int W>
__device__ uint32_t asm_find(const AsmDev &d, const uint64_t *key, uint32_t part)
{
    const uint64_t h = asm_hash<W>(key, part);
    const uint32_t tag = (uint32_t)(h >> 32);
    uint64_t s = h & d.capmask;
    for (;;) {
        const unsigned long long e = d.table[s];
        if (e == ASM_EMPTY64) return ASM_EMPTY32;
        if ((uint32_t)(e >> 32) == tag) {
            const uint32_t b = (uint32_t)e;
            const uint64_t *kb = d.keys + (uint64_t)b * W;
            bool same = d.wpart[b] == part;
#pragma unroll
            for (int w = 0; w < W; ++w) same &= key[w] == kb[w];
            if (same) return b;
        }
        s = (s + 1) & d.capmask;
    }
}

// the solid key of the rolled window: its window id and strand, or ASM_EMPTY32
template <int W>
__device__ __forceinline__ uint32_t asm_find_solid(const AsmDev &d, const LocRoll<W> &roll, uint32_t part, uint32_t &strand)
{
    uint64_t key[W];
    strand = asm_canonical<W>(roll, key);
    const uint32_t id = asm_find<W>(d, key, part);
    return (id != ASM_EMPTY32 && d.cnt[id] >= d.min_count) ? id : ASM_EMPTY32;
}

// ... that no earlier round of the cleaning removed (CLEAN = 1; without cleaning every solid key is live).  k_asm_degree alone asks
// this: heads and walks follow its masks, which say where a live node is, so they never read liveness and the count is all they check
template <int W, int CLEAN>
__device__ __forceinline__ bool asm_is_live(const AsmDev &d, const LocRoll<W> &roll, uint32_t part)
{
    uint32_t strand;
    const uint32_t id = asm_find_solid<W>(d, roll, part, strand);
    return id != ASM_EMPTY32 && !(CLEAN && d.dead[id]);
}

// the key of the rolled window where a degree mask of this round says it is live: no look at the count or at liveness
template <int W>
__device__ __forceinline__ uint32_t asm_find_node(const AsmDev &d, const LocRoll<W> &roll, uint32_t part, uint32_t &strand)
{
    uint64_t key[W];
    strand = asm_canonical<W>(roll, key);
    return asm_find<W>(d, key, part);
}

// ---- keys and counts --------------------------------------------------------------------------------------------------------
// run t of the launch: read r with cpre[r] <= t < cpre[r + 1], windows (t - cpre[r]) * ASM_RUN .. of it
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_keys(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    uint64_t n_valid = 0;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < d.n_runs; t += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = d.n_reads;            // last r with cpre[r] <= t
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (d.cpre[mid] <= t) lo = mid; else hi = mid;
        }
        const uint64_t first = (t - d.cpre[lo]) * ASM_RUN, in_read = d.wpre[lo + 1] - d.wpre[lo];
        const uint32_t count = (uint32_t)min((uint64_t)ASM_RUN, in_read - first);
        const uint8_t *s = d.bases + d.roff[lo] + first;
        const uint32_t part = d.rpart[lo];
        const uint64_t a0 = d.wpre[lo] + first;
        LocRoll<W> roll;
        roll.clear();
        int good = 0;
        for (uint32_t j = 0; j < (uint32_t)K - 1u + count; ++j) {
            uint32_t v;
            const uint32_t c = loc_code(s[j], v);
            roll.push(c, topbits);
            good = v ? good + 1 : 0;
            if (j + 1u < (uint32_t)K) continue;
            const uint64_t a = a0 + (j + 1u - (uint32_t)K);
            uint64_t key[W];
            roll.canonical(key);
#pragma unroll
            for (int w = 0; w < W; ++w) d.keys[a * W + w] = key[w];
            d.grp[a] = good >= K ? (uint32_t)a : ASM_EMPTY32;
            d.wpart[a] = part;
            n_valid += good >= K;
        }
    }
    n_valid = wave_sum_u64(n_valid);
    if ((threadIdx.x & 63u) == 0 && n_valid) atomicAdd(&d.ctr[0], (unsigned long long)n_valid);
}

// k_loc_group of kv_localize.hip with the partition in the pair and a count at the owner
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_group(AsmDev d)
{
    for (uint64_t a = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; a < d.n_windows; a += (uint64_t)gridDim.x * blockDim.x) {
        if (d.grp[a] == ASM_EMPTY32) continue;
        const uint64_t *ka = d.keys + a * W;
        const uint32_t part = d.wpart[a];
        const uint64_t h = asm_hash<W>(ka, part);
        const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | (uint32_t)a;
        uint64_t s = h & d.capmask;
        uint32_t owner;
        for (;;) {
            const unsigned long long prev = atomicCAS(&d.table[s], ASM_EMPTY64, mine);
            if (prev == ASM_EMPTY64) { owner = (uint32_t)a; break; }
            if ((prev >> 32) == (h >> 32)) {
                const uint32_t b = (uint32_t)prev;
                const uint64_t *kb = d.keys + (uint64_t)b * W;
                bool same = d.wpart[b] == part;
#pragma unroll
                for (int w = 0; w < W; ++w) same &= ka[w] == kb[w];
                if (same) { owner = b; break; }
            }
            s = (s + 1) & d.capmask;
        }
        d.grp[a] = owner;
        atomicAdd(&d.cnt[owner], 1u);
    }
}

// ---- degrees ----------------------------------------------------------------------------------------------------------------
// CLEAN = 0 is the kernel of a call that does not clean: no liveness test, the registers it had before there was cleaning
template <int W, int CLEAN>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_degree(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    uint64_t n_distinct = 0, n_solid = 0;
    for (uint64_t a = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; a < d.n_windows; a += (uint64_t)gridDim.x * blockDim.x) {
        if (d.grp[a] != (uint32_t)a) continue;
        ++n_distinct;
        if (d.cnt[a] < d.min_count) continue;
        ++n_solid;
        if (CLEAN && d.dead[a]) { d.info[a] = 0; continue; }           // removed in an earlier round: no node
        const uint32_t part = d.wpart[a];
        LocRoll<W> node;
        asm_load<W>(node, d.keys + a * W, K, topbits, 0);
        uint32_t mask = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            LocRoll<W> t = node;
            t.push(b, topbits);
            if (asm_is_live<W, CLEAN>(d, t, part)) mask |= 1u << b;
            t = node;
            asm_push_front<W>(t, b, topbits);
            if (asm_is_live<W, CLEAN>(d, t, part)) mask |= 16u << b;
        }
        d.info[a] = ASM_SOLID | mask;
    }
    n_distinct = wave_sum_u64(n_distinct);
    n_solid = wave_sum_u64(n_solid);
    if ((threadIdx.x & 63u) == 0 && (!CLEAN || d.count_pass)) {
        if (n_distinct) atomicAdd(&d.ctr[1], (unsigned long long)n_distinct);
        if (n_solid) atomicAdd(&d.ctr[2], (unsigned long long)n_solid);
    }
}

// ---- heads ------------------------------------------------------------------------------------------------------------------
// does the oriented node `node` (mask m in its own orientation) start a unitig?
template <int W>
__device__ __forceinline__ bool asm_is_head(const AsmDev &d, const LocRoll<W> &node, uint32_t m, uint32_t part, int topbits)
{
    const uint32_t pm = m >> 4;
    if (__popc(pm) != 1) return true;
    LocRoll<W> v = node;
    asm_push_front<W>(v, (uint32_t)__ffs(pm) - 1u, topbits);
    uint32_t strand;
    const uint32_t id = asm_find_solid<W>(d, v, part, strand);
    if (id == ASM_EMPTY32) return true;                 // (the mask says it is there)
    return __popc(asm_orient(d.info[id], strand) & 15u) != 1;
}

// a workgroup takes chunks of ASM_THREADS consecutive windows, a lane one window of the chunk
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_heads(AsmDev d)
{
    __shared__ uint32_t wsum[ASM_THREADS / 64];
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    const uint64_t n_chunks = (d.n_windows + ASM_THREADS - 1) / ASM_THREADS;
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t a = chunk * ASM_THREADS + threadIdx.x;
        const uint32_t info = a < d.n_windows ? d.info[a] : 0u;
        uint32_t flags = 0;
        if (info & ASM_SOLID) {
            const uint32_t part = d.wpart[a];
            LocRoll<W> node;
            asm_load<W>(node, d.keys + a * W, K, topbits, 0);
            if (asm_is_head<W>(d, node, asm_orient(info, 0), part, topbits)) flags |= ASM_HEAD0;
            asm_flip(node);
            if (asm_is_head<W>(d, node, asm_orient(info, 1), part, topbits)) flags |= ASM_HEAD1;
            if (flags) d.info[a] = info | flags;        // (the other lanes read bits 0-8 only, and those stay)
        }
        const uint32_t incl = wave_incl_scan((uint32_t)__popc(flags));
        if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        if (threadIdx.x == 0) d.ccount[chunk] = waves_before(wsum, (uint32_t)(ASM_THREADS / 64));
        __syncthreads();
    }
}

__global__ __launch_bounds__(ASM_THREADS) void k_asm_compact(AsmDev d)
{
    __shared__ uint32_t wsum[ASM_THREADS / 64];
    const uint64_t n_chunks = (d.n_windows + ASM_THREADS - 1) / ASM_THREADS;
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t a = chunk * ASM_THREADS + threadIdx.x;
        const uint32_t info = a < d.n_windows ? d.info[a] : 0u;
        const uint32_t mine = (uint32_t)__popc(info & (ASM_HEAD0 | ASM_HEAD1));
        const uint32_t incl = wave_incl_scan(mine);
        if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint64_t at = d.hbase[chunk] + waves_before(wsum, threadIdx.x >> 6) + incl - mine;
        if (d.hinv) {
            if (info & ASM_HEAD0) d.hinv[2 * a] = (uint32_t)at;
            if (info & ASM_HEAD1) d.hinv[2 * a + 1] = (uint32_t)(at + ((info & ASM_HEAD0) ? 1u : 0u));
        }
        if (info & ASM_HEAD0) d.heads[at++] = 2u * (uint32_t)a;
        if (info & ASM_HEAD1) d.heads[at] = 2u * (uint32_t)a + 1u;
        __syncthreads();
    }
}

// ---- walk -------------------------------------------------------------------------------------------------------------------
// WRITE = 0: the length of every head's unitig, and whether it is the strand that is reported.  WRITE = 1: the bases of those.
template <int W, int WRITE>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_walk(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    uint64_t n_kept = 0, n_on = 0;                      // unitigs this lane keeps, solid keys on them
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < d.n_heads; h += (uint64_t)gridDim.x * blockDim.x) {
        if (WRITE && !d.kflag[h]) continue;
        const uint32_t a = d.heads[h] >> 1, strand0 = d.heads[h] & 1u;
        const uint32_t part = d.wpart[a];
        LocRoll<W> node;
        asm_load<W>(node, d.keys + (uint64_t)a * W, K, topbits, strand0);
        uint64_t first[W];
#pragma unroll
        for (int w = 0; w < W; ++w) first[w] = node.f[w];
        uint32_t m = asm_orient(d.info[a], strand0);
        uint8_t *out = nullptr;
        if (WRITE) {
            const uint64_t u = d.uidx[h];
            out = d.out + d.ubase[h];
            d.uoff[u] = d.out_base + d.ubase[h];
            d.upart[u] = d.part0 + part;
            for (int j = 0; j < K; ++j) out[j] = (uint8_t)((0x54474341u >> (8u * asm_base<W>(first, K, j))) & 0xFFu);     // "ACGT"
        }
        const uint32_t guard = d.guard[part];
        uint32_t steps = 0;
        while (steps < guard) {
            const uint32_t sm = m & 15u;
            if (__popc(sm) != 1) break;
            const uint32_t b = (uint32_t)__ffs(sm) - 1u;
            LocRoll<W> next = node;
            next.push(b, topbits);
            uint32_t strand;
            const uint32_t id = asm_find_solid<W>(d, next, part, strand);
            if (id == ASM_EMPTY32) break;               // (the mask says it is there)
            const uint32_t m2 = asm_orient(d.info[id], strand);
            if (__popc(m2 >> 4) != 1) break;
            node = next;
            m = m2;
            ++steps;
            if (WRITE) out[(uint32_t)K - 1u + steps] = (uint8_t)((0x54474341u >> (8u * b)) & 0xFFu);
        }
        if (!WRITE) {
            // the reverse complement of this unitig starts with the reverse complement of the last node
            bool less = false, decided = false;
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (!decided && first[w] != node.r[w]) { less = first[w] < node.r[w]; decided = true; }
            const bool keep = less || !decided;         // !decided: the unitig is its own reverse complement, this head is both
            d.kflag[h] = keep ? 1u : 0u;
            d.klen[h] = keep ? (uint32_t)K + steps : 0u;
            if (keep) {
                ++n_kept;
                n_on += decided ? steps + 1u : (steps + 1u) / 2u;      // its own reverse complement: every key is on it twice
                atomicAdd(&d.pcount[part], 1u);
            }
        }
    }
    if (!WRITE) {                                       // one atomic per wave and counter
        n_kept = wave_sum_u64(n_kept);
        n_on = wave_sum_u64(n_on);
        if ((threadIdx.x & 63u) == 0 && n_kept) {
            atomicAdd(&d.ctr[3], (unsigned long long)n_kept);
            atomicAdd(&d.ctr[4], (unsigned long long)n_on);
        }
    }
}

// ---- cleaning: measure, decide, apply -------------------------------------------------------------------------------------------
// a lane per head: the record of its unitig on this round's graph
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_measure(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < d.n_heads; h += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = d.heads[h] >> 1, strand0 = d.heads[h] & 1u;
        const uint32_t part = d.wpart[a];
        LocRoll<W> node;
        asm_load<W>(node, d.keys + (uint64_t)a * W, K, topbits, strand0);
        uint32_t m = asm_orient(d.info[a], strand0), strand;
        const uint32_t pm = m >> 4;
        uint32_t pcode = ASM_EMPTY32, qcode = ASM_EMPTY32, last = d.heads[h];
        if (__popc(pm) == 1) {
            LocRoll<W> v = node;
            asm_push_front<W>(v, (uint32_t)__ffs(pm) - 1u, topbits);
            const uint32_t id = asm_find_node<W>(d, v, part, strand);
            if (id != ASM_EMPTY32) pcode = 2u * id + strand;
        }
        uint64_t sum = d.cnt[a];
        const uint32_t guard = d.guard[part];
        uint32_t steps = 0;
        while (steps < guard) {
            const uint32_t sm = m & 15u;
            if (__popc(sm) != 1) break;
            LocRoll<W> next = node;
            next.push((uint32_t)__ffs(sm) - 1u, topbits);
            const uint32_t id = asm_find_node<W>(d, next, part, strand);
            if (id == ASM_EMPTY32) break;               // (the mask says it is there)
            qcode = 2u * id + strand;                   // the one node of Q, if the walk ends here
            const uint32_t m2 = asm_orient(d.info[id], strand);
            if (__popc(m2 >> 4) != 1) break;
            node = next;
            m = m2;
            ++steps;
            sum += d.cnt[id];
            last = qcode;
            qcode = ASM_EMPTY32;
        }
        d.rm[h] = steps + 1u;
        d.rsum[h] = sum;
        d.rpq[h] = pm | ((m & 15u) << 4);
        d.rlast[h] = last;
        d.rpcode[h] = pcode;
        d.rqcode[h] = qcode;
    }
}

// is the canonical key that window x owns smaller than the one y owns?
template <int W>
__device__ __forceinline__ bool asm_key_less(const AsmDev &d, uint32_t x, uint32_t y)
{
    const uint64_t *kx = d.keys + (uint64_t)x * W, *ky = d.keys + (uint64_t)y * W;
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (kx[w] != ky[w]) return kx[w] < ky[w];
    return false;
}

// id(U): the window that owns the smaller canonical key of the first and the last node
template <int W>
__device__ __forceinline__ uint32_t asm_unit_id(const AsmDev &d, uint64_t h)
{
    const uint32_t first = d.heads[h] >> 1, last = d.rlast[h] >> 1;
    return asm_key_less<W>(d, last, first) ? last : first;
}

// a lane per head: rules 3a and 3b from the records of this round, which nothing changes while this runs
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_decide(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    uint64_t n_tips = 0, n_tip_keys = 0, n_arms = 0, n_arm_keys = 0;
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < d.n_heads; h += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t code = d.heads[h], a = code >> 1, m = d.rm[h], pq = d.rpq[h], pcode = d.rpcode[h];
        const uint32_t qn = (uint32_t)__popc(pq >> 4);
        const bool tip = qn == 0 && m <= d.tip_nodes, arm = qn == 1 && m <= d.bubble_nodes && d.rqcode[h] != ASM_EMPTY32;
        uint32_t flag = 0;
        if (__popc(pq & 15u) == 1 && pcode != ASM_EMPTY32 && (tip || arm)) {
            const uint32_t part = d.wpart[a], other = d.rlast[h] ^ 1u;      // the head of the reverse complement of this unitig
            const uint32_t jid = pcode >> 1, jstrand = pcode & 1u;
            const uint32_t sm = asm_orient(d.info[jid], jstrand) & 15u;
            LocRoll<W> j;
            asm_load<W>(j, d.keys + (uint64_t)jid * W, K, topbits, jstrand);
            const uint64_t S = d.rsum[h];
            for (uint32_t b = 0; b < 4; ++b) {
                if (!((sm >> b) & 1u)) continue;
                LocRoll<W> s = j;
                s.push(b, topbits);
                uint32_t strand;
                const uint32_t sid = asm_find_node<W>(d, s, part, strand);
                if (sid == ASM_EMPTY32) continue;       // (the mask says it is there)
                const uint32_t scode = 2u * sid + strand;
                if (scode == code) continue;
                if (tip) {
                    const uint32_t cs = d.cnt[sid], c1 = d.cnt[a];
                    if (cs > c1 || (cs == c1 && asm_key_less<W>(d, sid, a))) flag = ASM_FLAG_TIP;
                    continue;
                }
                if (scode == other) continue;           // its own reverse complement, from a to rc(a), is no rival
                const uint64_t hv = d.hinv[scode];      // a successor of a node with two is a head
                if (hv >= d.n_heads || d.heads[hv] != scode) continue;
                const uint32_t mv = d.rm[hv], pqv = d.rpq[hv];
                if (mv > d.bubble_nodes || __popc(pqv & 15u) != 1 || __popc(pqv >> 4) != 1 || d.rqcode[hv] != d.rqcode[h]) continue;
                const uint64_t lhs = d.rsum[hv] * (uint64_t)m, rhs = S * (uint64_t)mv;
                bool beaten;
                if (lhs != rhs) beaten = lhs > rhs;
                else if (mv != m) beaten = mv > m;
                else beaten = asm_key_less<W>(d, asm_unit_id<W>(d, hv), asm_unit_id<W>(d, h));
                if (beaten) flag = ASM_FLAG_ARM;
            }
        }
        // a tip is one in one orientation only; an arm in both, and the head with the smaller code counts it (one head: both)
        if (flag == ASM_FLAG_TIP) { flag |= ASM_FLAG_MARKS; ++n_tips; n_tip_keys += m; }
        if (flag == ASM_FLAG_ARM && code <= (d.rlast[h] ^ 1u)) {
            flag |= ASM_FLAG_MARKS;
            ++n_arms;
            n_arm_keys += code == (d.rlast[h] ^ 1u) ? m / 2u : m;       // its own reverse complement: every key is on it twice
        }
        d.rflag[h] = flag;
    }
    n_tips = wave_sum_u64(n_tips);
    n_tip_keys = wave_sum_u64(n_tip_keys);
    n_arms = wave_sum_u64(n_arms);
    n_arm_keys = wave_sum_u64(n_arm_keys);
    if ((threadIdx.x & 63u) == 0 && (n_tips | n_arms)) {
        atomicAdd(&d.ctr[5], (unsigned long long)n_tips);
        atomicAdd(&d.ctr[6], (unsigned long long)n_tip_keys);
        atomicAdd(&d.ctr[7], (unsigned long long)n_arms);
        atomicAdd(&d.ctr[8], (unsigned long long)n_arm_keys);
        atomicAdd(&d.ctr[9], (unsigned long long)(n_tip_keys + n_arm_keys));
    }
}

// a lane per flagged unitig: its keys are dead from the next round on.  Reads masks and records only, never liveness.
template <int W>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_kill(AsmDev d)
{
    const int K = d.K, topbits = 2 * K - 64 * (W - 1);
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < d.n_heads; h += (uint64_t)gridDim.x * blockDim.x) {
        if (!(d.rflag[h] & ASM_FLAG_MARKS)) continue;
        const uint32_t a = d.heads[h] >> 1, strand0 = d.heads[h] & 1u;
        const uint32_t part = d.wpart[a], nodes = d.rm[h];
        LocRoll<W> node;
        asm_load<W>(node, d.keys + (uint64_t)a * W, K, topbits, strand0);
        uint32_t m = asm_orient(d.info[a], strand0);
        d.dead[a] = 1u;
        for (uint32_t i = 1; i < nodes; ++i) {
            const uint32_t sm = m & 15u;
            if (__popc(sm) != 1) break;                 // (the record says there are `nodes`)
            node.push((uint32_t)__ffs(sm) - 1u, topbits);
            uint32_t strand;
            const uint32_t id = asm_find_node<W>(d, node, part, strand);
            if (id == ASM_EMPTY32) break;
            d.dead[id] = 1u;
            m = asm_orient(d.info[id], strand);
        }
    }
}

}  // namespace

// a stream's working memory, kept between calls (grow-only; kv_scratch_trim gives it back): gigabytes at 20 000 partitions a call,
// and allocating and freeing them costs more than the kernels
struct AsmScratch {
    KvArena main, table, heads, out;
};
static KvPerStream<AsmScratch> g_asm_scratch;
void kv_asm_scratch_release()
{
    g_asm_scratch.for_each([](AsmScratch &a) { a.main.release(); a.table.release(); a.heads.release(); a.out.release(); });
}

struct kv_assembly {
    std::vector<char> bases;
    std::vector<uint64_t> off;              // n_unitigs + 1
    std::vector<uint32_t> part, count;      // per unitig; per partition
    uint64_t stats[KV_ASSEMBLE_NSTATS] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t clean[KV_ASSEMBLE_NCLEAN] = {0, 0, 0, 0, 0};
};

namespace {

// degrees and heads of the live keys, the chunks' head counts summed: how many heads there are
template <int W>
int asm_count_heads(const AsmDev &d, uint64_t nw, uint64_t n_chunks, uint64_t *d_hbase, hipStream_t st, uint64_t *n_heads)
{
    const dim3 block(ASM_THREADS);
    {
        KvProfScope prof("k_asm_degree");
        if (d.dead) hipLaunchKernelGGL((k_asm_degree<W, 1>), dim3(asm_grid(nw)), block, 0, st, d);
        else hipLaunchKernelGGL((k_asm_degree<W, 0>), dim3(asm_grid(nw)), block, 0, st, d);
    }
    { KvProfScope prof("k_asm_heads"); hipLaunchKernelGGL(k_asm_heads<W>, dim3(asm_grid(nw)), block, 0, st, d); }
    KV_HIP(hipGetLastError());
    { KvProfScope prof("k_asm_scan"); kv_excl_scan_launch(d.ccount, (uint32_t)n_chunks, d_hbase, st); }
    KV_HIP(hipGetLastError());
    hipError_t re = hipSuccess;
    KvReadback rb;
    const uint64_t *got = rb.add((const uint64_t *)d_hbase + n_chunks, 1, st, &re);
    KV_HIP(re);
    KV_HIP(rb.wait(st));
    *n_heads = *got;
    KV_REQUIRE(*n_heads < 0xFFFFFFF0ull, KV_ERR_CAPACITY, "too many unitig heads in one launch (%llu)", (unsigned long long)*n_heads);
    return KV_OK;
}

// rules 3a to 3c: rounds of measure, decide and -- in a launch of its own -- apply, until one removes nothing.  *final_heads is
// set, to the number of heads, when the last round removed nothing: its degrees, heads and chunk sums are those of the final graph
template <int W>
int asm_clean_rounds(AsmDev &d, AsmScratch &scratch, uint64_t nw, uint64_t n_chunks, uint64_t *d_hbase, uint32_t clean_rounds, hipStream_t st,
                     uint64_t *removing_rounds, uint64_t *final_heads)
{
    const dim3 block(ASM_THREADS);
    uint64_t removed = 0;
    for (uint32_t round = 0; round < clean_rounds; ++round) {
        uint64_t n_heads = 0;
        KV_STEP(asm_count_heads<W>(d, nw, n_chunks, d_hbase, st, &n_heads));
        d.count_pass = 0;
        if (!n_heads) { *final_heads = 0; break; }      // (cycles alone: nothing to remove)
        const size_t hs[8] = {n_heads * 4, n_heads * 4, n_heads * 4, n_heads * 4, n_heads * 4, n_heads * 4, n_heads * 4, n_heads * 8};
        KvCarve<8> hc(hs);
        const hipError_t e = hc.from(scratch.heads);
        KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "assembly head record allocation failed: %s", hipGetErrorString(e));
        d.n_heads = n_heads;
        d.heads = hc.at<uint32_t>(0); d.rm = hc.at<uint32_t>(1); d.rpq = hc.at<uint32_t>(2); d.rlast = hc.at<uint32_t>(3);
        d.rpcode = hc.at<uint32_t>(4); d.rqcode = hc.at<uint32_t>(5); d.rflag = hc.at<uint32_t>(6); d.rsum = hc.at<uint64_t>(7);
        hipLaunchKernelGGL(k_asm_compact, dim3(asm_grid(nw)), block, 0, st, d);
        { KvProfScope prof("k_asm_measure"); hipLaunchKernelGGL(k_asm_measure<W>, dim3(asm_grid(n_heads)), block, 0, st, d); }
        { KvProfScope prof("k_asm_decide"); hipLaunchKernelGGL(k_asm_decide<W>, dim3(asm_grid(n_heads)), block, 0, st, d); }
        KV_HIP(hipGetLastError());
        hipError_t re = hipSuccess;
        KvReadback rb;
        const uint64_t *got = rb.add((const uint64_t *)d.ctr + 9, 1, st, &re);     // keys removed so far: 8 bytes a round
        KV_HIP(re);
        KV_HIP(rb.wait(st));
        if (*got == removed) { *final_heads = n_heads; break; }
        removed = *got;
        ++*removing_rounds;
        { KvProfScope prof("k_asm_kill"); hipLaunchKernelGGL(k_asm_kill<W>, dim3(asm_grid(n_heads)), block, 0, st, d); }
        KV_HIP(hipGetLastError());
    }
    return KV_OK;
}

template <int W>
int asm_launch(const AsmLaunch &L, AsmDev d, hipStream_t st, const char *bases, const uint64_t *read_off, const uint64_t *part_first,
               uint32_t clean_rounds, kv_assembly *res)
{
    const bool cleaning = asm_cleaning(d.tip_nodes, d.bubble_nodes);
    const uint64_t nr = L.read1 - L.read0, np = L.part1 - L.part0, nw = L.n_windows, n_chunks = asm_chunks(nw);
    // the host's view of the launch: everything counted from its first read and first partition
    std::vector<uint64_t> roff(nr + 1), wpre(nr + 1), cpre(nr + 1);
    std::vector<uint32_t> rpart(nr + 1, 0), guard(np + 1, 0);
    const uint64_t base0 = read_off[L.read0];
    wpre[0] = cpre[0] = 0;
    for (uint64_t p = 0; p < np; ++p) {
        const uint64_t r0 = part_first[L.part0 + p] - L.read0, r1 = part_first[L.part0 + p + 1] - L.read0;
        for (uint64_t r = r0; r < r1; ++r) {
            const uint64_t len = read_off[L.read0 + r + 1] - read_off[L.read0 + r];
            roff[r] = read_off[L.read0 + r] - base0;
            rpart[r] = (uint32_t)p;
            wpre[r + 1] = wpre[r] + asm_read_windows(len, d.K);
            cpre[r + 1] = cpre[r] + asm_read_runs(len, d.K);
        }
        guard[p] = (uint32_t)(2 * (wpre[r1] - wpre[r0]) + 2);
    }
    roff[nr] = L.n_bases;
    const size_t sizes[17] = {L.n_bases + 16, (nr + 1) * 8, (nr + 1) * 8, (nr + 1) * 8, (nr + 1) * 4, (np + 1) * 4, (np + 1) * 4,
                              nw * W * 8, nw * 4, nw * 4, nw * 4, nw * 4, (n_chunks + 1) * 4, (n_chunks + 1) * 8, ASM_CTR_BYTES,
                              cleaning ? nw * 4 : 0, cleaning ? nw * 8 : 0};
    KvCarve<17> c(sizes);
    AsmScratch &scratch = g_asm_scratch.get(st);
    hipError_t e = c.from(scratch.main);
    if (e == hipSuccess) e = scratch.table.need(L.table_cap * 8);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "assembly buffers allocation failed: %s", hipGetErrorString(e));
    uint8_t *d_bases = c.at<uint8_t>(0);
    uint64_t *d_roff = c.at<uint64_t>(1), *d_wpre = c.at<uint64_t>(2), *d_cpre = c.at<uint64_t>(3);
    uint32_t *d_rpart = c.at<uint32_t>(4), *d_guard = c.at<uint32_t>(5);
    d.bases = d_bases; d.roff = d_roff; d.wpre = d_wpre; d.cpre = d_cpre; d.rpart = d_rpart; d.guard = d_guard;
    d.pcount = c.at<uint32_t>(6);
    d.keys = c.at<uint64_t>(7); d.grp = c.at<uint32_t>(8); d.wpart = c.at<uint32_t>(9); d.cnt = c.at<uint32_t>(10);
    d.info = c.at<uint32_t>(11); d.ccount = c.at<uint32_t>(12);
    uint64_t *d_hbase = c.at<uint64_t>(13);
    d.hbase = d_hbase;
    d.table = (unsigned long long *)scratch.table.p; d.capmask = L.table_cap - 1; d.ctr = c.at<unsigned long long>(14);
    d.n_reads = nr; d.n_windows = nw; d.n_runs = L.n_runs; d.part0 = (uint32_t)L.part0; d.out_base = res->bases.size();
    KV_HIP(hipMemcpyAsync(d_bases, bases + base0, L.n_bases, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_roff, roff.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_wpre, wpre.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_cpre, cpre.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_rpart, rpart.data(), (nr + 1) * 4, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_guard, guard.data(), (np + 1) * 4, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemsetAsync(d.pcount, 0, (np + 1) * 4, st));
    KV_HIP(hipMemsetAsync(d.cnt, 0, c.off[12] - c.off[10], st));        // counts and masks
    KV_HIP(hipMemsetAsync(d.table, 0xFF, L.table_cap * 8, st));
    KV_HIP(hipMemsetAsync(d.ctr, 0, ASM_CTR_BYTES, st));
    d.count_pass = 1;
    d.dead = nullptr; d.hinv = nullptr;
    if (cleaning) {
        d.dead = c.at<uint32_t>(15); d.hinv = c.at<uint32_t>(16);
        KV_HIP(hipMemsetAsync(d.dead, 0, nw * 4, st));
    }
    const dim3 block(ASM_THREADS);
    { KvProfScope prof("k_asm_keys"); hipLaunchKernelGGL(k_asm_keys<W>, dim3(asm_grid(L.n_runs)), block, 0, st, d); }
    { KvProfScope prof("k_asm_group"); hipLaunchKernelGGL(k_asm_group<W>, dim3(asm_grid(nw)), block, 0, st, d); }
    uint64_t removing_rounds = 0;
    uint64_t n_heads = ASM_EMPTY64;
    if (cleaning) KV_STEP(asm_clean_rounds<W>(d, scratch, nw, n_chunks, d_hbase, clean_rounds, st, &removing_rounds, &n_heads));
    if (n_heads == ASM_EMPTY64) KV_STEP(asm_count_heads<W>(d, nw, n_chunks, d_hbase, st, &n_heads));     // (else the last round left them)
    d.hinv = nullptr;                                   // (the last compact has no one to leave the inverse map to)
    uint64_t n_unitigs = 0, n_out = 0;
    if (n_heads) {
        const size_t hs[5] = {n_heads * 4, n_heads * 4, n_heads * 4, (n_heads + 1) * 8, (n_heads + 1) * 8};
        KvCarve<5> hc(hs);
        e = hc.from(scratch.heads);
        KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "assembly head buffers allocation failed: %s", hipGetErrorString(e));
        d.n_heads = n_heads;
        d.heads = hc.at<uint32_t>(0); d.klen = hc.at<uint32_t>(1); d.kflag = hc.at<uint32_t>(2);
        uint64_t *d_ubase = hc.at<uint64_t>(3), *d_uidx = hc.at<uint64_t>(4);
        d.ubase = d_ubase; d.uidx = d_uidx;
        hipLaunchKernelGGL(k_asm_compact, dim3(asm_grid(nw)), block, 0, st, d);
        { KvProfScope prof("k_asm_walk_len"); hipLaunchKernelGGL((k_asm_walk<W, 0>), dim3(asm_grid(n_heads)), block, 0, st, d); }
        KV_HIP(hipGetLastError());
        {
            KvProfScope prof("k_asm_scan");
            kv_excl_scan_launch(d.klen, (uint32_t)n_heads, d_ubase, st);
            kv_excl_scan_launch(d.kflag, (uint32_t)n_heads, d_uidx, st);
        }
        KV_HIP(hipGetLastError());
        {
            hipError_t re = hipSuccess;
            KvReadback rb;
            const uint64_t *b = rb.add((const uint64_t *)d_ubase + n_heads, 1, st, &re);
            const uint64_t *u = rb.add((const uint64_t *)d_uidx + n_heads, 1, st, &re);
            KV_HIP(re);
            KV_HIP(rb.wait(st));
            n_out = *b; n_unitigs = *u;
        }
    }
    const size_t at_u = res->part.size(), at_b = res->bases.size();
    if (n_unitigs) {
        const size_t os[3] = {n_out, n_unitigs * 8, n_unitigs * 4};
        KvCarve<3> oc(os);
        e = oc.from(scratch.out);
        KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "assembly output buffers allocation failed: %s", hipGetErrorString(e));
        d.out = oc.at<uint8_t>(0); d.uoff = oc.at<uint64_t>(1); d.upart = oc.at<uint32_t>(2);
        { KvProfScope prof("k_asm_walk_write"); hipLaunchKernelGGL((k_asm_walk<W, 1>), dim3(asm_grid(n_heads)), block, 0, st, d); }
        KV_HIP(hipGetLastError());
        res->bases.resize(at_b + n_out);
        res->part.resize(at_u + n_unitigs);
        res->off.resize(at_u + n_unitigs + 1);
        KV_HIP(hipMemcpyAsync(res->bases.data() + at_b, d.out, n_out, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(res->off.data() + at_u, d.uoff, n_unitigs * 8, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(res->part.data() + at_u, d.upart, n_unitigs * 4, hipMemcpyDeviceToHost, st));
    }
    unsigned long long ctrs[ASM_CTR_BYTES / 8];
    KV_HIP(hipMemcpyAsync(res->count.data() + L.part0, d.pcount, np * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(ctrs, d.ctr, sizeof(ctrs), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    res->off[at_u + n_unitigs] = at_b + n_out;
    res->stats[0] += ctrs[0]; res->stats[1] += ctrs[1]; res->stats[2] += ctrs[2]; res->stats[3] += n_heads; res->stats[4] += ctrs[3];
    res->stats[5] += ctrs[2] - ctrs[9] - ctrs[4];      // solid, less the removed: live keys; less those on a unitig
    res->stats[6] += 1;
    for (int i = 0; i < 4; ++i) res->clean[i] += ctrs[5 + i];
    res->clean[4] += removing_rounds;
    return KV_OK;
}

}  // namespace

extern "C" int kv_assemble_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                                uint64_t mem_budget, uint64_t *launch_ends, uint64_t *n_launches)
{
    KV_REQUIRE(launch_ends && n_launches, KV_ERR_ARG, "kv_assemble_plan: null argument");
    KV_STEP(asm_check_args(read_off, n_reads, part_first, n_parts, ksize, 1));
    std::vector<AsmLaunch> launches;
    KV_STEP(asm_plan(read_off, n_reads, part_first, n_parts, ksize, mem_budget ? mem_budget : ASM_DEFAULT_BUDGET, launches));
    for (size_t l = 0; l < launches.size(); ++l) launch_ends[l] = launches[l].part1;
    *n_launches = launches.size();
    return KV_OK;
}

extern "C" int kv_assemble_clean_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                                      uint64_t mem_budget, uint32_t tip_nodes, uint32_t bubble_nodes, uint32_t clean_rounds,
                                      uint64_t *launch_ends, uint64_t *n_launches)
{
    KV_REQUIRE(launch_ends && n_launches, KV_ERR_ARG, "kv_assemble_clean_plan: null argument");
    KV_STEP(asm_check_args(read_off, n_reads, part_first, n_parts, ksize, 1));
    KV_STEP(asm_check_clean(tip_nodes, bubble_nodes, clean_rounds));
    std::vector<AsmLaunch> launches;
    KV_STEP(asm_plan(read_off, n_reads, part_first, n_parts, ksize, mem_budget ? mem_budget : ASM_DEFAULT_BUDGET, launches,
                     asm_cleaning(tip_nodes, bubble_nodes)));
    for (size_t l = 0; l < launches.size(); ++l) launch_ends[l] = launches[l].part1;
    *n_launches = launches.size();
    return KV_OK;
}

extern "C" int kv_assemble_batch(const char *bases, const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts,
                                 int ksize, uint32_t min_count, uint64_t mem_budget, uint64_t *n_unitigs, uint64_t *n_bases, kv_assembly **out)
{
    return kv_assemble_clean_batch(bases, read_off, n_reads, part_first, n_parts, ksize, min_count, mem_budget, 0, 0, ASM_DEFAULT_CLEAN_ROUNDS,
                                   n_unitigs, n_bases, out);
}

extern "C" int kv_assemble_clean_batch(const char *bases, const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts,
                                       int ksize, uint32_t min_count, uint64_t mem_budget, uint32_t tip_nodes, uint32_t bubble_nodes,
                                       uint32_t clean_rounds, uint64_t *n_unitigs, uint64_t *n_bases, kv_assembly **out)
{
    KV_REQUIRE(out && n_unitigs && n_bases, KV_ERR_ARG, "kv_assemble_batch: null argument");
    KV_STEP(asm_check_args(read_off, n_reads, part_first, n_parts, ksize, min_count));
    KV_STEP(asm_check_clean(tip_nodes, bubble_nodes, clean_rounds));
    KV_REQUIRE(bases || read_off[n_reads] == 0, KV_ERR_ARG, "kv_assemble_batch: null argument");
    std::vector<AsmLaunch> launches;
    KV_STEP(asm_plan(read_off, n_reads, part_first, n_parts, ksize, mem_budget ? mem_budget : ASM_DEFAULT_BUDGET, launches,
                     asm_cleaning(tip_nodes, bubble_nodes)));
    hipStream_t st = kv_stream();
    kv_assembly *res = new kv_assembly;
    struct Guard { kv_assembly *h; ~Guard() { delete h; } } guard{res};
    res->count.assign(n_parts, 0);
    res->off.assign(1, 0);
    AsmDev d = AsmDev();
    d.K = ksize;
    d.min_count = min_count;
    d.tip_nodes = tip_nodes;
    d.bubble_nodes = bubble_nodes;
    for (const AsmLaunch &L : launches) {
        if (L.n_windows == 0) continue;                 // (nothing to assemble: the counts stay 0)
        if (ksize <= 31) KV_STEP(asm_launch<1>(L, d, st, bases, read_off, part_first, clean_rounds, res));
        else KV_STEP(asm_launch<2>(L, d, st, bases, read_off, part_first, clean_rounds, res));
    }
    *n_unitigs = res->part.size();
    *n_bases = res->bases.size();
    guard.h = nullptr;
    *out = res;
    return KV_OK;
}

extern "C" int kv_assemble_fetch(kv_assembly *h, char *bases_out, uint64_t *offsets_out, uint32_t *part_out, uint32_t *count_out)
{
    KV_REQUIRE(h && offsets_out && (bases_out || h->bases.empty()) && (part_out || h->part.empty()) && (count_out || h->count.empty()),
               KV_ERR_ARG, "kv_assemble_fetch: null argument");
    std::copy(h->bases.begin(), h->bases.end(), bases_out);
    std::copy(h->off.begin(), h->off.end(), offsets_out);
    std::copy(h->part.begin(), h->part.end(), part_out);
    std::copy(h->count.begin(), h->count.end(), count_out);
    return KV_OK;
}

extern "C" int kv_assemble_stats(kv_assembly *h, uint64_t *stats_out)
{
    KV_REQUIRE(h && stats_out, KV_ERR_ARG, "kv_assemble_stats: null argument");
    std::copy(h->stats, h->stats + KV_ASSEMBLE_NSTATS, stats_out);
    return KV_OK;
}

extern "C" int kv_assemble_clean_stats(kv_assembly *h, uint64_t *clean_out)
{
    KV_REQUIRE(h && clean_out, KV_ERR_ARG, "kv_assemble_clean_stats: null argument");
    std::copy(h->clean, h->clean + KV_ASSEMBLE_NCLEAN, clean_out);
    return KV_OK;
}

extern "C" int kv_assemble_destroy(kv_assembly *h)
{
    delete h;
    return KV_OK;
}
