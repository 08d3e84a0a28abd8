// kv_localize.hip -- exact seed matching for `kevlar localize` (kevlar/localize.py:113-144, kevlar/reference.py:83-103):
// every window of length Z of every contig is a seed; the reference hands them to `bwa mem -k Z -T Z -a`, which reports the
// perfect full-length matches only.  That is a join between the canonical seed set and every window of the genome:
//   (1) create: canonical 2-bit key of every contig window, equal keys grouped in an open-addressing table whose slots hold
//       (hash tag, id of the first window that claimed the key), keys kept in an array of their own, one prefilter bit per seed;
//   (2) scan: genome text streamed chunk by chunk; a lane rolls the forward and reverse-complement key over a run of
//       consecutive windows, tests one prefilter bit per window, and only a window whose bit is set probes the table; a slot
//       with the window's tag is confirmed by a full key compare before (seed id, global position) is appended.
// Validity is per position: a window matches only if all Z bytes are A/C/G/T (either case); anything else -- N, IUPAC codes,
// the separator the caller puts between sequences -- resets the run of valid bases.
#include <algorithm>

#include "kv_device.h"
#include "kv_genome_plan.h"
#include "kv_roll2bit_device.h"

namespace {

#define LOC_EMPTY32 0xFFFFFFFFu
#define LOC_EMPTY64 0xFFFFFFFFFFFFFFFFull
#define LOC_THREADS 256
#define LOC_RUN 64                                  // consecutive windows a lane rolls over
#define LOC_TILE (LOC_THREADS * LOC_RUN)            // window starts per workgroup
#define LOC_OVERLAP_WORDS 8                         // 16-base words behind the tile: Z - 1 <= 127 bases of overlap
#define LOC_WORDS (LOC_TILE / 16 + LOC_OVERLAP_WORDS)
#define LOC_MAX_Z 128

// low bits: table slot; high 32 bits: slot tag and prefilter bit
template <int W>
__device__ __forceinline__ uint64_t loc_hash(const uint64_t *key)
{
    uint64_t h = 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (int w = 0; w < W; ++w) h = fmix64(h ^ key[w]) + 0x632be59bd9b4e019ull * (uint64_t)(w + 1);
    return h;
}

// ---- create -----------------------------------------------------------------------------------------------------------------
// window a of the concatenated contigs: contig c with wpre[c] <= a < wpre[c + 1], starting at base off[c] + (a - wpre[c])
template <int W>
__global__ void k_loc_keys(const uint8_t *bases, const uint64_t *off, const uint64_t *wpre, uint64_t n_contigs, uint64_t n_windows,
                           int Z, uint64_t *keys, uint32_t *grp)
{
    const int topbits = 2 * Z - 64 * (W - 1);
    for (uint64_t a = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; a < n_windows; a += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n_contigs;            // last c with wpre[c] <= a
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (wpre[mid] <= a) lo = mid; else hi = mid;
        }
        const uint8_t *s = bases + off[lo] + (a - wpre[lo]);
        LocRoll<W> roll;
        roll.clear();
        uint32_t all_valid = 1;
        for (int j = 0; j < Z; ++j) {
            uint32_t v;
            const uint32_t c = loc_code(s[j], v);
            all_valid &= v;
            roll.push(c, topbits);
        }
        uint64_t key[W];
        roll.canonical(key);
#pragma unroll
        for (int w = 0; w < W; ++w) keys[a * W + w] = key[w];
        grp[a] = all_valid ? (uint32_t)a : LOC_EMPTY32;
    }
}

// k_group of kv_graph.hip with a tag beside the owner
template <int W>
__global__ void k_loc_group(const uint64_t *keys, uint64_t n_windows, unsigned long long *table, uint64_t capmask, uint32_t *grp,
                            unsigned long long *n_distinct)
{
    for (uint64_t a = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; a < n_windows; a += (uint64_t)gridDim.x * blockDim.x) {
        if (grp[a] == LOC_EMPTY32) continue;
        const uint64_t *ka = keys + a * W;
        const uint64_t h = loc_hash<W>(ka);
        const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | (uint32_t)a;
        uint64_t s = h & capmask;
        for (;;) {
            const unsigned long long prev = atomicCAS(&table[s], LOC_EMPTY64, mine);
            if (prev == LOC_EMPTY64) { atomicAdd(n_distinct, 1ull); break; }
            if ((prev >> 32) == (h >> 32)) {
                const uint64_t *kb = keys + (uint64_t)(uint32_t)prev * W;
                bool same = true;
#pragma unroll
                for (int w = 0; w < W; ++w) same &= ka[w] == kb[w];
                if (same) { grp[a] = (uint32_t)prev; break; }
            }
            s = (s + 1) & capmask;
        }
    }
}

// one prefilter bit per seed (the windows that are their own seed), once the number of distinct seeds has sized the filter
template <int W>
__global__ void k_loc_prefilter(const uint64_t *keys, uint64_t n_windows, const uint32_t *grp, uint32_t *pf, uint32_t pfmask)
{
    for (uint64_t a = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; a < n_windows; a += (uint64_t)gridDim.x * blockDim.x) {
        if (grp[a] != (uint32_t)a) continue;
        const uint32_t bit = (uint32_t)(loc_hash<W>(keys + a * W) >> 32) & pfmask;
        atomicOr(&pf[bit >> 5], 1u << (bit & 31));
    }
}

// ---- scan -------------------------------------------------------------------------------------------------------------------
struct LocScan {
    const uint8_t *text;           // the chunk; `alloc` readable bytes (a multiple of 16), `n` of them text
    uint64_t n, alloc, goff;       // goff: position of text[0] in the whole genome text
    int Z;
    const uint64_t *keys;
    const unsigned long long *table;
    uint64_t capmask;
    const uint32_t *pf;
    uint32_t pfmask;
    uint32_t *occ;                 // per seed id: occurrences so far
    unsigned long long *ctr;       // [0] matches of this call, [1] valid windows, [2] prefilter passes, [3] matches (running totals)
    uint32_t *out_ids;
    uint64_t *out_pos;
    uint64_t cap;
    int count;                     // 0: this chunk was counted by the call that overflowed; append only
};

// the seed id of the window starting at tile-local base q, or LOC_EMPTY32
template <int W>
__device__ uint32_t loc_probe(const LocScan &p, const uint32_t *codes, uint32_t q, uint64_t h)
{
    uint64_t key[W];
    bool built = false;
    const uint32_t tag = (uint32_t)(h >> 32);
    uint64_t s = h & p.capmask;
    for (;;) {
        const unsigned long long e = p.table[s];
        if (e == LOC_EMPTY64) return LOC_EMPTY32;
        if ((uint32_t)(e >> 32) == tag) {
            if (!built) {
                LocRoll<W> roll;
                roll.clear();
                const int topbits = 2 * p.Z - 64 * (W - 1);
                for (int j = 0; j < p.Z; ++j) {
                    const uint32_t b = q + (uint32_t)j;
                    roll.push((codes[b >> 4] >> (2 * (b & 15))) & 3u, topbits);
                }
                roll.canonical(key);
                built = true;
            }
            const uint64_t *kb = p.keys + (uint64_t)(uint32_t)e * W;
            bool same = true;
#pragma unroll
            for (int w = 0; w < W; ++w) same &= key[w] == kb[w];
            if (same) return (uint32_t)e;
        }
        s = (s + 1) & p.capmask;
    }
}

template <int W>
__global__ __launch_bounds__(LOC_THREADS) void k_loc_scan(LocScan p)
{
    __shared__ uint32_t s_codes[LOC_WORDS];     // 16 bases per word, 2 bits each
    __shared__ uint16_t s_valid[LOC_WORDS];     // one bit per base
    const uint64_t tile_base = (uint64_t)blockIdx.x * LOC_TILE;
    // the tile and its overlap, 16 bytes of text per load, packed on the way into LDS
    for (uint32_t v = threadIdx.x; v < LOC_WORDS; v += LOC_THREADS) {
        const uint64_t byte0 = tile_base + 16ull * v;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (byte0 + 16 <= p.alloc) q = *reinterpret_cast<const uint4 *>(p.text + byte0);
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
        uint32_t cw = 0, vw = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t ok;
            const uint32_t c = loc_code((w4[i >> 2] >> (8 * (i & 3))) & 0xFFu, ok);
            ok &= (uint32_t)(byte0 + (uint64_t)i < p.n);
            cw |= c << (2 * i);
            vw |= ok << i;
        }
        s_codes[v] = cw;
        s_valid[v] = (uint16_t)vw;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    if (tile_base + (uint64_t)(threadIdx.x - lane) * LOC_RUN >= p.n) return;     // the whole wave starts behind the text

    const int Z = p.Z, topbits = 2 * Z - 64 * (W - 1);
    const int nwords = (LOC_RUN + Z - 1 + 15) >> 4;          // <= 12: word threadIdx.x * 4 + 11 <= LOC_WORDS - 1
    const uint32_t run0 = threadIdx.x * LOC_RUN;             // tile-local base the lane's run starts at
    LocRoll<W> roll;
    roll.clear();
    int good = 0;
    uint64_t n_valid = 0, n_pass = 0, n_match = 0;
    // the words in front of the run's first window end (Z - 1 bases, whole words of them) only fill the keys: nothing to hash
    const int nwarm = (Z - 1) >> 4;
    for (int wd = 0; wd < nwarm; ++wd) {
        const uint32_t cw = s_codes[threadIdx.x * (LOC_RUN / 16) + wd];
        const uint32_t vw = s_valid[threadIdx.x * (LOC_RUN / 16) + wd];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            roll.push((cw >> (2 * i)) & 3u, topbits);
            good = ((vw >> i) & 1u) ? good + 1 : 0;
        }
    }
    for (int wd = nwarm; wd < nwords; ++wd) {
        const uint32_t cw = s_codes[threadIdx.x * (LOC_RUN / 16) + wd];
        const uint32_t vw = s_valid[threadIdx.x * (LOC_RUN / 16) + wd];
        uint64_t h[16];
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            roll.push((cw >> (2 * i)) & 3u, topbits);
            good = ((vw >> i) & 1u) ? good + 1 : 0;
            uint64_t key[W];
            roll.canonical(key);
            h[i] = loc_hash<W>(key);
            const int start = wd * 16 + i - (Z - 1);          // the window ending at this base, relative to run0
            if (good >= Z && start >= 0 && start < LOC_RUN) vm |= 1u << i;
        }
        uint32_t cand = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t bit = (uint32_t)(h[i] >> 32) & p.pfmask;
            cand |= ((p.pf[bit >> 5] >> (bit & 31)) & 1u) << i;
        }
        cand &= vm;
        n_valid += __popc(vm);
        n_pass += __popc(cand);
        while (__ballot(cand != 0)) {
            const bool mine = cand != 0;
            const int sel = mine ? __ffs(cand) - 1 : 0;
            cand &= cand - 1;                                  // (0 stays 0)
            uint64_t hh = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) hh = (i == sel) ? h[i] : hh;
            const uint32_t start = (uint32_t)(wd * 16 + sel - (Z - 1));
            const uint32_t id = mine ? loc_probe<W>(p, s_codes, run0 + start, hh) : LOC_EMPTY32;
            const bool match = id != LOC_EMPTY32;
            const uint64_t m = __ballot(match);
            if (m) {                                           // one returning atomic per wave
                const int leader = __ffsll((unsigned long long)m) - 1;
                unsigned long long base = 0;
                if ((int)lane == leader) base = atomicAdd(&p.ctr[0], (unsigned long long)__popcll(m));
                base = __shfl(base, leader);
                if (match) {
                    const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (at < p.cap) {
                        p.out_ids[at] = id;
                        p.out_pos[at] = p.goff + tile_base + run0 + start;
                    }
                    if (p.count) atomicAdd(&p.occ[id], 1u);
                    ++n_match;
                }
            }
        }
    }
    if (p.count) {
        n_valid = wave_sum_u64(n_valid);
        n_pass = wave_sum_u64(n_pass);
        n_match = wave_sum_u64(n_match);
        if (lane == 0) {
            atomicAdd(&p.ctr[1], (unsigned long long)n_valid);
            atomicAdd(&p.ctr[2], (unsigned long long)n_pass);
            if (n_match) atomicAdd(&p.ctr[3], (unsigned long long)n_match);
        }
    }
}

inline unsigned loc_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096)); }
inline uint64_t loc_pow2(uint64_t n, uint64_t least) { uint64_t c = least; while (c < n) c <<= 1; return c; }

}  // namespace

struct kv_localize {
    int Z = 0, W = 0;
    uint64_t n_windows = 0, n_distinct = 0, capmask = 0;
    uint32_t pfmask = 0;
    uint64_t *d_keys = nullptr;
    unsigned long long *d_table = nullptr, *d_ctr = nullptr;
    uint32_t *d_pf = nullptr, *d_occ = nullptr;
    KvArena text;                           // the chunk being scanned; bytes, a multiple of 16
    KvArena ids, pos;                       // its matches: uint32_t contig ids, uint64_t positions
    bool ovf = false;                       // the last call overflowed its buffer at (ovf_off, ovf_len): its repeat must not count again
    uint64_t ovf_off = 0, ovf_len = 0;
    ~kv_localize()
    {
        void *all[] = {d_keys, d_table, d_ctr, d_pf, d_occ, text.p, ids.p, pos.p};
        for (void *p : all)
            if (p) (void)hipFree(p);
    }
};

// Prefilter size in bits (a power of two), from the number of DISTINCT seeds.  32 bits per seed while that fits 2 MiB, half of one XCD's L2, so the bit a window
// tests is an L2 hit beside the streamed text; more seeds than that keep the 2 MiB until one window in eight would pass, then the
// filter grows with the seeds (8 bits each) and leaves L2 for the Infinity Cache.
static uint64_t loc_prefilter_bits(uint64_t n_seeds)
{
    const uint64_t l2_bits = 1ull << 24;
    if (32 * n_seeds <= l2_bits) return loc_pow2(32 * n_seeds, 1ull << 13);
    if (8 * n_seeds <= l2_bits) return l2_bits;
    return std::min<uint64_t>(loc_pow2(8 * n_seeds, l2_bits), 1ull << 32);
}

extern "C" int kv_localize_create(const char *bases, const uint64_t *offsets, uint64_t n_contigs, int seedsize, uint32_t *seed_of_window,
                                  uint64_t n_windows, uint64_t *n_distinct, kv_localize **out)
{
    KV_REQUIRE(out && offsets && (bases || offsets[n_contigs] == 0) && n_distinct, KV_ERR_ARG, "kv_localize_create: null argument");
    KV_REQUIRE(seedsize >= 1 && seedsize <= LOC_MAX_Z, KV_ERR_ARG, "seed size must be 1..%d (got %d)", LOC_MAX_Z, seedsize);
    std::vector<uint64_t> wpre(n_contigs + 1, 0);
    for (uint64_t c = 0; c < n_contigs; ++c) {
        KV_REQUIRE(offsets[c] <= offsets[c + 1], KV_ERR_ARG, "kv_localize_create: contig offsets must not decrease");
        const uint64_t len = offsets[c + 1] - offsets[c];
        wpre[c + 1] = wpre[c] + (len >= (uint64_t)seedsize ? len - (uint64_t)seedsize + 1 : 0);
    }
    KV_REQUIRE(wpre[n_contigs] == n_windows, KV_ERR_ARG, "kv_localize_create: the contigs have %llu windows of length %d, not %llu",
               (unsigned long long)wpre[n_contigs], seedsize, (unsigned long long)n_windows);
    KV_REQUIRE(n_windows < 0x7FFFFFF0ull, KV_ERR_CAPACITY, "too many contig windows (%llu)", (unsigned long long)n_windows);
    KV_REQUIRE(n_windows == 0 || seed_of_window, KV_ERR_ARG, "kv_localize_create: null argument");
    hipStream_t st = kv_stream();
    kv_localize *h = new kv_localize;
    struct Guard { kv_localize *h; ~Guard() { delete h; } } guard{h};
    h->Z = seedsize;
    h->W = (seedsize + 31) / 32;
    h->n_windows = n_windows;
    const uint64_t cap = loc_pow2(2 * n_windows + 16, 1024);
    h->capmask = cap - 1;
    const uint64_t n_bases = offsets[n_contigs];
    uint8_t *d_bases = nullptr;
    uint64_t *d_off = nullptr, *d_wpre = nullptr;
    uint32_t *d_grp = nullptr;
    struct Tmp { void **p; ~Tmp() { if (*p) (void)hipFree(*p); } };
    Tmp t1{(void **)&d_bases}, t2{(void **)&d_off}, t3{(void **)&d_wpre}, t4{(void **)&d_grp};
    hipError_t e = kv_hip_malloc(&h->d_keys, std::max<uint64_t>(n_windows, 1) * h->W * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_table, cap * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_ctr, 64);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_occ, std::max<uint64_t>(n_windows, 1) * 4);
    if (e == hipSuccess) e = kv_hip_malloc(&d_bases, std::max<uint64_t>(n_bases, 16));
    if (e == hipSuccess) e = kv_hip_malloc(&d_off, (n_contigs + 1) * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&d_wpre, (n_contigs + 1) * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&d_grp, std::max<uint64_t>(n_windows, 1) * 4);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "seed table allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemsetAsync(h->d_table, 0xFF, cap * 8, st));
    KV_HIP(hipMemsetAsync(h->d_ctr, 0, 64, st));
    KV_HIP(hipMemsetAsync(h->d_occ, 0, std::max<uint64_t>(n_windows, 1) * 4, st));
    if (n_windows) {
        KV_HIP(hipMemcpyAsync(d_bases, bases, n_bases, hipMemcpyHostToDevice, st));
        KV_HIP(hipMemcpyAsync(d_off, offsets, (n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
        KV_HIP(hipMemcpyAsync(d_wpre, wpre.data(), (n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
        KvProfScope prof("k_loc_create");
        const dim3 grid(loc_grid(n_windows)), block(256);
#define LOC_CREATE(WW)                                                                                                              \
    do {                                                                                                                            \
        hipLaunchKernelGGL(k_loc_keys<WW>, grid, block, 0, st, d_bases, d_off, d_wpre, n_contigs, n_windows, seedsize, h->d_keys,   \
                           d_grp);                                                                                                  \
        hipLaunchKernelGGL(k_loc_group<WW>, grid, block, 0, st, h->d_keys, n_windows, h->d_table, h->capmask, d_grp, h->d_ctr + 4); \
    } while (0)
        switch (h->W) {
        case 1: LOC_CREATE(1); break;
        case 2: LOC_CREATE(2); break;
        case 3: LOC_CREATE(3); break;
        default: LOC_CREATE(4); break;
        }
#undef LOC_CREATE
    }
    KV_HIP(hipGetLastError());
    unsigned long long distinct = 0;
    if (n_windows) {
        KV_HIP(hipMemcpyAsync(seed_of_window, d_grp, n_windows * 4, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(&distinct, h->d_ctr + 4, 8, hipMemcpyDeviceToHost, st));
    }
    KV_HIP(hipStreamSynchronize(st));
    h->n_distinct = *n_distinct = distinct;
    const uint64_t pfbits = loc_prefilter_bits(distinct);
    h->pfmask = (uint32_t)(pfbits - 1);
    e = kv_hip_malloc(&h->d_pf, pfbits / 8);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "prefilter allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemsetAsync(h->d_pf, 0, pfbits / 8, st));
    if (n_windows) {
        KvProfScope prof("k_loc_create");
        const dim3 grid(loc_grid(n_windows)), block(256);
        switch (h->W) {
        case 1: hipLaunchKernelGGL(k_loc_prefilter<1>, grid, block, 0, st, h->d_keys, n_windows, d_grp, h->d_pf, h->pfmask); break;
        case 2: hipLaunchKernelGGL(k_loc_prefilter<2>, grid, block, 0, st, h->d_keys, n_windows, d_grp, h->d_pf, h->pfmask); break;
        case 3: hipLaunchKernelGGL(k_loc_prefilter<3>, grid, block, 0, st, h->d_keys, n_windows, d_grp, h->d_pf, h->pfmask); break;
        default: hipLaunchKernelGGL(k_loc_prefilter<4>, grid, block, 0, st, h->d_keys, n_windows, d_grp, h->d_pf, h->pfmask); break;
        }
        KV_HIP(hipGetLastError());
    }
    KV_HIP(hipStreamSynchronize(st));
    guard.h = nullptr;
    *out = h;
    return KV_OK;
}

extern "C" int kv_localize_scan(kv_localize *h, const char *text, uint64_t n_bytes, uint64_t global_offset, uint32_t *ids_out,
                                uint64_t *pos_out, uint64_t capacity, uint64_t *n_found)
{
    KV_REQUIRE(h && n_found && (text || n_bytes == 0) && (capacity == 0 || (ids_out && pos_out)), KV_ERR_ARG,
               "kv_localize_scan: null argument");
    KV_REQUIRE(n_bytes < (1ull << 40), KV_ERR_ARG, "kv_localize_scan: chunk of %llu bytes", (unsigned long long)n_bytes);
    *n_found = 0;
    const bool repeat = h->ovf && h->ovf_off == global_offset && h->ovf_len == n_bytes;
    h->ovf = false;
    if (n_bytes < (uint64_t)h->Z || h->n_distinct == 0) return KV_OK;
    hipStream_t st = kv_stream();
    hipError_t e = h->text.need_exact((n_bytes + 15) & ~15ull);
    if (e == hipSuccess) e = h->ids.need_exact(std::max<uint64_t>(capacity, 1) * 4);
    if (e == hipSuccess) e = h->pos.need_exact(std::max<uint64_t>(capacity, 1) * 8);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "scan buffers allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemcpyAsync(h->text.p, text, n_bytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemsetAsync(h->d_ctr, 0, 8, st));
    LocScan p;
    p.text = (const uint8_t *)h->text.p; p.n = n_bytes; p.alloc = h->text.bytes; p.goff = global_offset; p.Z = h->Z;
    p.keys = h->d_keys; p.table = h->d_table; p.capmask = h->capmask; p.pf = h->d_pf; p.pfmask = h->pfmask;
    p.occ = h->d_occ; p.ctr = h->d_ctr; p.out_ids = (uint32_t *)h->ids.p; p.out_pos = (uint64_t *)h->pos.p; p.cap = capacity; p.count = repeat ? 0 : 1;
    const uint64_t n_tiles = (n_bytes - (uint64_t)h->Z + 1 + LOC_TILE - 1) / LOC_TILE;
    KV_REQUIRE(n_tiles < 0x7FFFFFFFull, KV_ERR_ARG, "kv_localize_scan: chunk too large");
    {
        KvProfScope prof("k_loc_scan");
        const dim3 grid((unsigned)n_tiles), block(LOC_THREADS);
        switch (h->W) {
        case 1: hipLaunchKernelGGL(k_loc_scan<1>, grid, block, 0, st, p); break;
        case 2: hipLaunchKernelGGL(k_loc_scan<2>, grid, block, 0, st, p); break;
        case 3: hipLaunchKernelGGL(k_loc_scan<3>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(k_loc_scan<4>, grid, block, 0, st, p); break;
        }
    }
    KV_HIP(hipGetLastError());
    hipError_t re = hipSuccess;
    KvReadback rb;
    const unsigned long long *found = rb.add((const unsigned long long *)h->d_ctr, 1, st, &re);
    KV_HIP(re);
    KV_HIP(rb.wait(st));
    *n_found = *found;
    const uint64_t n_copy = std::min<uint64_t>(*found, capacity);
    if (n_copy) {
        KV_HIP(hipMemcpyAsync(ids_out, h->ids.p, n_copy * 4, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(pos_out, h->pos.p, n_copy * 8, hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
    }
    if (*found > capacity) { h->ovf = true; h->ovf_off = global_offset; h->ovf_len = n_bytes; }
    return KV_OK;
}

// kv_localize_scan over the text of a genome that sits in HBM (kv_genome.hip): nothing is uploaded.  All chunks append to the one
// pair of match buffers and are counted by the one d_ctr[0]; a chunk that begins on a 16-byte boundary is scanned where it lies,
// any other is copied to the handle's aligned chunk buffer first (k_loc_scan loads the text 16 bytes at a time).
extern "C" int kv_localize_scan_genome(kv_localize *h, kv_genome *g, uint64_t chunk_bytes, uint32_t *ids_out, uint64_t *pos_out, uint64_t capacity,
                                       uint64_t *n_found)
{
    KV_REQUIRE(h && g && n_found && (capacity == 0 || (ids_out && pos_out)), KV_ERR_ARG, "kv_localize_scan_genome: null argument");
    KvGenomeView gv;
    KV_STEP(kv_genome_view(g, &gv));
    KV_REQUIRE(gv.n < (1ull << 40), KV_ERR_ARG, "kv_localize_scan_genome: text of %llu bytes", (unsigned long long)gv.n);
    *n_found = 0;
    // (the uid of a genome, inverted, is no offset a chunk of an uploaded text has)
    const bool repeat = h->ovf && h->ovf_off == ~gv.uid && h->ovf_len == gv.n;
    h->ovf = false;
    if (gv.n < (uint64_t)h->Z || h->n_distinct == 0) return KV_OK;
    const GnScanPlan plan = gn_scan_plan(gv.n, (uint64_t)h->Z, chunk_bytes);
    KV_REQUIRE((plan.len + LOC_TILE - 1) / LOC_TILE < 0x7FFFFFFFull, KV_ERR_ARG, "kv_localize_scan_genome: chunk too large");
    hipStream_t st = kv_stream();
    hipError_t e = h->ids.need_exact(std::max<uint64_t>(capacity, 1) * 4);
    if (e == hipSuccess) e = h->pos.need_exact(std::max<uint64_t>(capacity, 1) * 8);
    if (e == hipSuccess && (plan.step & 15) && plan.n_chunks > 1) e = h->text.need_exact((plan.len + 15) & ~15ull);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "scan buffers allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemsetAsync(h->d_ctr, 0, 8, st));
    LocScan p;
    p.Z = h->Z;
    p.keys = h->d_keys; p.table = h->d_table; p.capmask = h->capmask; p.pf = h->d_pf; p.pfmask = h->pfmask;
    p.occ = h->d_occ; p.ctr = h->d_ctr; p.out_ids = (uint32_t *)h->ids.p; p.out_pos = (uint64_t *)h->pos.p; p.cap = capacity; p.count = repeat ? 0 : 1;
    {
        KvProfScope prof("k_loc_scan");
        for (uint64_t k = 0; k < plan.n_chunks; ++k) {
            const uint64_t start = k * plan.step, size = std::min<uint64_t>(plan.len, gv.n - start);
            if (size < (uint64_t)h->Z) break;
            if ((start & 15) == 0) {
                p.text = gv.text + start;
                p.alloc = std::min<uint64_t>((size + 15) & ~15ull, gv.alloc - start);
            } else {
                KV_HIP(hipMemcpyAsync(h->text.p, gv.text + start, size, hipMemcpyDeviceToDevice, st));
                p.text = (const uint8_t *)h->text.p;
                p.alloc = h->text.bytes & ~15ull;
            }
            p.n = size; p.goff = start;
            const uint64_t n_tiles = (size - (uint64_t)h->Z + 1 + LOC_TILE - 1) / LOC_TILE;
            const dim3 grid((unsigned)n_tiles), block(LOC_THREADS);
            switch (h->W) {
            case 1: hipLaunchKernelGGL(k_loc_scan<1>, grid, block, 0, st, p); break;
            case 2: hipLaunchKernelGGL(k_loc_scan<2>, grid, block, 0, st, p); break;
            case 3: hipLaunchKernelGGL(k_loc_scan<3>, grid, block, 0, st, p); break;
            default: hipLaunchKernelGGL(k_loc_scan<4>, grid, block, 0, st, p); break;
            }
        }
    }
    KV_HIP(hipGetLastError());
    hipError_t re = hipSuccess;
    KvReadback rb;
    const unsigned long long *found = rb.add((const unsigned long long *)h->d_ctr, 1, st, &re);
    KV_HIP(re);
    KV_HIP(rb.wait(st));
    *n_found = *found;
    const uint64_t n_copy = std::min<uint64_t>(*found, capacity);
    if (n_copy) {
        KV_HIP(hipMemcpyAsync(ids_out, h->ids.p, n_copy * 4, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(pos_out, h->pos.p, n_copy * 8, hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
    }
    if (*found > capacity) { h->ovf = true; h->ovf_off = ~gv.uid; h->ovf_len = gv.n; }
    return KV_OK;
}

extern "C" int kv_localize_counts(kv_localize *h, uint32_t *counts_out, uint64_t n_windows)
{
    KV_REQUIRE(h && (counts_out || n_windows == 0), KV_ERR_ARG, "kv_localize_counts: null argument");
    KV_REQUIRE(n_windows == h->n_windows, KV_ERR_ARG, "kv_localize_counts: the seed set has %llu windows, not %llu",
               (unsigned long long)h->n_windows, (unsigned long long)n_windows);
    if (n_windows) {
        hipStream_t st = kv_stream();
        KV_HIP(hipMemcpyAsync(counts_out, h->d_occ, n_windows * 4, hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
    }
    return KV_OK;
}

extern "C" int kv_localize_stats(kv_localize *h, uint64_t *stats_out)
{
    KV_REQUIRE(h && stats_out, KV_ERR_ARG, "kv_localize_stats: null argument");
    hipStream_t st = kv_stream();
    unsigned long long c[4] = {0, 0, 0, 0};
    KV_HIP(hipMemcpyAsync(c, h->d_ctr, sizeof(c), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    stats_out[0] = c[1]; stats_out[1] = c[2]; stats_out[2] = c[3]; stats_out[3] = h->n_distinct;
    return KV_OK;
}

extern "C" int kv_localize_destroy(kv_localize *h)
{
    if (h) {
        (void)hipStreamSynchronize(kv_stream());
        delete h;
    }
    return KV_OK;
}
