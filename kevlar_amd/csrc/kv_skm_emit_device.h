// kv_skm_emit_device.h -- device half of kv_skm.hip, stages S1 and S2: the geometry every stage shares (SkmGeom, its counters),
// the kernels that cut reads into super-k-mer records (k_skm_emit*) and the ones that split the coarse streams into fine
// buckets (k_skm_split*).  Included by kv_skm.hip only (one translation unit); the stages are described at its top.
#pragma once
#include "kv_binned.h"
#include "kv_novel_device.h"
#include "kv_skm_device.h"

struct SkmGeom {
    int k, m, w, wpow;               // wpow: largest power of two <= w
    int kw, nbw, recw, ncap;         // key words, base words and total words of a record, most k-mers of a record
    uint32_t C1, F2, fbits;          // coarse buckets, fine buckets per coarse bucket (2^fbits)
    uint32_t nwg1, nwg2, quota1;     // writers of S1 (persistent workgroups) and S2 (workgroups per coarse bucket)
    uint32_t cap1, cap2;             // records per private segment
    uint32_t np_max;                 // most bases any tile stages
    uint64_t stride;                 // record position = read * stride + offset
    uint64_t *seg1; uint32_t *cnt1;  // [C1][nwg1][cap1] records / [C1][nwg1]
    uint64_t *seg2; uint32_t *cnt2;  // [C1 * F2][nwg2][cap2] / [C1 * F2][nwg2]
    uint64_t *loose; uint64_t loose_cap;
    unsigned long long *ctr;         // [SKM_CTR_COUNT] counters, zeroed for every batch: the slots are the SkmCtr enumerators below
    uint32_t n_buckets, quota3;
    uint32_t sbw;                    // words of record-start bits per wave in the bucket walk
    uint64_t bucket_kmers;           // average k-mers per fine bucket
    uint32_t force_loose;            // KV_SKM_FORCE_LOOSE: k_skm_count sends one key in 64 through the loose list
    // abundance list the count pass writes (KvAbundList; abl_keys == nullptr: off): every workgroup appends to its own
    // stretch of abl_cap_wg entries and notes where each bucket's entries start
    uint64_t *abl_keys; uint8_t *abl_cnts; uint32_t *abl_bstart, *abl_bcount; uint32_t abl_cap_wg;
    // S2 over records that several ranks emitted (minimizer-sharded exchange, kv_skm_mex_route): seg1 / cnt1 then hold n_src
    // slabs of [C1][nwg1] segments one after the other, and a coarse bucket has n_src * nwg1 segments (0 / 1: the usual one slab)
    // distinct list the count pass writes for a batch that is going to be scanned (SkmIndex::dl; dl_keys == nullptr: off): EVERY
    // distinct k-mer of a bucket with its hash, appended like the abundance list (a stretch per workgroup, start + count per bucket)
    uint64_t *dl_keys, *dl_hash; uint32_t *dl_bstart, *dl_bcount; uint32_t dl_cap_wg;
    uint32_t dl_chunk, dl_nchunks;   // k_skm_route only: != 0 -- the list is a pool of dl_nchunks chunks of dl_chunk entries that the workgroups draw from (SKM_CTR_POOL_CHUNKS) instead of one stretch each
    uint32_t n_src;
    const uint64_t *seg1_off;        // non-null: segment `slot` starts at record seg1_off[slot] (compacted records) instead of slot * cap1
    uint64_t read_base;              // global index of the batch's first read (record positions of a read shard; 0 otherwise)
    // seg1 / cnt1 laid out [nwg1][C1] instead of [C1][nwg1]: a writer's ~250 open segments then lie within a few megabytes -- two or
    // three pages of the address translation -- instead of one every nwg1 x cap1 records (11 MB: a page each).  The exchange
    // layouts keep bucket-major order (a destination's coarse buckets must be contiguous: kv_skm_mex_pack).
    uint32_t seg1_wmajor;
    // compact: the records of this batch are 16-byte records without positions (kv_skm_device.h; recw = 2) -- a count into a sketch
    // that is not going to be scanned from this batch.  Loose records keep the classic form: lrecw = 1 + nbw words each.
    uint32_t compact;
    int lrecw;
    // (records are oriented: a record whose minimizer stands reversed in the read (strand bit of its value, skm_order_s) holds the
    // REVERSE COMPLEMENT of the read's bases (header flag), so every k-mer of every record is stored on the strand on which its minimizer
    // is canonical -- and that strand is the k-mer's key in the bucket tables: the walk takes k-mers as they stand, no second strand, no
    // comparison.  The exchange layouts cut them the same way.)
    uint32_t passes;                 // k_skm_route takes a bucket's k-mers in at least this many passes (0 / 1: one) -- buckets bigger than its LDS table
    uint32_t bpt;                    // buckets per ticket of the bucket kernels' work counter (a power of two)
};

// the slots of SkmGeom::ctr
enum SkmCtr {
    SKM_CTR_LOOSE = 0,               // records on the loose list
    SKM_CTR_FAIL = 1,                // failure flag: a record was lost (loose list overflow), a table could not take a key, or the pass was given up
    SKM_CTR_TICKET_S1 = 2, SKM_CTR_TICKET_COUNT = 3, SKM_CTR_TICKET_SCAN = 4,     // work tickets of S1 (tiles), of the count / route pass and of the scan (buckets)
    SKM_CTR_RECORDS = 5,             // records S1 emitted
    SKM_CTR_LOOSE_S12 = 6,           // loose records S1 + S2 left behind (the host copies SKM_CTR_LOOSE here before the bucket kernels add theirs)
    SKM_CTR_DISTINCT = 7,            // distinct k-mers the count / route pass found in its LDS tables
    SKM_CTR_ARRIVED = 8,             // k-mer occurrences that arrived at an exchange owner (k_mex_sum_kmers)
    SKM_CTR_DL_RAN_OUT = 9,          // workgroups whose stretch of the distinct list ran out, or draws from its pool of chunks that found it empty
    SKM_CTR_SET_HITS = 10,           // hits kv_skm_mex_scan_set stored (SetHitSink::count)
    SKM_CTR_POOL_CHUNKS = 13,        // (nothing uses 11 and 12) chunks drawn from the distinct list's pool (k_skm_route, dl_chunk != 0)
    SKM_CTR_COUNT
};
// the slots of other stages' counters that kernels here touch: BinGeom::ctr (kv_binned.h), KvRouteSink::ctr (kv_internal.h)
enum { BIN_CTR_FAIL = 1, BIN_CTR_ADDED = 2, ROUTE_CTR_OVERFLOW = 1, ROUTE_CTR_DEST0 = 18 };

// segment `seg` of coarse bucket c in seg1 / cnt1, counted in segments
__device__ __forceinline__ uint64_t skm_seg1_slot(const SkmGeom &sg, uint32_t c, uint32_t seg)
{
    if (sg.seg1_wmajor) return (uint64_t)seg * sg.C1 + c;
    if (sg.n_src <= 1u) return (uint64_t)c * sg.nwg1 + seg;
    const uint32_t src = seg / sg.nwg1, w = seg - src * sg.nwg1;
    return ((uint64_t)src * sg.C1 + c) * sg.nwg1 + w;
}
__device__ __forceinline__ uint32_t skm_seg1_count(const SkmGeom &sg) { return sg.nwg1 * (sg.n_src > 1u ? sg.n_src : 1u); }
// first record of segment `slot`
__device__ __forceinline__ uint64_t skm_seg1_first(const SkmGeom &sg, uint64_t slot) { return sg.seg1_off ? sg.seg1_off[slot] : slot * sg.cap1; }

namespace {

#define SKM_THREADS1 512
#define SKM_S1_WAVE_THREADS_DEFAULT 512u      // threads per workgroup of k_skm_emit_wave (1024: one workgroup per CU, see the kernel)
// One global counter hands out work; a returning atomic on one word saturates at ~90 per microsecond on this chip
// (MI355X_MICROARCH.md, "dequeue"), i.e. 1.3 ms for the 117 k tiles of a 7.5 M-read sample if every tile were a
// ticket.  A ticket therefore covers several units of work.
#define SKM_TILES_PER_TICKET 8u

// (32-byte records -- one aligned sector each, two 16-byte stores -- were measured against these 24-byte ones: WRITE_SIZE
// fell from 2.5 to 2.3 GB per sample for 1.3 / 1.7 GB stored, the readers fetched 0.4 GB more each, times did not move.)
// a record in as few store instructions as its size allows (every lane of a scattered store is its own cache line: the memory pipe
// takes an instruction's 64 lines one by one, so three 8-byte stores cost three passes where a 16-byte and an 8-byte one cost two)
__device__ __forceinline__ void skm_store_record_wide(uint64_t *dst, uint64_t hdr, const uint64_t *bw, int nbw)
{
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2), aligned(8)));
    *(u64x2 *)dst = u64x2{hdr, bw[0]};
    if (nbw == 2) dst[2] = bw[1];
    else if (nbw == 3) *(u64x2 *)(dst + 2) = u64x2{bw[1], bw[2]};
}

__device__ __forceinline__ void skm_store_record(uint64_t *dst, uint64_t hdr, const uint64_t *bw, int nbw)
{
    dst[0] = hdr;
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (t < nbw) dst[1 + t] = bw[t];
}

__device__ __forceinline__ void skm_loose_push(const SkmGeom &sg, uint64_t hdr, const uint64_t *bw)
{
    const unsigned long long idx = atomicAdd(&sg.ctr[SKM_CTR_LOOSE], 1ull);
    if (idx < sg.loose_cap) skm_store_record(sg.loose + idx * (uint64_t)sg.lrecw, hdr, bw, sg.nbw);
    else sg.ctr[SKM_CTR_FAIL] = 1;
}

// ---- S1 ------------------------------------------------------------------------------------------------
struct SkmTile {
    uint32_t len[KV_TILE_MAX_READS], nk[KV_TILE_MAX_READS];
    uint32_t bpre[KV_TILE_MAX_READS + 1];      // staged-base prefix: flat position of a read's first base
    uint32_t wpre[KV_TILE_MAX_READS + 1];      // packed-word prefix inside the tile
    uint32_t cpre[KV_TILE_MAX_READS + 1];      // chunk prefix (a chunk = CH consecutive k-mer starts of one read)
    uint32_t uni_wpr, uni_cpr, uni_len;        // words / chunks / bases per read if all reads of the tile have the same length, else 0
    float inv_wpr, inv_cpr, inv_len;
    uint32_t seg_start, read0, next_tile;
    uint32_t wtot[3][SKM_THREADS1 / 64];       // run starts per (round, wave)
};

// q / d for q < 2^16 with the precomputed float reciprocal (off by at most one before the fix-up)
__device__ __forceinline__ uint32_t skm_div(uint32_t q, uint32_t d, float inv)
{
    uint32_t r = (uint32_t)((float)q * inv);
    if (r * d > q) r -= 1;
    else if ((r + 1) * d <= q) r += 1;
    return r;
}

__device__ __forceinline__ uint32_t skm_search(const uint32_t *pre, uint32_t n, uint32_t q)
{
    uint32_t lo = 0, hi = n;      // largest r with pre[r] <= q (empty entries share their successor's prefix)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// CH consecutive k-mer starts per thread in the window-minimum pass; needs w > CH
template <int CH>
__global__ __launch_bounds__(SKM_THREADS1, 6) void k_skm_emit(ReadsDev rd, uint32_t n_tiles, SkmGeom sg)   // 6 waves per SIMD: three workgroups per CU
{
    __shared__ SkmTile sh;
    __shared__ uint32_t cur[256];
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t nwl = sg.np_max / 16u + KV_TILE_MAX_READS + 8u;     // every read starts on a word: up to one partial word each
    uint32_t *wl = smem;                                              // the tile's packed words
    uint32_t *mh = smem + nwl;                                        // order value of the m-mer starting at every base
    uint16_t *starts = (uint16_t *)(mh + sg.np_max + 96u);            // run starts (flat positions < 2^16), in position order
    const int k = sg.k, m = sg.m, w = sg.w;
    const int lane = threadIdx.x & 63;
    for (uint32_t c = threadIdx.x; c < sg.C1; c += SKM_THREADS1) cur[c] = 0;
    if (threadIdx.x == 0) sh.next_tile = (uint32_t)atomicAdd(&sg.ctr[SKM_CTR_TICKET_S1], 1ull) * SKM_TILES_PER_TICKET;
    uint64_t n_rec = 0;
    // Batches of equal-length reads (rd.uni_len): the layout of a tile is arithmetic, so the packed words of the NEXT
    // tile are requested while this one is processed (two registers per thread) and the per-tile chain of dependent loads
    // -- tile descriptor, word offsets, lengths, words: half of this kernel's time went there -- disappears.
    const bool uni = rd.uni_len != 0;
    const uint32_t uni_wpr = (rd.uni_len + 15u) >> 4;
    uint32_t pf0 = 0, pf1 = 0, pf_tile = 0xffffffffu;
    auto prefetch = [&](uint32_t tile) {
        pf_tile = tile;
        if (tile >= n_tiles) return;
        const uint64_t r0 = (uint64_t)tile * rd.uni_per_tile;
        const uint32_t nr = (uint32_t)min((uint64_t)rd.uni_per_tile, rd.n_reads - r0), nw = nr * uni_wpr;
        const uint32_t *src = rd.words + r0 * uni_wpr;
        pf0 = threadIdx.x < nw ? src[threadIdx.x] : 0u;
        pf1 = threadIdx.x + SKM_THREADS1 < nw ? src[threadIdx.x + SKM_THREADS1] : 0u;
    };
    if (uni) {
        __syncthreads();
        prefetch(sh.next_tile);
    }
    for (uint32_t taken = 0; taken < sg.quota1; ++taken) {
        __syncthreads();                                   // previous tile finished, ticket visible
        const uint32_t tile = sh.next_tile;
        if (tile >= n_tiles) break;
        TileDesc td;
        if (uni) { td.first = tile * rd.uni_per_tile; td.count = (uint32_t)min((uint64_t)rd.uni_per_tile, rd.n_reads - td.first); td.seg_start = 0; td.seg = 0; }
        else td = rd.tile[tile];
        const uint32_t r0 = td.first, nr = td.count;
        const uint32_t seg_start = td.seg ? td.seg_start : 0u;
        const uint64_t w0 = uni ? (uint64_t)r0 * uni_wpr : rd.woff[r0] + (seg_start >> 4);
        uint32_t nwords;
        if (uni) {
            nwords = nr * uni_wpr;
        } else if (td.seg) {
            const uint32_t rest = rd.len[r0] - seg_start, want = (uint32_t)KV_SEG_BASES + (uint32_t)k - 1u;
            nwords = ((rest < want ? rest : want) + 15u) >> 4;
        } else {
            nwords = (uint32_t)(rd.woff[r0 + nr] - w0);
        }
        if (uni) {
            if (threadIdx.x < 64) {
                const uint32_t i0 = 2 * threadIdx.x, i1 = i0 + 1, L = rd.uni_len;
                const uint32_t kk = L >= (uint32_t)k ? L - (uint32_t)k + 1u : 0u, cc = (kk + CH - 1) / CH;
                if (i0 < nr) { sh.len[i0] = L; sh.nk[i0] = kk; sh.bpre[i0] = i0 * L; sh.cpre[i0] = i0 * cc; sh.wpre[i0] = i0 * uni_wpr; }
                if (i1 < nr) { sh.len[i1] = L; sh.nk[i1] = kk; sh.bpre[i1] = i1 * L; sh.cpre[i1] = i1 * cc; sh.wpre[i1] = i1 * uni_wpr; }
                if (threadIdx.x == 0) {
                    sh.bpre[nr] = nr * L; sh.cpre[nr] = nr * cc; sh.wpre[nr] = nr * uni_wpr; sh.seg_start = 0; sh.read0 = r0;
                    const bool okk = L >= (uint32_t)k;
                    sh.uni_wpr = okk ? uni_wpr : 0u; sh.uni_cpr = okk ? cc : 0u;
                    sh.inv_wpr = okk ? 1.0f / (float)uni_wpr : 0.0f; sh.inv_cpr = okk ? 1.0f / (float)cc : 0.0f;
                    sh.uni_len = okk ? L : 0u; sh.inv_len = okk ? 1.0f / (float)L : 0.0f;
                }
            }
        } else if (threadIdx.x < 64) {
            const uint32_t i0 = 2 * threadIdx.x, i1 = i0 + 1;
            uint32_t l0 = 0, l1 = 0;
            if (i0 < nr) {
                l0 = rd.len[r0 + i0];
                if (td.seg) {
                    const uint32_t rest = l0 - seg_start, want = (uint32_t)KV_SEG_BASES + (uint32_t)k - 1u;
                    l0 = rest < want ? rest : want;
                }
            }
            if (i1 < nr) l1 = rd.len[r0 + i1];
            const uint32_t k0 = l0 >= (uint32_t)k ? l0 - (uint32_t)k + 1u : 0u, k1 = l1 >= (uint32_t)k ? l1 - (uint32_t)k + 1u : 0u;
            const uint32_t c0 = (k0 + CH - 1) / CH, c1 = (k1 + CH - 1) / CH;
            uint32_t eb, tot, ecb, ctot;
            const uint32_t ea = wave_excl_scan2(l0, l1, eb, tot);
            const uint32_t eca = wave_excl_scan2(c0, c1, ecb, ctot);
            if (i0 < nr) { sh.len[i0] = l0; sh.nk[i0] = k0; sh.bpre[i0] = ea; sh.cpre[i0] = eca; }
            if (i1 < nr) { sh.len[i1] = l1; sh.nk[i1] = k1; sh.bpre[i1] = eb; sh.cpre[i1] = ecb; }
            if (threadIdx.x == 0) { sh.bpre[nr] = tot; sh.cpre[nr] = ctot; sh.seg_start = seg_start; sh.read0 = r0; }
            const uint32_t ref = __shfl(l0, 0);
            const bool same = (i0 >= nr || l0 == ref) && (i1 >= nr || l1 == ref);
            const bool uniform = __all(same) && ref >= (uint32_t)k;
            if (threadIdx.x == 0) {
                const uint32_t wpr = (ref + 15u) >> 4, cpr = (ref - (uint32_t)k + 1u + CH - 1) / CH;
                sh.uni_wpr = uniform ? wpr : 0u; sh.uni_cpr = uniform ? cpr : 0u;
                sh.inv_wpr = uniform ? 1.0f / (float)wpr : 0.0f; sh.inv_cpr = uniform ? 1.0f / (float)cpr : 0.0f;
                sh.uni_len = uniform ? ref : 0u; sh.inv_len = uniform ? 1.0f / (float)ref : 0.0f;
            }
            if (td.seg) {
                if (threadIdx.x == 0) { sh.wpre[0] = 0; sh.wpre[1] = (l0 + 15) >> 4; }
            } else {
                if (i0 < nr) sh.wpre[i0] = (uint32_t)(rd.woff[r0 + i0] - w0);
                if (i1 < nr) sh.wpre[i1] = (uint32_t)(rd.woff[r0 + i1] - w0);
                if (threadIdx.x == 0) sh.wpre[nr] = (uint32_t)(rd.woff[r0 + nr] - w0);
            }
        }
        if (uni && pf_tile == tile && nwords + 8u <= 2u * SKM_THREADS1) {
            wl[threadIdx.x] = pf0;                                             // (zero beyond the tile's words)
            if (threadIdx.x + SKM_THREADS1 < nwords + 8u) wl[threadIdx.x + SKM_THREADS1] = pf1;
        } else {
            for (uint32_t i = threadIdx.x; i < nwords + 8u; i += SKM_THREADS1) wl[i] = i < nwords ? rd.words[w0 + i] : 0u;
        }
        __syncthreads();
        // the next ticket is fetched while this tile is processed (everybody has read the current one by now)
        if (threadIdx.x == 0) {
            if ((tile + 1u) % SKM_TILES_PER_TICKET) sh.next_tile = tile + 1u;       // same ticket
            else sh.next_tile = taken + 1 < sg.quota1 ? (uint32_t)atomicAdd(&sg.ctr[SKM_CTR_TICKET_S1], 1ull) * SKM_TILES_PER_TICKET : 0xffffffffu;
        }
        const uint32_t NB = sh.bpre[nr];
        // P1: one thread per packed word: the order values of the m-mers starting at its 16 bases
        const uint32_t mmask = m == 16 ? 0xffffffffu : ((1u << (2 * m)) - 1u);
        for (uint32_t wi = threadIdx.x; wi < nwords; wi += SKM_THREADS1) {
            const uint32_t r = sh.uni_wpr ? skm_div(wi, sh.uni_wpr, sh.inv_wpr) : skm_search(sh.wpre, nr, wi);
            const uint32_t j0 = (wi - sh.wpre[r]) * 16u, L = sh.len[r];
            const uint32_t q0 = sh.bpre[r] + j0;
            const uint64_t win = (uint64_t)wl[wi] | ((uint64_t)wl[wi + 1] << 32);
            // the reverse complement of all 32 bases once: base i of `win`, complemented, is base 31 - i of `rcw`, so the reverse
            // complement of the m-mer at base jj is the m-mer of rcw at base 32 - m - jj (m <= 16, jj <= 15)
            const uint64_t rcw = ~skm_rev2_64(win);
            const uint32_t rc0 = 2u * (32u - (uint32_t)m);
            // lane l starts at base l mod 16 of its word: the 64 stores of one instruction then fall into different banks
#pragma unroll
            for (int step = 0; step < 16; ++step) {
                const uint32_t jj = ((uint32_t)step + (uint32_t)lane) & 15u, j = j0 + jj;
                const uint32_t f = (uint32_t)(win >> (2u * jj)) & mmask, r = (uint32_t)(rcw >> (rc0 - 2u * jj)) & mmask;
                if (j < L) mh[q0 + jj] = j + (uint32_t)m <= L ? skm_order_s(f, r) : 0xffffffffu;
            }
        }
        if (threadIdx.x < 96) mh[NB + threadIdx.x] = 0xffffffffu;
        __syncthreads();
        if (uni) prefetch(sh.next_tile);                   // written before this barrier; lands during P2 .. P4
        // P2: one thread per chunk of CH k-mer starts: the minimum over the w m-mers of each (shared suffix of the chunk + the
        // w - 1 - CH values every window contains + a growing prefix) and where it changes.  A run is a stretch of k-mers with the
        // same minimizer VALUE (its bucket is a function of that value, taken once per run in P4; two values that share a bucket
        // -- one pair in C1 x F2 -- merely give two records where one would have done).
        const uint32_t nchunks = sh.cpre[nr];                                      // <= 8192 / CH + 64 < 3 * SKM_THREADS1
        const uint32_t nrounds = (nchunks + SKM_THREADS1 - 1u) / SKM_THREADS1;
        uint32_t my_q[3], my_starts[3];
#pragma unroll
        for (int round = 0; round < 3; ++round) {
            const uint32_t ci = (uint32_t)round * SKM_THREADS1 + threadIdx.x;
            uint32_t startmask = 0, q = 0;
            if (ci < nchunks) {
                const uint32_t r = sh.uni_cpr ? skm_div(ci, sh.uni_cpr, sh.inv_cpr) : skm_search(sh.cpre, nr, ci);
                const uint32_t j = (ci - sh.cpre[r]) * CH, nkr = sh.nk[r];
                q = sh.bpre[r] + j;
                uint32_t suf[CH + 1];                     // suf[i + 1] = min(mh[q + i .. q + CH - 1]), i = -1 .. CH - 1
                uint32_t run = 0xffffffffu;
#pragma unroll
                for (int i = CH - 1; i >= 0; --i) { run = min(run, mh[q + i]); suf[i + 1] = run; }
                suf[0] = j > 0 ? min(run, mh[q - 1]) : run;
                uint32_t mid = 0xffffffffu;
                for (uint32_t t = CH; t + 2 <= (uint32_t)w; ++t) mid = min(mid, mh[q + t]);     // mh[q + CH .. q + w - 2]
                uint32_t prev = min(suf[0], mid);         // minimizer of the k-mer in front of the chunk (unused when j == 0)
                uint32_t diff = j == 0 ? 1u : 0u;
                run = 0xffffffffu;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    run = min(run, mh[q + (uint32_t)w - 1u + i]);
                    const uint32_t v = min(min(suf[i + 1], mid), run);
                    diff |= (v != prev ? 1u : 0u) << i;
                    prev = v;
                }
                const uint32_t nv = min((uint32_t)CH, nkr - j);          // k-mers of the read that start in this chunk (>= 1)
                startmask = diff & ((2u << (nv - 1u)) - 1u);
            }
            my_q[round] = q; my_starts[round] = startmask;
        }
        // run starts in position order (chunks are numbered in position order): prefix over lanes, waves, rounds
        uint32_t incl[3] = {0u, 0u, 0u};
#pragma unroll
        for (int round = 0; round < 3; ++round) {
            if ((uint32_t)round < nrounds) {
                const uint32_t v = wave_incl_scan((uint32_t)__popc(my_starts[round]));
                incl[round] = v;
                if (lane == 63) sh.wtot[round][threadIdx.x >> 6] = v;
            }
        }
        __syncthreads();
        uint32_t nstart = 0;
#pragma unroll
        for (int round = 0; round < 3; ++round) {
            if ((uint32_t)round < nrounds) {
                uint32_t before = nstart;
                for (uint32_t wv = 0; wv < SKM_THREADS1 / 64; ++wv) {
                    const uint32_t n = sh.wtot[round][wv];
                    if (wv < (threadIdx.x >> 6)) before += n;
                    nstart += n;
                }
                uint32_t base = before + incl[round] - (uint32_t)__popc(my_starts[round]);
                uint32_t bits = my_starts[round];
                while (bits) {
                    const int i = __ffs((int)bits) - 1;
                    bits &= bits - 1;
                    starts[base++] = (uint16_t)(my_q[round] + (uint32_t)i);
                }
            }
        }
        __syncthreads();
        // P4: one thread per run: measure it, cut it into records of <= ncap k-mers, store them
        for (uint32_t i = threadIdx.x; i < nstart; i += SKM_THREADS1) {
            const uint32_t q = starts[i];
            const uint32_t r = sh.uni_len ? skm_div(q, sh.uni_len, sh.inv_len) : skm_search(sh.bpre, nr, q), j = q - sh.bpre[r];
            const uint32_t limit = q - j + sh.nk[r];          // flat position one past the read's last k-mer
            const uint32_t nxt = i + 1 < nstart ? (uint32_t)starts[i + 1] : limit;     // the next run (of this read or a later one)
            uint32_t left = (nxt < limit ? nxt : limit) - q;
            uint32_t minv = 0xffffffffu;
            for (uint32_t t = 0; t < (uint32_t)w; ++t) minv = min(minv, mh[q + t]);
            uint32_t coarse, fine;
            skm_bucket_of(minv, sg.C1, sg.fbits, coarse, fine);
            uint64_t pos = (sg.read_base + sh.read0 + r) * sg.stride + sh.seg_start + j;
            uint32_t b = sh.wpre[r] * 16u + j;                // base index inside wl
            while (left) {
                const uint32_t n = min(left, (uint32_t)sg.ncap);
                uint64_t bw[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? skm_bases32(wl, b + 32u * t) : 0ull;
                const uint32_t rev = minv & 1u;
                if (rev) skm_rc_bases(bw, sg.nbw, n + (uint32_t)k - 1u);
                const uint64_t hdr = skm_header(pos, n, fine, rev);
                const uint32_t p = atomicAdd(&cur[coarse], 1u);
                if (p < sg.cap1) skm_store_record(sg.seg1 + (skm_seg1_slot(sg, coarse, blockIdx.x) * sg.cap1 + p) * (uint64_t)sg.recw, hdr, bw, sg.nbw);
                else skm_loose_push(sg, hdr, bw);
                n_rec += 1;
                left -= n; pos += n; b += n;
            }
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < sg.C1; c += SKM_THREADS1) sg.cnt1[skm_seg1_slot(sg, c, blockIdx.x)] = min(cur[c], sg.cap1);
    n_rec = wave_sum_u64(n_rec);
    if ((threadIdx.x & 63) == 0 && n_rec) atomicAdd(&sg.ctr[SKM_CTR_RECORDS], (unsigned long long)n_rec);
}

// ---- S1, batches of equal-length reads: a wave per group of reads -----------------------------------------------
// The tile kernel above spends most of its time parked: six workgroup barriers per tile, between phases that keep 60-80 % of
// the lanes busy, and a phase is as slow as its slowest wave (dissected: skeleton 0.37 ms, order values 0.37, minima + run
// starts 0.43, records 0.30, their stores 0.43 per 7.5 M reads).  When every read of the batch has the same length the layout
// is arithmetic, so a WAVE can take R consecutive reads (R x words per read <= 64: one packed word per lane) through the same
// four phases on its own slice of LDS with no workgroup barrier at all -- only the order of its own LDS operations -- and the
// 24 waves of a CU are in different phases at any time.  The workgroup still shares the coarse cursors and its segments.
#define SKM_MT_PER_TICKET 64u     // 1 M groups per 7.5 M reads: one device-wide counter takes ~90 updates per microsecond (16 per ticket: 0.74 ms of the kernel)
#define SKM_WAVE_RUNS 128u        // runs of a group listed at a time (a group has ~55; more go round again)
// Flat position of base j of the group's read r: r * Lp + j with Lp = 16 * words per read, so a position is also the base index
// into the staged words.  Order values live at mh[p + (p >> PS)], PS = log2(CH): a padding word per chunk, so that lanes that
// walk consecutive chunks (P2) or consecutive words (P1) hit different banks and every offset inside a chunk is a constant.
__host__ __device__ inline uint32_t skm_wave_slice_words(uint32_t R, uint32_t L, uint32_t nk, int ch)
{
    const uint32_t lp = 16u * ((L + 15u) >> 4), pmax = R * lp + 96u;
    (void)nk;
    return 132u + pmax + pmax / (uint32_t)ch + 2u + SKM_WAVE_RUNS + (SKM_WAVE_RUNS + 2u) / 2u;      // words (twice), order values, minimizer + start of SKM_WAVE_RUNS runs at a time
}

// THREADS: 512 (three workgroups per CU, 768 writers) or 1024 (ONE workgroup of 16 waves per CU, 256 writers).  A writer keeps one
// open cache line per coarse bucket, and the L2 of an XCD (4 MB) merges a record's 16- and 8-byte stores into whole lines only while
// the open lines of the XCD's workgroups fit beside the rest of its traffic: 251 buckets x 96 workgroups x 128 B = 3 MB do not
// (WRITE_SIZE 2.5-2.7 GB per 1.36 GB of records, measured with 512 and with 768 writers), 251 x 32 x 128 B = 1 MB do (1.0 x).
template <int CH, int THREADS>
__global__ __launch_bounds__(THREADS, THREADS == 1024 ? 4 : 6) void k_skm_emit_wave(ReadsDev rd, SkmGeom sg, uint32_t R, uint32_t n_mt, uint32_t quota_mt, uint32_t per_ticket)
{
    constexpr uint32_t PS = CH == 16 ? 4u : 3u;
    __shared__ uint32_t cur[256];
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t wave = threadIdx.x >> 6;
    const int k = sg.k, m = sg.m, w = sg.w;
    const uint32_t L = rd.uni_len, wpr = (L + 15u) >> 4, Lp = 16u * wpr, nk = L - (uint32_t)k + 1u, cpr = (nk + CH - 1) / CH;
    const float inv_wpr = 1.0f / (float)wpr, inv_cpr = 1.0f / (float)cpr;
    const uint32_t pmax = R * Lp + 96u;
    uint32_t *wl0 = smem + wave * skm_wave_slice_words(R, L, nk, CH), *mh = wl0 + 132u;
    uint32_t *sval = mh + pmax + pmax / CH + 2u;
    uint16_t *starts = (uint16_t *)(sval + SKM_WAVE_RUNS);
    for (uint32_t c = threadIdx.x; c < sg.C1; c += THREADS) cur[c] = 0;
    if ((threadIdx.x & 63u) < 2u) { wl0[64u + (threadIdx.x & 63u)] = 0; wl0[130u + (threadIdx.x & 63u)] = 0; }
    __syncthreads();
    const uint32_t mmask = m == 16 ? 0xffffffffu : ((1u << (2 * m)) - 1u);
    const uint32_t rc0 = 2u * (32u - (uint32_t)m);
    uint64_t n_rec = 0;
    uint64_t *const my_seg = sg.seg1 + skm_seg1_slot(sg, 0u, blockIdx.x) * sg.cap1 * (uint64_t)sg.recw;       // + coarse * cstride: this workgroup's segment of a coarse bucket
    const uint64_t cstride = (sg.seg1_wmajor ? 1ull : (uint64_t)sg.nwg1) * sg.cap1 * (uint64_t)sg.recw;
    uint32_t mt = 0, mt_end = 0, taken = 0, pf = 0, pf_mt = 0xffffffffu, parity = 0;
    for (;;) {
        // (everything P1 and P2 derive from the lane number alone is the same for every group; left to itself the compiler
        // computes all of it once in front of the loop -- 16 shift pairs, 32 lane masks -- and spills it: 196 bytes of scratch
        // per lane and two reloads per order value.  An opaque copy of the lane number keeps the arithmetic where it is used.)
        uint32_t lane = threadIdx.x & 63u;
        asm volatile("" : "+v"(lane));
        auto words_of = [&](uint32_t t) -> uint32_t {
            const uint64_t r0 = (uint64_t)t * R;
            const uint32_t nr = (uint32_t)min((uint64_t)R, rd.n_reads - r0);
            return lane < nr * wpr ? rd.words[r0 * wpr + lane] : 0u;
        };
        if (mt == mt_end) {
            if (taken >= quota_mt) break;
            uint32_t t = 0;
            if (lane == 0) t = (uint32_t)atomicAdd(&sg.ctr[SKM_CTR_TICKET_S1], 1ull);
            t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
            if ((uint64_t)t * per_ticket >= n_mt) break;
            mt = t * per_ticket;
            mt_end = min(mt + per_ticket, n_mt);
        }
        const uint64_t r0 = (uint64_t)mt * R;
        const uint32_t nr = (uint32_t)min((uint64_t)R, rd.n_reads - r0), nwords = nr * wpr;
        // The next group's words are requested now and WAITED FOR in front of P4: a wait at the top of the next round would also
        // wait for this round's record stores (one counter, in order), i.e. for a round trip to HBM per group.
        uint32_t *wl = wl0 + 66u * parity;
        uint32_t word;
        if (pf_mt == mt) word = pf;                               // (already in the other buffer's place: stored below)
        else { word = words_of(mt); wl[lane] = word; }
        const bool more = mt + 1u < mt_end;
        if (more) { pf = words_of(mt + 1u); pf_mt = mt + 1u; }
        // P1: the order values of the m-mers starting at the 16 bases of this lane's word.  (Values of m-mers that run past the
        // end of their read are garbage: no window of a k-mer of the read contains them.)
        if (lane < nwords) {
            const uint32_t up = (uint32_t)__shfl_down((int)word, 1);
            const uint64_t win = (uint64_t)word | ((uint64_t)(lane == 63u ? 0u : up) << 32);
            const uint64_t rcw = ~skm_rev2_64(win);
            uint32_t *dst = mh + 16u * lane + (CH == 16 ? lane : 2u * lane);
#pragma unroll
            for (int step = 0; step < 16; ++step) {
                const uint32_t f = (uint32_t)(win >> (2 * step)) & mmask, rv = (uint32_t)(rcw >> (rc0 - 2u * (uint32_t)step)) & mmask;
                dst[step + (step >> PS)] = skm_order_s(f, rv);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // P2: a lane per chunk of CH k-mer starts: window minima (shared suffix of the chunk + the values every window of the chunk
        // contains + a growing prefix) and where they change; then every run start with its minimizer, in position order
        const uint32_t nchunks = nr * cpr;
        uint32_t startmask = 0, q = 0;
        uint32_t v[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) v[i] = 0;
        if (lane < nchunks) {
            const uint32_t r = skm_div(lane, cpr, inv_cpr);
            const uint32_t j = (lane - r * cpr) * CH;
            q = r * Lp + j;                                   // a multiple of CH
            const uint32_t *src = mh + q + (q >> PS);
            auto at = [&](uint32_t i) -> uint32_t { return src[i + (i >> PS)]; };       // i: constant offsets from the chunk's first value
            uint32_t suf[CH + 1];
            uint32_t run = 0xffffffffu;
#pragma unroll
            for (int i = CH - 1; i >= 0; --i) { run = min(run, at((uint32_t)i)); suf[i + 1] = run; }
            suf[0] = j > 0 ? min(run, mh[q - 1u + ((q - 1u) >> PS)]) : run;
            uint32_t mid = 0xffffffffu;
            for (uint32_t t = CH; t + 2 <= (uint32_t)w; ++t) mid = min(mid, at(t));
            uint32_t prev = min(suf[0], mid);
            uint32_t diff = j == 0 ? 1u : 0u;
            run = 0xffffffffu;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                run = min(run, at((uint32_t)w - 1u + (uint32_t)i));
                v[i] = min(min(suf[i + 1], mid), run);
                diff |= (v[i] != prev ? 1u : 0u) << i;
                prev = v[i];
            }
            const uint32_t nv = min((uint32_t)CH, nk - j);
            startmask = diff & ((2u << (nv - 1u)) - 1u);
        }
        uint32_t incl = (uint32_t)__popc(startmask);     // (wave_incl_scan of kv_scan_device.h written out: through the helper this kernel did not compile to the same code)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t upv = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += upv;
        }
        const uint32_t nstart = (uint32_t)__shfl((int)incl, 63);
        if (more) wl0[66u * (parity ^ 1u) + lane] = pf;
        for (uint32_t lo = 0; lo < nstart; lo += SKM_WAVE_RUNS) {
            // runs lo .. lo + SKM_WAVE_RUNS (one more than are processed: the end of the last one), listed by the lanes that found them
            {
                uint32_t at = incl - (uint32_t)__popc(startmask) - lo;          // wraps for runs in front of this round: fails the test below
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    if ((startmask >> i) & 1u) {
                        if (at <= SKM_WAVE_RUNS) { starts[at] = (uint16_t)(q + (uint32_t)i); if (at < SKM_WAVE_RUNS) sval[at] = v[i]; }
                        at += 1u;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // P4: a lane per run: its bucket, its records
            const uint32_t here = min(SKM_WAVE_RUNS, nstart - lo);
            for (uint32_t i = lane; i < here; i += 64u) {
                const uint32_t qs = starts[i];
                const uint32_t r = skm_div(qs >> 4, wpr, inv_wpr), j = qs - r * Lp;
                const uint32_t limit = qs - j + nk;                // position one past the read's last k-mer
                const uint32_t nxt = lo + i + 1u < nstart ? (uint32_t)starts[i + 1] : limit;
                uint32_t left = (nxt < limit ? nxt : limit) - qs;
                uint32_t coarse, fine;
                skm_bucket_of(sval[i], sg.C1, sg.fbits, coarse, fine);
                uint64_t pos = (sg.read_base + r0 + r) * sg.stride + j;
                uint32_t b = qs;
                while (left) {
                    const uint32_t n = min(left, (uint32_t)sg.ncap);
                    uint64_t bw[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? skm_bases32(wl, b + 32u * t) : 0ull;
                    const uint32_t rev = sval[i] & 1u;
                    if (rev) skm_rc_bases(bw, sg.nbw, n + (uint32_t)k - 1u);
                    const uint64_t hdr = skm_header(pos, n, fine, rev);
                    const uint32_t p = atomicAdd(&cur[coarse], 1u);
                    if (p < sg.cap1) skm_store_record_wide(my_seg + coarse * cstride + p * (uint32_t)sg.recw, hdr, bw, sg.nbw);
                    else skm_loose_push(sg, hdr, bw);
                    n_rec += 1;
                    left -= n; pos += n; b += n;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        parity ^= 1u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        mt += 1; taken += 1;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < sg.C1; c += THREADS) sg.cnt1[skm_seg1_slot(sg, c, blockIdx.x)] = min(cur[c], sg.cap1);
    n_rec = wave_sum_u64(n_rec);
    if ((threadIdx.x & 63u) == 0 && n_rec) atomicAdd(&sg.ctr[SKM_CTR_RECORDS], (unsigned long long)n_rec);
}

// ---- S1, batches of equal-length reads: a LANE per read (round 5) ---------------------------------------------------
// The wave kernel above deals a group of 7 reads over the lanes three different ways (a lane per packed word, per chunk of k-mer
// starts, per run) with the order values, the run starts and their minimizers passing through LDS between the phases: 57
// lane-instructions per base, a third of the lanes idle in every phase (100 bases are 6.25 words; 7 reads are 49 words and 63 chunks).
// Here a lane takes ONE READ and walks its m-mers in order, all 64 lanes at the same position -- so everything that depends on the
// position alone (which words, which shifts, whether a k-mer ends here) is scalar -- and the window minimum is the streaming form of
// the block decomposition: m-mers in blocks of B = 20; the k-mer whose window ENDS at m-mer p takes min(suffix minimum of the block
// it starts in, [the whole block between, for w = 40,] prefix minimum of the block p is in); a block's values overwrite the suffix
// minima they have just been compared with, and one backward pass turns them into the next block's suffix minima.  Per m-mer:
// two extractions (forward and reverse complement from the block's 64-bit window, constant shifts), a minimum, the order multiply;
// per k-mer: three minima and a compare.  A lane whose minimizer changes appends the run it has just finished -- (minimizer, read,
// first k-mer, length) -- to the wave's list in LDS (ballot + mbcnt; one in thirteen lanes per position), and every few blocks the
// list is turned into records a lane per RUN, all lanes busy: the record code of the kernels above, unchanged, so the records are
// the same records.  No order value, window minimum or run start ever goes through LDS; the words do, once.
// Work is dealt statically (group g to wave g mod waves): a wave has ~19 groups of 64 reads per 7.5 M-read sample, tickets of any
// useful size would leave a tail of a ticket, and the device-wide counter is not in the picture.
// Instances: w = 20 (k = 31: C = 1) and w = 40 (k = 51: C = 2), m = 12, reads of up to 16 x NW bases; everything else takes the kernels above.
#define SKM_LANE_B 20
#define SKM_LANE_CAP 320u         // finished runs a wave lists between two flushes (64 reads x 40 k-mers bring ~250; what does not fit is written at once)
#define SKM_LANE_FLUSH_BLOCKS 2u  // blocks of B m-mers between two flushes of that list (the kernel takes it as an argument: compiled in, the
                                  // cut of 24-byte records measured ~5 us of 1040 slower per launch)
#define SKM_LANE_THREADS 512
#define SKM_LANE_WAVES 6          // waves per SIMD the kernel is compiled for (3 workgroups per CU)
// a wave's slice of LDS: the group's words, their reverse complement read by read (oriented records), the run list
__host__ __device__ inline uint32_t skm_lane_slice_words(uint32_t wpr) { return 2u * (64u * wpr + 4u) + 2u * SKM_LANE_CAP + 2u; }

// one block of B m-mers for every lane's read: Sold holds the suffix minima of the block the finishing k-mers START in (C blocks
// back) and receives this block's values; Smid (C = 2) the suffix minima of the block between, Smid[0] its minimum
template <int C, typename Append>
__device__ __forceinline__ void skm_lane_block(const uint32_t *wl, uint32_t rbase, uint32_t lane, uint32_t b, uint32_t npos, uint32_t nk,
                                               uint32_t (&Sold)[SKM_LANE_B], const uint32_t (&Smid)[SKM_LANE_B], uint32_t &prev_v, uint32_t &start_prev,
                                               uint32_t &n_ent, Append append)
{
    constexpr int B = SKM_LANE_B;
    const uint32_t bit0 = 2u * B * b, w0 = bit0 >> 5, s0 = bit0 & 31u;
    const uint32_t x0 = wl[rbase + w0], x1 = wl[rbase + w0 + 1u], x2 = wl[rbase + w0 + 2u];
    const uint32_t xlo = __builtin_amdgcn_alignbit(x1, x0, s0), xhi = __builtin_amdgcn_alignbit(x2, x1, s0);
    const uint64_t X = (uint64_t)xlo | ((uint64_t)xhi << 32);          // bases 20 b .. 20 b + 31 of the read
    const uint64_t R = ~skm_rev2_64(X);                                // their reverse complement: the m-mer at base j in bits 40 - 2 j .. 63 - 2 j
    uint32_t pre = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        const uint32_t p = (uint32_t)B * b + (uint32_t)j;
        if (p >= npos) break;                                          // (the same for every lane: a scalar branch)
        const uint32_t f = (uint32_t)(X >> (2 * j)) & 0xffffffu, rv = (uint32_t)(R >> (40 - 2 * j)) & 0xffffffu;
        const uint32_t val = skm_order_s(f, rv);
        pre = min(pre, val);
        if (p + 1u >= (uint32_t)(C * B)) {
            const uint32_t i = p + 1u - (uint32_t)(C * B);             // the k-mer whose window ends at this m-mer
            if (i < nk) {
                uint32_t minv;
                if (C == 1) minv = j == B - 1 ? pre : min(Sold[j == B - 1 ? 0 : j + 1], pre);
                else minv = j == B - 1 ? min(Smid[0], pre) : min(min(Sold[j == B - 1 ? 0 : j + 1], Smid[0]), pre);
                if (i == 0u) {
                    prev_v = minv; start_prev = lane;                 // lane | first k-mer << 6: the upper word of the run's entry, but for its end
                } else {
                    // (a lane that finds the list full keeps its run open and asks again at the next k-mer, after the flush that full
                    // list brings about: the run is then cut a few k-mers late -- k-mers in a bucket other than their minimizer's, which
                    // costs deduplication, never correctness: adds of a k-mer's occurrences compose whichever buckets they met in)
                    // (lanes without a read walk words of zeros: one minimizer from end to end, no run ever finishes)
                    const bool want = minv != prev_v;
                    const unsigned long long bal = __ballot(want);
                    if (want && append(bal, prev_v, start_prev, i)) { prev_v = minv; start_prev = lane | (i << 6); }
                    n_ent += (uint32_t)__popcll(bal);
                }
            }
        }
        Sold[j] = val;
    }
#pragma unroll
    for (int j = B - 2; j >= 0; --j) Sold[j] = min(Sold[j], Sold[j + 1]);
}

// (C = 2 keeps two arrays of suffix minima: 4 waves per SIMD -- two workgroups per CU, 128 registers -- where C = 1 runs 6; the kernel
// is bound by instruction issue from 4 waves per SIMD up, so the lower occupancy costs nothing: measured with 512 writers at C = 1)
template <int C, int NW>
__global__ __launch_bounds__(SKM_LANE_THREADS, C == 2 ? 4 : SKM_LANE_WAVES) void k_skm_emit_lane(ReadsDev rd, SkmGeom sg, uint32_t n_groups, uint32_t flush_blocks)
{
    constexpr int B = SKM_LANE_B;
    __shared__ uint32_t cur[256];
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nwaves = SKM_LANE_THREADS / 64;
    const uint32_t L = rd.uni_len, wpr = (L + 15u) >> 4, nk = L - (uint32_t)sg.k + 1u, npos = L - 12u + 1u;
    uint32_t *wl = smem + wave * skm_lane_slice_words(wpr);
    uint32_t *rcl = wl + 64u * wpr + 4u;             // read r's reverse complement: base i of it = complement of the read's base L - 1 - i
    unsigned long long *ent = (unsigned long long *)(rcl + 64u * wpr + 4u);
    for (uint32_t c = threadIdx.x; c < sg.C1; c += SKM_LANE_THREADS) cur[c] = 0;
    __syncthreads();
    uint64_t n_rec = 0;
    uint64_t *const my_seg = sg.seg1 + skm_seg1_slot(sg, 0u, blockIdx.x) * sg.cap1 * (uint64_t)sg.recw;       // + coarse * cstride: this workgroup's segment of a coarse bucket
    const uint64_t cstride = (sg.seg1_wmajor ? 1ull : (uint64_t)sg.nwg1) * sg.cap1 * (uint64_t)sg.recw;
    const uint64_t n_words = rd.n_reads * (uint64_t)wpr;
    const uint32_t nblocks = (npos + B - 1u) / B;
    const uint32_t gstep = gridDim.x * nwaves;
    // words of group g as the wave loads them: word t = lane + 64 i of the group's 64 x wpr
    // (lanes and words beyond the batch's end read as zeros)
    auto fetch = [&](uint32_t g, uint32_t (&dst)[NW]) {
        const uint64_t first = (uint64_t)g * 64u * wpr;
        const uint32_t *gw = rd.words + first;
        const uint32_t have = (uint32_t)min((uint64_t)64u * wpr, n_words - first);
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));              // (or the 64-bit addresses of all NW words are computed once in front of the loop, and spilled)
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t t = ln + 64u * (uint32_t)i;
            dst[i] = t < have ? gw[t] : 0u;
        }
    };
    uint32_t pf[NW];
    uint32_t g = blockIdx.x * nwaves + wave;
    if (g < n_groups) fetch(g, pf);
    for (; g < n_groups; g += gstep) {
        const uint64_t r0 = (uint64_t)g * 64u;
        const uint32_t nr = (uint32_t)min((uint64_t)64u, rd.n_reads - r0);
        const bool active = lane < nr;
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if ((uint32_t)i < wpr) wl[lane + 64u * (uint32_t)i] = pf[i];
        if (lane < 4u) { wl[64u * wpr + lane] = 0u; rcl[64u * wpr + lane] = 0u; }
        // the next group's words are requested now; they are waited for in front of the first flush (below), not at the top of the
        // next round, where the wait would also cover this round's record stores
        const bool more = g + gstep < n_groups;
        if (more) fetch(g + gstep, pf);
        bool pf_waited = !more;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            // every lane reverses and complements its own read once: the 16 wpr base slots of its words turned round (word order and
            // the bases inside each word), complemented, and the 16 wpr - L slots of padding that came to the front shifted out.  A
            // reversed run's bases are then read from this image exactly as a forward run's are read from the words.
            const uint32_t sh = 2u * (16u * wpr - L);                  // < 32
            uint32_t prev = ~skm_rev2_32(wl[lane * wpr + wpr - 1u]);
            for (uint32_t t = 0; t < wpr; ++t) {
                const uint32_t next = t + 1u < wpr ? ~skm_rev2_32(wl[lane * wpr + wpr - 2u - t]) : 0u;
                rcl[lane * wpr + t] = __builtin_amdgcn_alignbit(next, prev, sh);
                prev = next;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        // a finished run as records (a run of more than ncap k-mers is cut)
        auto emit_run = [&](uint32_t v, uint32_t r, uint32_t j, uint32_t left) {
            uint32_t coarse, fine;
            skm_bucket_of(v, sg.C1, sg.fbits, coarse, fine);
            uint64_t pos = (sg.read_base + r0 + r) * sg.stride + j;
            const uint32_t rev = v & 1u;
            const uint32_t *src = rev ? rcl : wl;
            uint32_t bidx = r * wpr * 16u + j;                        // the piece's first base in the read (in wl)
            while (left) {
                const uint32_t n = min(left, (uint32_t)sg.ncap);
                // (a reversed piece: its n + k - 1 bases end at base L - j' of the reverse complement, j' its first base in the read)
                const uint32_t from = rev ? 2u * r * wpr * 16u + L - bidx - (n + (uint32_t)sg.k - 1u) : bidx;
                uint64_t bw[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? skm_bases32(src, from + 32u * t) : 0ull;
                const uint64_t hdr = skm_header(pos, n, fine, rev);
                const uint32_t p = atomicAdd(&cur[coarse], 1u);
                if (p < sg.cap1) {
                    if (sg.compact) {                                 // one aligned 16-byte store: bases, n and the fine bucket (no position)
                        typedef uint64_t u64x2a __attribute__((ext_vector_type(2), aligned(16)));
                        *(u64x2a *)(my_seg + coarse * cstride + p * 2u) = u64x2a{bw[0], skm_c_pack1(bw[1], n, fine, rev)};
                    } else {
                        skm_store_record_wide(my_seg + coarse * cstride + p * (uint32_t)sg.recw, hdr, bw, sg.nbw);
                    }
                }
                else skm_loose_push(sg, hdr, bw);
                n_rec += 1;
                left -= n; pos += n; bidx += n;
            }
        };
        uint32_t n_ent = 0;
        // an entry: the run's minimizer | (lane | first k-mer << 6 | the k-mer behind its last << 18) << 32
        auto append = [&](unsigned long long bal, uint32_t v, uint32_t lane_start, uint32_t end) -> bool {
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, n_ent));
            if (slot >= SKM_LANE_CAP) return false;                   // (a wave of reads that change minimizer at nearly every k-mer)
            ent[slot] = (unsigned long long)v | ((unsigned long long)(lane_start | (end << 18)) << 32);
            return true;
        };
        auto flush = [&]() {
            if (!pf_waited) {
#pragma unroll
                for (int i = 0; i < NW; ++i) asm volatile("" : "+v"(pf[i]));          // the prefetched words have arrived from here on
                pf_waited = true;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t n = min(n_ent, SKM_LANE_CAP);
            for (uint32_t e = lane; e < n; e += 64u) {
                const unsigned long long en = ent[e];
                const uint32_t hi = (uint32_t)(en >> 32), first = (hi >> 6) & 4095u;
                emit_run((uint32_t)en, hi & 63u, first, (hi >> 18) - first);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            n_ent = 0;
        };
        uint32_t Sa[B], Sb[B];
#pragma unroll
        for (int j = 0; j < B; ++j) { Sa[j] = 0xffffffffu; Sb[j] = 0xffffffffu; }
        uint32_t prev_v = 0, start_prev = 0;
        const uint32_t rbase = lane * wpr;
        uint32_t since = 0;
        for (uint32_t b = 0; b < nblocks; b += (C == 2 ? 2u : 1u)) {
            skm_lane_block<C>(wl, rbase, lane, b, npos, nk, Sa, Sb, prev_v, start_prev, n_ent, append);
            if (C == 2 && b + 1u < nblocks) skm_lane_block<C>(wl, rbase, lane, b + 1u, npos, nk, Sb, Sa, prev_v, start_prev, n_ent, append);
            since += (C == 2 ? 2u : 1u);
            // (the last block's runs leave with the final ones; a list that is filling up is flushed whatever the count says)
            if ((since >= flush_blocks || n_ent + 192u > SKM_LANE_CAP) && n_ent && b + (C == 2 ? 2u : 1u) < nblocks) { flush(); since = 0; }
        }
        // the run every read ends in (room for all 64: the list is emptied first if need be)
        if (n_ent + 64u > SKM_LANE_CAP) flush();
        {
            const unsigned long long bal = __ballot(active);
            if (active) (void)append(bal, prev_v, start_prev, nk);
            n_ent += (uint32_t)__popcll(bal);
        }
        flush();
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < sg.C1; c += SKM_LANE_THREADS) sg.cnt1[skm_seg1_slot(sg, c, blockIdx.x)] = min(cur[c], sg.cap1);
    n_rec = wave_sum_u64(n_rec);
    if ((threadIdx.x & 63u) == 0 && n_rec) atomicAdd(&sg.ctr[SKM_CTR_RECORDS], (unsigned long long)n_rec);
}

// ---- S2 ------------------------------------------------------------------------------------------------
#define SKM_THREADS2 512
#define SKM_MAX_F2 4096u          // fine buckets per coarse bucket (12 bits of a k-mer's bucket id in S1; 16 in a record header)
// COMPACT: 16-byte records (kv_skm_device.h: the fine bucket sits in the second word; one 16-byte load and store each)
template <bool COMPACT>
__global__ __launch_bounds__(SKM_THREADS2) void k_skm_split(SkmGeom sg)
{
    __shared__ uint32_t cur[SKM_MAX_F2];
    __shared__ uint32_t spre[769];                    // record prefix over the coarse segments this workgroup drains
    const uint32_t c = blockIdx.y;
    for (uint32_t f = threadIdx.x; f < sg.F2; f += SKM_THREADS2) cur[f] = 0;
    // segments seg = blockIdx.x, blockIdx.x + nwg2, ...: their records are enumerated flat, so every thread has work
    const uint32_t nmine = (skm_seg1_count(sg) - blockIdx.x + sg.nwg2 - 1) / sg.nwg2;       // <= 768
    for (uint32_t i = threadIdx.x; i < nmine; i += SKM_THREADS2) spre[i + 1] = sg.cnt1[skm_seg1_slot(sg, c, blockIdx.x + i * sg.nwg2)];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t i = 0; i < nmine; ++i) { const uint32_t n = spre[i + 1]; spre[i] = acc; acc += n; }
        spre[nmine] = acc;
    }
    __syncthreads();
    const uint32_t total = spre[nmine];
    const int recw = COMPACT ? 2 : sg.recw;
    for (uint32_t i = threadIdx.x; i < total; i += SKM_THREADS2) {
        const uint32_t si = skm_search(spre, nmine, i);
        const uint32_t seg = blockIdx.x + si * sg.nwg2;
        const uint64_t *rec = sg.seg1 + (skm_seg1_first(sg, skm_seg1_slot(sg, c, seg)) + (i - spre[si])) * (uint64_t)recw;
        if (COMPACT) {
            typedef uint64_t u64x2a __attribute__((ext_vector_type(2), aligned(16)));
            const u64x2a both = *(const u64x2a *)rec;
            const uint32_t fine = skm_c_fine(both.y);
            const uint32_t p = atomicAdd(&cur[fine], 1u);
            if (p < sg.cap2) {
                *(u64x2a *)(sg.seg2 + ((((uint64_t)c * sg.F2 + fine) * sg.nwg2 + blockIdx.x) * sg.cap2 + p) * 2ull) = both;
            } else {                                         // (leaves in the loose list's classic form, position unknown)
                uint64_t lw[3] = {both.x, skm_c_b1(both.y), 0ull};
                skm_loose_push(sg, skm_header(0ull, skm_c_n(both.y), fine, skm_c_rev(both.y)), lw);
            }
            continue;
        }
        const uint64_t hdr = rec[0];
        uint64_t bw[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? rec[1 + t] : 0ull;
        const uint32_t fine = skm_hdr_fine(hdr);
        const uint32_t p = atomicAdd(&cur[fine], 1u);
        if (p < sg.cap2)
            skm_store_record(sg.seg2 + ((((uint64_t)c * sg.F2 + fine) * sg.nwg2 + blockIdx.x) * sg.cap2 + p) * (uint64_t)recw, hdr, bw, sg.nbw);
        else skm_loose_push(sg, hdr, bw);
    }
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < sg.F2; f += SKM_THREADS2)
        sg.cnt2[((uint64_t)c * sg.F2 + f) * sg.nwg2 + blockIdx.x] = min(cur[f], sg.cap2);
}

// S2 with the scatter sorted in LDS first.  The plain kernel above stores every record where it falls: 64 lanes, 64
// different cache lines per store instruction, 8-byte pieces of 24-byte records that straddle 32-byte sectors -- PMC:
// 2.5 GB written for 1.36 GB of records, 68 % of the wave cycles stalled on the memory pipe.  Here a workgroup takes
// a chunk of records at a time, ranks them by fine bucket (LDS atomics: rank inside the chunk's share of the bucket),
// lays them out bucket by bucket in LDS and copies that image out with consecutive lanes on consecutive words: a bucket's
// records of one chunk leave as one contiguous run.  Used while a chunk holds at least 2 records per bucket.
//
// What the kernel's time follows is the LENGTH of those runs, not how many waves wait side by side: measured at config 2
// (F2 = 256, 16-byte records, per launch), chunks of 2048 records at two workgroups per CU 0.65 ms, the same chunks at three
// per CU (80 registers) 0.72, at four 0.66; chunks of 4096 at two per CU 0.57, at one 0.73.  So the chunk is as large as
// two workgroups' images fit a CU's 160 KB of LDS -- 64 KB for 16- and 32-byte records, 60 KB for 24-byte ones -- with the
// counters behind the image sized by the fine buckets of THIS launch (12 bytes each; 12 KB at the most), and the kernel is
// compiled for the four waves per SIMD that two workgroups are (128 registers: eight records a thread in flight twice over).
#define SKM_S2_MAXF 1024u                                                 // the most fine buckets the sorted kernel takes (two a thread in its scan)
constexpr uint32_t skm_s2_chunk(int recw) { return recw == 2 ? 4096u : recw == 3 ? 2560u : 2048u; }    // records per chunk
constexpr bool skm_s2_sorted_fits(int recw, uint32_t F2) { return F2 <= SKM_S2_MAXF && 2u * F2 <= skm_s2_chunk(recw); }
// dynamic LDS of a launch: the image, then cur / hist / off of F2 counters each
constexpr size_t skm_s2_lds(int recw, uint32_t F2) { return (size_t)skm_s2_chunk(recw) * recw * 8 + 3 * (size_t)F2 * 4; }
template <int RECW>
__global__ __launch_bounds__(SKM_THREADS2, 4) void k_skm_split_sorted(SkmGeom sg)
{
    constexpr uint32_t CHUNK = skm_s2_chunk(RECW);
    __shared__ uint32_t spre[769];
    __shared__ uint32_t wsum[SKM_THREADS2 / 64];
    extern __shared__ __attribute__((aligned(16))) uint64_t img[];     // [CHUNK][RECW], then the three counter arrays
    const uint32_t c = blockIdx.y, F2 = sg.F2;
    uint32_t *const cur = (uint32_t *)(img + CHUNK * RECW);           // records this workgroup has stored per fine bucket
    uint32_t *const hist = cur + F2;                                  // the chunk's records per bucket, then slot of sorted position 0 minus that position
    uint32_t *const off = hist + F2;                                  // sorted position of the bucket's first record of the chunk
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t f = threadIdx.x; f < F2; f += SKM_THREADS2) { cur[f] = 0; hist[f] = 0; }
    const uint32_t nmine = (skm_seg1_count(sg) - blockIdx.x + sg.nwg2 - 1) / sg.nwg2;       // <= 768
    for (uint32_t i = threadIdx.x; i < nmine; i += SKM_THREADS2) spre[i + 1] = sg.cnt1[skm_seg1_slot(sg, c, blockIdx.x + i * sg.nwg2)];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t i = 0; i < nmine; ++i) { const uint32_t n = spre[i + 1]; spre[i] = acc; acc += n; }
        spre[nmine] = acc;
    }
    __syncthreads();
    const uint32_t total = spre[nmine];
    constexpr uint32_t PER = CHUNK / SKM_THREADS2;                    // records per thread and chunk
    const uint32_t fper = (F2 + SKM_THREADS2 - 1) / SKM_THREADS2;     // buckets per thread in the scan (1 or 2)
    uint64_t *const out = sg.seg2 + ((uint64_t)c * F2 * sg.nwg2 + blockIdx.x) * sg.cap2 * RECW;      // + fine * nwg2 * cap2 * RECW
    const uint64_t fstride = (uint64_t)sg.nwg2 * sg.cap2 * RECW;
    // the records of the NEXT chunk are requested before this chunk is ranked, laid out and stored: a workgroup's chunk used to begin
    // with a round trip to HBM that nothing covered
    uint64_t nh[PER], n0[PER], n1[PER], n2[PER];
    // A thread's records come in rising order, SKM_THREADS2 apart, through this chunk and the next: the segment of each is found by
    // walking spre forward from the segment of the one before (a segment holds a few hundred records: a step or two), not by a
    // binary search of eight dependent LDS reads in front of every load.  All the walks of a thread together make <= nmine steps.
    uint32_t si = 0;
    auto request = [&](uint32_t c0) {
        const uint32_t n = c0 < total ? min(CHUNK, total - c0) : 0u;
#pragma unroll
        for (uint32_t r = 0; r < PER; ++r) {
            const uint32_t i = r * SKM_THREADS2 + threadIdx.x;
            nh[r] = 0; n0[r] = 0; n1[r] = 0; n2[r] = 0;
            if (i < n) {
                const uint32_t gi = c0 + i;
                while (spre[si + 1] <= gi) ++si;                      // (gi < total = spre[nmine]: the walk ends at nmine - 1 at the latest)
                const uint32_t seg = blockIdx.x + si * sg.nwg2;
                const uint64_t *rec = sg.seg1 + (skm_seg1_first(sg, skm_seg1_slot(sg, c, seg)) + (gi - spre[si])) * (uint64_t)RECW;
                if (RECW == 2) {                                      // compact: the word that says the bucket is the second one
                    typedef uint64_t u64x2a __attribute__((ext_vector_type(2), aligned(16)));
                    const u64x2a both = *(const u64x2a *)rec;
                    n0[r] = both.x; nh[r] = both.y;
                } else {
                    nh[r] = rec[0]; n0[r] = rec[1]; n1[r] = rec[2];
                    if (RECW == 4) n2[r] = rec[3];
                }
            }
        }
    };
    request(0);
    for (uint32_t c0 = 0; c0 < total; c0 += CHUNK) {
        const uint32_t n = min(CHUNK, total - c0);
        uint64_t hdr[PER], w0[PER], w1[PER], w2[PER];
        uint32_t rank[PER];
#pragma unroll
        for (uint32_t r = 0; r < PER; ++r) { hdr[r] = nh[r]; w0[r] = n0[r]; w1[r] = n1[r]; w2[r] = n2[r]; rank[r] = 0; }
        request(c0 + CHUNK);
#pragma unroll
        for (uint32_t r = 0; r < PER; ++r)
            if (r * SKM_THREADS2 + threadIdx.x < n) rank[r] = atomicAdd(&hist[RECW == 2 ? skm_c_fine(hdr[r]) : skm_hdr_fine(hdr[r])], 1u);
        __syncthreads();
        // exclusive scan of the chunk's histogram; the bucket's run then starts at slot cur[f] of the private segment
        {
            uint32_t h[2] = {0, 0}, sum = 0;
            for (uint32_t j = 0; j < fper; ++j) {
                const uint32_t f = threadIdx.x * fper + j;
                h[j] = f < F2 ? hist[f] : 0u;
                sum += h[j];
            }
            uint32_t incl = sum;                        // (wave_incl_scan of kv_scan_device.h written out: through the helper this kernel did not compile to the same code)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if (lane >= (uint32_t)d) incl += up;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t before = incl - sum;
            for (uint32_t wv = 0; wv < wave; ++wv) before += wsum[wv];
            for (uint32_t j = 0; j < fper; ++j) {
                const uint32_t f = threadIdx.x * fper + j;
                if (f < F2) {
                    off[f] = before;
                    const uint32_t at = cur[f];
                    cur[f] = at + h[j];
                    hist[f] = at - before;              // slot = sorted position + this (mod 2^32)
                    before += h[j];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < PER; ++r) {
            if (r * SKM_THREADS2 + threadIdx.x < n) {
                uint64_t *dst = img + (off[RECW == 2 ? skm_c_fine(hdr[r]) : skm_hdr_fine(hdr[r])] + rank[r]) * (uint32_t)RECW;
                if (RECW == 2) { dst[0] = w0[r]; dst[1] = hdr[r]; }
                else { dst[0] = hdr[r]; dst[1] = w0[r]; dst[2] = w1[r]; }
                if (RECW == 4) dst[3] = w2[r];
            }
        }
        __syncthreads();
        for (uint32_t wd = threadIdx.x; wd < n * RECW; wd += SKM_THREADS2) {
            const uint32_t q = wd / RECW, part = wd - q * RECW;
            const uint64_t h0 = img[q * RECW + (RECW == 2 ? 1 : 0)];
            const uint32_t f = RECW == 2 ? skm_c_fine(h0) : skm_hdr_fine(h0);
            const uint32_t slot = q + hist[f];
            if (slot < sg.cap2) out[(uint64_t)f * fstride + (slot * (uint32_t)RECW + part)] = img[wd];
            else if (part == 0) {
                if (RECW == 2) {                                      // a compact record leaves in the loose list's (classic) form, position unknown
                    uint64_t bw[3] = {img[q * RECW], skm_c_b1(h0), 0ull};
                    skm_loose_push(sg, skm_header(0ull, skm_c_n(h0), f, skm_c_rev(h0)), bw);
                } else {
                    uint64_t bw[3] = {img[q * RECW + 1], img[q * RECW + 2], RECW == 4 ? img[q * RECW + 3] : 0ull};
                    skm_loose_push(sg, h0, bw);
                }
            }
        }
        __syncthreads();
        for (uint32_t f = threadIdx.x; f < F2; f += SKM_THREADS2) hist[f] = 0;
        // (the next chunk's atomics on hist come after its loads and after the barrier below at the latest: the loop's
        // first barrier orders them behind this reset only if every thread passes it, so reset before a barrier)
        __syncthreads();
    }
    for (uint32_t f = threadIdx.x; f < F2; f += SKM_THREADS2)
        sg.cnt2[((uint64_t)c * F2 + f) * sg.nwg2 + blockIdx.x] = min(cur[f], sg.cap2);
}

}  // namespace
