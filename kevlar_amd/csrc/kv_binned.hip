// kv_binned.hip -- K2 count for large batches: no global atomics on the tables.
//
// The straightforward kernel (k_consume) performs T saturating read-modify-writes per k-mer at
// random table positions.  Measured on MI355X each one moves a 64-B sector in and out of HBM
// (269 GB per 525 M k-mers, profiles/r1_naive) and the device tops out at ~27 G atomics/s.
// Counting is a histogram, so this file computes it the way large GPU histograms are done:
//
//   A  k_bin_hash_direct  hash every k-mer once (same LDS-staged tiles as k_consume), band/mask filter,
//                   and for each of the T tables append the bin to one of C coarse buckets
//                   (bin range = F slices of 65536 bins).  Every workgroup owns a private segment
//                   of every bucket; its write cursor lives in LDS and the item is stored straight
//                   to HBM (L2 merges the partial lines): no global atomic, no barrier.
//                   (k_bin_list takes hashes from a list instead of reads.)
//   B  k_bin_split  each coarse bucket is split into its F slices; items shrink to the 16-bit
//                   offset inside the slice.  The fan-out is too wide for direct stores here, so
//                   items collect in per-workgroup LDS rings and leave as coalesced bursts.
//   C  k_bin_apply  one workgroup per (table, slice): the slice's 64 KB of counters is loaded
//                   into LDS, every item is applied with an LDS compare-and-swap (saturating at
//                   255 / 15 / 1), and the slice is written back once.  Table 0 also yields the
//                   exact change of n_occupied.
//
// HBM traffic per k-mer: ~T*(4+4+2+2) B of items + one read and one write of the tables,
// against T*128 B for the atomic kernel.  The result is bit-identical (saturating adds commute).
//
// Skewed inputs (one k-mer repeated millions of times) cannot break it: a bucket that fills
// up diverts further items to a spill list that is applied with global atomics after stage C;
// if even that overflows, the launcher reports it and kv_consume falls back to k_consume.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "kv_binned.h"
#include "kv_device.h"
#include "kv_kmer2bit_device.h"

namespace {

#define BIN_B_ITEMS 8       // items per thread per round in stage B (the planner's constants: kv_bin_plan.h)

// ---- LDS write-combining rings ------------------------------------------------------------
// ns streams, each a ring of R items (R a power of two) plus an append counter and a flushed
// counter.  Appends are LDS atomics; after a workgroup barrier every wave flushes the streams it
// owns: the owning lane decides, one global atomic claims the space, then the whole wave copies
// the burst (coalesced).  A stream that receives more than R items between two flushes diverts
// the excess to the caller's overflow path, so skew costs speed, never correctness.
template <typename ItemT>
struct Rings {
    ItemT *ring;
    uint32_t *cnt, *base;
    uint32_t R;
    uint32_t skew;      // item p of stream s sits in slot (p + skew * s) & (R - 1): streams fill in step, so unskewed
                        // slots would share LDS banks; stage B uses 8 so that 8-item vectors stay aligned
};

template <typename ItemT>
__device__ __forceinline__ bool ring_append(const Rings<ItemT> &rs, uint32_t s, ItemT item)
{
    const uint32_t pos = atomicAdd(&rs.cnt[s], 1u);
    if (pos - rs.base[s] >= rs.R) return false;
    rs.ring[s * rs.R + ((pos + rs.skew * s) & (rs.R - 1))] = item;
    return true;
}

// `written` is the owning lane's count of items already flushed for ITS stream (one stream per
// lane: callers guarantee ns <= 64 * waves), i.e. the position inside the private segment whose
// first element index the same lane holds in `seg_base`.  Bursts are copied two at a time, one per
// half-wave (a burst is 32-48 items, so a whole wave per burst would idle half its lanes), and all
// per-burst parameters travel by v_readlane: the flush phase is instruction-bound, not bandwidth-bound.
template <typename ItemT, typename Store, typename Overflow>
__device__ __forceinline__ void rings_flush(const Rings<ItemT> &rs, uint32_t ns, bool final, uint32_t &written,
                                            uint64_t seg_base, uint32_t cap, Store store, Overflow overflow, uint32_t quantum = 32u)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const uint32_t per_wave = (ns + nwaves - 1) / nwaves;             // <= 64
    const uint32_t s0 = wave * per_wave, s_end = min(ns, s0 + per_wave);
    const uint32_t s = s0 + lane;
    uint32_t n = 0, base = 0, pos = 0;
    if (s < s_end) {
        base = rs.base[s];
        const uint32_t avail = rs.cnt[s] - base;
        uint32_t newbase = base;
        if (avail > rs.R) { n = rs.R; newbase = base + avail; }   // overran: the excess was diverted at append time
        else if (final) { n = avail; newbase = base + n; }
        else if (avail >= rs.R / 2) { n = avail & ~(quantum - 1u); newbase = base + n; }   // whole half-wave bursts: one copy iteration, all lanes busy
        if (n) { pos = written; written += n; rs.base[s] = newbase; }
    }
    const uint32_t seg_lo = (uint32_t)seg_base, seg_hi = (uint32_t)(seg_base >> 32);
    const bool upper = lane >= 32;
    const uint32_t sub = lane & 31u;
    unsigned long long todo = __ballot(n > 0);
    while (todo) {
        const int l0 = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int l1 = todo ? __ffsll((long long)todo) - 1 : l0;
        const bool two = todo != 0;
        if (two) todo &= todo - 1;
        // wave-uniform lane indices: v_readlane, not an LDS permute
        const uint32_t n0 = __builtin_amdgcn_readlane(n, l0), n1 = two ? __builtin_amdgcn_readlane(n, l1) : 0u;
        const uint32_t b0 = __builtin_amdgcn_readlane(base, l0), b1 = __builtin_amdgcn_readlane(base, l1);
        const uint32_t p0 = __builtin_amdgcn_readlane(pos, l0), p1 = __builtin_amdgcn_readlane(pos, l1);
        const uint32_t g0l = __builtin_amdgcn_readlane(seg_lo, l0), g1l = __builtin_amdgcn_readlane(seg_lo, l1);
        const uint32_t g0h = __builtin_amdgcn_readlane(seg_hi, l0), g1h = __builtin_amdgcn_readlane(seg_hi, l1);
        const uint32_t sl = s0 + (uint32_t)(upper ? l1 : l0);
        const uint32_t nl = upper ? n1 : n0, bl = upper ? b1 : b0, pl = upper ? p1 : p0;
        const uint64_t gl = ((uint64_t)(upper ? g1h : g0h) << 32) | (upper ? g1l : g0l);
        for (uint32_t j = sub; j < nl; j += 32) {
            const ItemT item = rs.ring[sl * rs.R + ((bl + j + rs.skew * sl) & (rs.R - 1))];
            if (pl + j < cap) store(gl + pl + j, item);
            else overflow(sl, item);
        }
    }
}

// Stage B's flush between rounds: the flush phase of rings_flush is instruction-bound (PMC: ~600 VALU
// wave-instructions per wave and round, 4/5 of them broadcasting per-burst parameters and looping), and a lane
// that copies its own burst writes every 64-byte sector with four store instructions, each of which touches as
// many lines as it has lanes.  So every lane that owns a ready stream only DECIDES (items, ring slot, place in
// the segment) and enters its lane number in the wave's list in LDS (ballot + mbcnt); then the wave serves the list
// sixteen streams a pass, four adjacent lanes a stream: lane l fetches the burst of the owner list[l >> 2] with two
// shuffles and copies quarter l & 3 of each of its sectors, one 16-byte LDS read and one 16-byte global store,
// so that a sector leaves whole, in one instruction.  Bursts are multiples of 32 items and the ring skew is 8,
// so vectors stay 16-byte aligned in LDS and in the segment (u16 and u32 items alike).  The rare misfits (segment
// nearly full, ring overrun that left the base unaligned) are left to rings_flush.
// stream_base, stream_stride: stream s' segment starts at item stream_base + s * stream_stride; ready: 64 bytes per wave.
template <typename ItemT, typename Overflow>
__device__ __forceinline__ void rings_flush_quads(const Rings<ItemT> &rs, uint32_t ns, uint32_t &written, uint64_t seg_base,
                                                  uint64_t stream_base, uint64_t stream_stride, uint32_t cap, ItemT *gbuf,
                                                  uint8_t *ready, Overflow overflow)
{
    constexpr uint32_t VEC = 16u / sizeof(ItemT);        // items per 16-byte vector
    constexpr uint32_t QUANTUM = 64u / sizeof(ItemT);    // bursts are whole 64-byte sectors
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const uint32_t per_wave = (ns + nwaves - 1) / nwaves;
    const uint32_t s0 = wave * per_wave, s_end = min(ns, s0 + per_wave);
    const uint32_t s = s0 + lane;
    bool misfit = false;
    uint32_t burst = 0, pos = 0;      // burst: first ring slot | items << 16 (both at most R <= BIN_RING_MAX); pos: its place in the segment
    if (s < s_end) {
        const uint32_t base = rs.base[s];
        const uint32_t avail = rs.cnt[s] - base;
        uint32_t n = 0, newbase = base;
        if (avail > rs.R) { n = rs.R; newbase = base + avail; }
        else if (avail >= rs.R / 2) { n = avail & ~(QUANTUM - 1u); newbase = base + n; }
        if (n) {
            if ((base & 7u) || written + n > cap || (newbase & 7u)) misfit = true;
            else {
                burst = ((base + rs.skew * s) & (rs.R - 1)) | n << 16;
                pos = written;
                written += n;
                rs.base[s] = newbase;
            }
        }
    }
    const unsigned long long todo = __ballot(burst != 0);
    if (todo) {
        uint8_t *list = ready + wave * 64u;
        if (burst) list[__builtin_amdgcn_mbcnt_hi((uint32_t)(todo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)todo, 0u))] = (uint8_t)lane;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t nready = (uint32_t)__popcll(todo);
        const uint32_t quarter = (lane & 3u) * VEC;
        for (uint32_t q0 = 0; q0 < nready; q0 += 16) {          // wave-uniform: the shuffles need every owner lane active
            const uint32_t q = q0 + (lane >> 2);
            const uint32_t owner = list[min(q, nready - 1u)];
            const uint32_t b = (uint32_t)__shfl((int)burst, (int)owner), p = (uint32_t)__shfl((int)pos, (int)owner);
            if (q < nready) {
                const uint32_t r = s0 + owner, n = b >> 16, slot = b & 0xffffu;
                const ItemT *ring = rs.ring + r * rs.R;
                ItemT *dst = gbuf + stream_base + (uint64_t)r * stream_stride + p;
                for (uint32_t v = quarter; v < n; v += QUANTUM)
                    *(uint4 *)(dst + v) = *(const uint4 *)(ring + ((slot + v) & (rs.R - 1)));
            }
        }
    }
    if (__ballot(misfit)) {
        auto store = [&](uint64_t idx, ItemT off) { gbuf[idx] = off; };
        rings_flush(rs, ns, false, written, seg_base, cap, store, overflow, QUANTUM);
    }
}

__device__ __forceinline__ void rings_store_counts(uint32_t ns, uint32_t written, uint32_t cap, uint32_t *counts, uint32_t stride, uint32_t writer)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const uint32_t per_wave = (ns + nwaves - 1) / nwaves;
    const uint32_t s = wave * per_wave + lane;
    if (lane < per_wave && s < ns) counts[(uint64_t)s * stride + writer] = written < cap ? written : cap;
}

// ---- stage A -----------------------------------------------------------------------------
// Every workgroup owns a private segment of every coarse bucket; the segment's write cursor lives in LDS and each item is stored
// straight to HBM -- no barrier, no flush phase between hashing a k-mer and storing its T items.  The write frontier (workgroups x
// buckets x one 128-B line) sits in L2, which merges the partial lines before they reach HBM.  The three kernels share four steps:
template <int THREADS> __device__ __forceinline__ void bin_clear_cursors(const BinGeom &g, uint32_t *cur)
{
    for (uint32_t s = threadIdx.x; s < (uint32_t)(g.T * g.C); s += THREADS) cur[s] = 0;
}

// the workgroup's next unit of work off the device-wide counter (its callers stop at g.quotaA tickets or past the last unit)
template <typename U> __device__ __forceinline__ U bin_ticket(const BinGeom &g, U *next)
{
    __syncthreads();
    if (threadIdx.x == 0) *next = (U)atomicAdd(&g.ctr[4], 1ull);
    __syncthreads();
    return *next;
}

// One hash into its T coarse buckets, in three passes so that the T LDS atomics are in flight together: all T items, all T
// cursor bumps, then the T stores (or the spill list for a segment that is full).  W: the item carries wgt - 1 (kv_bin_plan.h).
template <bool W> __device__ __forceinline__ void bin_route(const BinGeom &g, const SketchDev *sk, uint32_t *cur, uint64_t h, uint32_t wgt)
{
    constexpr uint32_t SB = BIN_SLICE_BITS;
    uint32_t sidx[BIN_MAX_T], item[BIN_MAX_T], pos[BIN_MAX_T];
    uint64_t bins[BIN_MAX_T];
#pragma unroll
    for (int t = 0; t < BIN_MAX_T; ++t) {
        if (t >= g.T) break;
        const uint64_t bin = fastmod(h, sk->size[t], sk->magic[t]);
        const uint32_t slice = (uint32_t)(bin >> SB);
        const uint32_t c = g.F == 1 ? slice : __umulhi(slice, g.recipF);
        bins[t] = bin;
        item[t] = ((slice - c * (uint32_t)g.F) << SB) | ((uint32_t)bin & ((1u << SB) - 1u)) | (W ? (wgt - 1u) << BIN_W_SHIFT : 0u);
        sidx[t] = (uint32_t)t * (uint32_t)g.C + c;
    }
#pragma unroll
    for (int t = 0; t < BIN_MAX_T; ++t)
        if (t < g.T) pos[t] = atomicAdd(&cur[sidx[t]], 1u);
#pragma unroll
    for (int t = 0; t < BIN_MAX_T; ++t) {
        if (t >= g.T) break;
        if (pos[t] < g.cap1) g.gbuf1[((uint64_t)sidx[t] * g.nwgA + blockIdx.x) * g.cap1 + pos[t]] = item[t];
        else spill_item(g, t, bins[t], wgt);
    }
}

// the segments' item counts; ADDED: and the workgroup's share of the k-mers added, one atomic a wave
template <int THREADS, bool ADDED = true> __device__ __forceinline__ void bin_close(const BinGeom &g, const uint32_t *cur, uint64_t n_added)
{
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < (uint32_t)(g.T * g.C); s += THREADS)
        g.gcnt1[(uint64_t)s * g.nwgA + blockIdx.x] = (uint32_t)min((uint64_t)cur[s], g.cap1);
    if (!ADDED) return;
    n_added = wave_sum_u64(n_added);
    if ((threadIdx.x & 63) == 0 && n_added) atomicAdd(&g.ctr[2], (unsigned long long)n_added);
}

template <int THREADS, int NW>
__global__ __launch_bounds__(THREADS, (THREADS == 512 ? 6 : 4)) void k_bin_hash_direct(
    ReadsDev rd, uint32_t n_tiles, const SketchDev *__restrict__ sk, const SketchDev *__restrict__ mask,
    ConsumeFilter f, BinGeom g)
{
    __shared__ TileShared sh;
    __shared__ uint32_t cur[BIN_MAX_T * BIN_C];
    __shared__ uint32_t next_tile;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (threadIdx.x == 0) sh.ascii = (uint32_t *)smem;
    bin_clear_cursors<THREADS>(g, cur);
    uint64_t n_added = 0;
    for (uint32_t taken = 0; taken < g.quotaA; ++taken) {
        const uint32_t tile = bin_ticket(g, &next_tile);
        if (tile >= n_tiles) break;
        uint32_t read0;
        const uint32_t nr = stage_tile(sh, rd, tile, f.hp.k, 0, 0, read0);
        const uint32_t total = sh.kpre[nr];
        const uint32_t run = (total + THREADS - 1) / THREADS;
        const uint32_t q0 = threadIdx.x * run, q1 = min(total, q0 + run);
        KmerRoll<(NW > 0 ? NW : 8)> w;
        if (NW > 0 && q0 < q1) {
            locate_kmer(sh, nr, q0, w.r, w.i);
            roll_load(w, sh, f.hp.k);
        }
        for (uint32_t step = 0; step < run; ++step) {
            const uint32_t q = NW > 0 ? q0 + step : step * THREADS + threadIdx.x;
            const bool live = NW > 0 ? q < q1 : q < total;
            if (!live) continue;
            uint64_t h;
            if (NW > 0) {
                h = roll_hash(w, f.hp);
                if (q + 1 < q1) roll_step(w, sh, nr, f.hp.k);
            } else {
                uint32_t r, i;
                locate_kmer(sh, nr, q, r, i);
                const uint32_t fwd = sh.foff[r] + i;
                const uint32_t rc = sh.roff[r] + (sh.len[r] - (uint32_t)f.hp.k - i);
                h = kmer_hash_lds(sh.ascii, fwd, rc, f.hp);
            }
            if (!consume_filter_pass(f, mask, h)) continue;
            n_added += 1;
            bin_route<false>(g, sk, cur, h, 1u);
        }
    }
    bin_close<THREADS>(g, cur, n_added);
}

// Stage A for batches of equal-length reads, hashed from the 2-bit form (kv_kmer2bit_device.h): a thread takes BIN2_CH consecutive
// k-mers of one read; what passes the band / mask filter is collected per wave and routed 64 at a time -- T reductions, T items through
// the LDS cursors, direct stores, exactly as k_bin_hash_direct stores them.  A ticket is BIN2_TILES tiles' worth of reads.
#define BIN2_CH 10
// FK = 31: the instance for kevlar's default k, with the murmurs' first multiplications from the product tables (skm_key_hash_pl)
template <int THREADS, int KW, int FK = 0>
__global__ __launch_bounds__(THREADS, (THREADS == 512 ? 6 : 4)) void k_bin_hash_2bit(
    ReadsDev rd, uint32_t n_units, const SketchDev *__restrict__ sk, const SketchDev *__restrict__ mask, ConsumeFilter f, BinGeom g)
{
    __shared__ __attribute__((aligned(8))) uint32_t lut[FK ? 1024 : 256];
    __shared__ uint32_t cur[BIN_MAX_T * BIN_C];
    __shared__ uint32_t next_unit;
    __shared__ unsigned long long queue[(THREADS / 64) * 128];
    bin_clear_cursors<THREADS>(g, cur);
    if (threadIdx.x < 256) {
        if (FK) { ((uint64_t *)lut)[threadIdx.x] = skm_ascii4_times(threadIdx.x, MM_C1); ((uint64_t *)lut)[256 + threadIdx.x] = skm_ascii4_times(threadIdx.x, MM_C2); }
        else lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    }
    const int k = FK ? FK : f.hp.k;
    const uint32_t L = rd.uni_len, wpr = (L + 15u) >> 4, nk = L - (uint32_t)k + 1u, cpr = (nk + BIN2_CH - 1u) / BIN2_CH;
    const float inv_cpr = 1.0f / (float)cpr;
    const uint64_t reads_per_unit = (uint64_t)BIN2_TILES * rd.uni_per_tile;
    WaveQueue wq;
    wq.q = queue + (threadIdx.x >> 6) * 128u;
    wq.n = 0;
    uint64_t n_added = 0;
    auto route = [&](bool have, uint64_t h) {
        if (!have) return;
        n_added += 1;
        bin_route<false>(g, sk, cur, h, 1u);
    };
    for (uint32_t taken = 0; taken < g.quotaA; ++taken) {
        const uint32_t unit = bin_ticket(g, &next_unit);
        if (unit >= n_units) break;
        const uint64_t r0 = (uint64_t)unit * reads_per_unit;
        const uint32_t nr = (uint32_t)min(reads_per_unit, rd.n_reads - r0), n_items = nr * cpr;
        // (whole waves go round together: the queue's ballots want every lane there)
        for (uint32_t i0 = (threadIdx.x & ~63u); i0 < n_items; i0 += THREADS) {
            const uint32_t i = i0 + (threadIdx.x & 63u);
            const bool mine = i < n_items;
            const uint32_t r = mine ? k2_div(i, cpr, inv_cpr) : 0u, j0 = mine ? (i - r * cpr) * BIN2_CH : 0u;
            const uint32_t cnt = mine ? min((uint32_t)BIN2_CH, nk - j0) : 0u;
            kmer2bit_walk<KW, BIN2_CH, FK>(rd.words + (r0 + r) * wpr, j0, cnt, k, lut, f.hp, [&](bool live, uint64_t h) {
                wave_queue_push(wq, live && consume_filter_pass(f, mask, h), h, route);
            });
        }
    }
    wave_queue_flush(wq, route);
    bin_close<THREADS>(g, cur, n_added);
}

// stage A over a list of hashes already in HBM (read-sharded multi-GPU count: the hashes of this
// rank's band arrive from the other ranks, kv_shard.hip).  Element i sits at list[i * stride].
// W: the list holds (hash, count) pairs -- element i at list[i * stride], its count at list[i * stride + 1] -- and the
// items carry min(count, 255) as their weight (what a band owner receives from ranks that deduplicated their shards)
template <int THREADS, bool W>
__global__ __launch_bounds__(THREADS, (THREADS == 512 ? 6 : 4)) void k_bin_list(
    const uint64_t *__restrict__ list, uint64_t n, uint32_t stride, const SketchDev *__restrict__ sk, BinGeom g)
{
    // same direct stores through LDS cursors as k_bin_hash_direct; the hashes just come from HBM
    __shared__ uint32_t cur[BIN_MAX_T * BIN_C];
    __shared__ uint64_t next_chunk;
    bin_clear_cursors<THREADS>(g, cur);
    const uint64_t chunk = (uint64_t)THREADS * BIN_LIST_ROUNDS;
    uint64_t n_added = 0;
    for (uint32_t taken = 0; taken < g.quotaA; ++taken) {
        const uint64_t i0 = bin_ticket(g, &next_chunk) * chunk;
        if (i0 >= n) break;
        uint64_t idx = i0 + threadIdx.x;
        uint64_t h_next = idx < n ? list[idx * stride] : 0, c_next = (W && idx < n) ? list[idx * stride + 1] : 1;
        for (int round = 0; round < BIN_LIST_ROUNDS; ++round) {
            const uint64_t h = h_next, count = c_next;
            const bool live = idx < n;
            idx += THREADS;
            if (round + 1 < BIN_LIST_ROUNDS && idx < n) {   // flies while this one is routed
                h_next = list[idx * stride];
                if (W) c_next = list[idx * stride + 1];
            }
            if (!live) continue;
            n_added += count;
            uint32_t left = W ? (uint32_t)min(count, (uint64_t)255) : 1u;
            while (left) {
                const uint32_t wgt = W ? min(left, BIN_W_MAX) : 1u;
                left -= wgt;
                bin_route<W>(g, sk, cur, h, wgt);
            }
        }
    }
    bin_close<THREADS, W>(g, cur, n_added);     // (an unweighted list's length is its caller's n_added)
}

// ---- stage B -----------------------------------------------------------------------------
// W = weighted items (kv_binned.h): a coarse item carries its increment in bits 25..31 and leaves as offset | increment << 16
template <bool W>
__global__ __launch_bounds__(BIN_B_THREADS) void k_bin_split(BinGeom g)
{
    typedef typename std::conditional<W, uint32_t, uint16_t>::type Out;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.y;                  // coarse stream = table * C + bucket
    const uint32_t t = s / (uint32_t)g.C, c = s % (uint32_t)g.C;
    const uint32_t F = (uint32_t)g.F;
    Rings<Out> rs;
    rs.R = g.ringB;
    rs.skew = 8;
    rs.ring = (Out *)smem;
    const BinSplitLds lay = bin_split_lds(F, rs.R, sizeof(Out));
    rs.cnt = (uint32_t *)(smem + lay.cnt); rs.base = (uint32_t *)(smem + lay.base);
    uint8_t *ready = smem + lay.ready;              // BIN_B_THREADS bytes: every wave's list of lanes with a burst to flush
    for (uint32_t i = threadIdx.x; i < F; i += BIN_B_THREADS) { rs.cnt[i] = 0; rs.base[i] = 0; }
    __syncthreads();
    uint32_t written = 0;
    uint64_t seg_base = 0;
    const uint64_t stream_base = ((uint64_t)s * F * g.nwgB + blockIdx.x) * g.cap2, stream_stride = (uint64_t)g.nwgB * g.cap2;
    {
        const uint32_t nwaves = BIN_B_THREADS >> 6, per_wave = (F + nwaves - 1) / nwaves;
        const uint32_t mine = (threadIdx.x >> 6) * per_wave + (threadIdx.x & 63);
        if ((threadIdx.x & 63) < per_wave && mine < F) seg_base = stream_base + mine * stream_stride;
    }
    Out *gbuf2 = (Out *)g.gbuf2;
    constexpr uint32_t SB = BIN_SLICE_BITS, OFFMASK = (1u << SB) - 1u;
    auto slice_of = [](uint32_t item) { return W ? (item >> SB) & ((1u << (BIN_W_SHIFT - SB)) - 1u) : item >> SB; };
    auto fine_of = [](uint32_t item) { return W ? (Out)((item & OFFMASK) | (((item >> BIN_W_SHIFT) + 1u) << 16)) : (Out)(item & OFFMASK); };
    auto spill_coarse = [&](uint32_t item) {
        spill_item(g, (int)t, (((uint64_t)c * F + slice_of(item)) << SB) | (item & OFFMASK), W ? (item >> BIN_W_SHIFT) + 1u : 1u);
    };
    auto store = [&](uint64_t idx, Out off) { gbuf2[idx] = off; };
    auto overflow = [&](uint32_t fi, Out off) {
        spill_item(g, (int)t, (((uint64_t)c * F + fi) << SB) | ((uint32_t)off & OFFMASK), W ? (uint32_t)off >> 16 : 1u);
    };
    // Weighted items are u32: rings of 32 entries (64 would leave room for one workgroup per CU only) and half as many
    // items per round, so that a round cannot overrun a ring that was below its flush threshold
    constexpr int ITEMS = W ? 4 : BIN_B_ITEMS;
    const uint64_t step = (uint64_t)BIN_B_THREADS * ITEMS;
    // this workgroup drains the private segments seg = blockIdx.x, blockIdx.x + nwgB, ... of bucket s
    for (uint32_t seg = blockIdx.x; seg < g.nwgA; seg += g.nwgB) {
        uint64_t end = g.gcnt1[(uint64_t)s * g.nwgA + seg];
        if (end > g.cap1) end = g.cap1;
        const uint32_t *src = g.gbuf1 + ((uint64_t)s * g.nwgA + seg) * g.cap1;
        uint4 va = make_uint4(0, 0, 0, 0), vb = va;
        auto fetch = [&](uint64_t r0, uint4 &a, uint4 &b) {
            const uint64_t i0 = r0 + (uint64_t)threadIdx.x * ITEMS;
            if (i0 + ITEMS <= end) { a = *(const uint4 *)(src + i0); if (ITEMS == 8) b = *(const uint4 *)(src + i0 + 4); }
        };
        fetch(0, va, vb);
        for (uint64_t r0 = 0; r0 < end; r0 += step) {
            const uint64_t i0 = r0 + (uint64_t)threadIdx.x * ITEMS;
            uint32_t items[ITEMS];
            int have = 0;
            if (i0 + ITEMS <= end) {
                items[0] = va.x; items[1] = va.y; items[2] = va.z; items[3] = va.w;
                if (ITEMS == 8) { items[ITEMS - 4] = vb.x; items[ITEMS - 3] = vb.y; items[ITEMS - 2] = vb.z; items[ITEMS - 1] = vb.w; }
                have = ITEMS;
            } else {
                for (uint64_t i = i0; i < end; ++i) items[have++] = src[i];
            }
            if (r0 + step < end) fetch(r0 + step, va, vb);          // next round's items fly during this round
            if (have == ITEMS) {
                // full vector: all ring positions are requested back to back (independent LDS atomics in flight
                // together), then consumed; an item whose ring is full is rare and handled after the fast path
                uint32_t pos[ITEMS], rbase[ITEMS];
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) pos[j] = atomicAdd(&rs.cnt[slice_of(items[j])], 1u);
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) rbase[j] = rs.base[slice_of(items[j])];
                uint32_t full = 0;
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) {
                    const uint32_t fi = slice_of(items[j]);
                    if (pos[j] - rbase[j] < rs.R) rs.ring[fi * rs.R + ((pos[j] + rs.skew * fi) & (rs.R - 1))] = fine_of(items[j]);
                    else full |= 1u << j;
                }
                if (full) {
#pragma unroll
                    for (int j = 0; j < ITEMS; ++j)
                        if (full & (1u << j)) spill_coarse(items[j]);
                }
            } else {
                for (int j = 0; j < have; ++j)
                    if (!ring_append(rs, slice_of(items[j]), fine_of(items[j]))) spill_coarse(items[j]);
            }
            __syncthreads();
            rings_flush_quads(rs, F, written, seg_base, stream_base, stream_stride, (uint32_t)g.cap2, gbuf2, ready, overflow);
            __syncthreads();
        }
    }
    rings_flush(rs, F, true, written, seg_base, (uint32_t)g.cap2, store, overflow, 64u / (uint32_t)sizeof(Out));
    rings_store_counts(F, written, (uint32_t)g.cap2, g.gcnt2 + (uint64_t)s * F * g.nwgB, g.nwgB, blockIdx.x);
}

// ---- stage C -----------------------------------------------------------------------------
// Where bin `off` keeps its counter: the index of its 32-bit word and the counter's shift inside it.  ST_BYTE: a byte per bin;
// ST_NIBBLE: two bins per byte, the even bin in the high nibble.
template <int STORAGE, typename Off> __device__ __forceinline__ void counter_slot(Off off, Off &word, uint32_t &shift)
{
    if (STORAGE == ST_BYTE) { word = off >> 2; shift = ((uint32_t)off & 3u) << 3; }
    else { word = off >> 3; shift = ((((uint32_t)off >> 1) & 3u) << 3) + ((off & 1u) ? 0u : 4u); }
}

// Eight saturating increments with the LDS round trips overlapped: all eight words are read first, then
// all eight compare-and-swaps are issued back to back, and only an item whose word changed in between
// (another lane, or an earlier item of this same vector, hit the same word) takes the retry loop.  Returns
// how many bins went 0 -> 1.  STORAGE is a template parameter and the fast path is branch-free: with a
// run-time switch and a branch per item this loop was instruction-bound (~175 instructions per item).
template <int STORAGE>
__device__ __forceinline__ uint32_t lds_inc8(uint32_t *lds, const uint32_t (&w)[4], uint32_t n)
{
    uint32_t fresh = 0;
    if (STORAGE == ST_BIT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t off = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
            if ((uint32_t)e < n) {
                const uint32_t bit = 1u << (off & 31);
                fresh += (atomicOr(&lds[off >> 5], bit) & bit) == 0 ? 1u : 0u;
            }
        }
        return fresh;
    }
    constexpr uint32_t maxv = STORAGE == ST_BYTE ? 255u : 15u;
    uint32_t widx[8], inc[8], old[8], prev[8];
    uint32_t retry = 0;                                  // bit e: item e lost its CAS
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t off = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
        uint32_t shift;
        counter_slot<STORAGE>(off, widx[e], shift);
        inc[e] = 1u << shift;
    }
    // two groups of four: the window between reading a word and swapping it stays short (fewer lost races)
#pragma unroll
    for (int g4 = 0; g4 < 8; g4 += 4) {
#pragma unroll
        for (int e = g4; e < g4 + 4; ++e) old[e] = lds[widx[e]];          // absent items (e >= n) read a harmless word
        bool live[4];
#pragma unroll
        for (int e = g4; e < g4 + 4; ++e) {
            // a saturated counter (field == inc * maxv) can only stay saturated; it and absent items issue a
            // compare-and-swap that writes back what it compared against: branch-free, and a no-op either way
            live[e - g4] = (uint32_t)e < n && (old[e] & (inc[e] * maxv)) != inc[e] * maxv;
            prev[e] = atomicCAS(&lds[widx[e]], old[e], old[e] + (live[e - g4] ? inc[e] : 0u));
        }
#pragma unroll
        for (int e = g4; e < g4 + 4; ++e) {
            const bool won = prev[e] == old[e];
            fresh += (live[e - g4] && won && (old[e] & (inc[e] * maxv)) == 0) ? 1u : 0u;
            retry |= (live[e - g4] && !won) ? (1u << e) : 0u;
        }
    }
    if (retry) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (!(retry & (1u << e))) continue;
            uint32_t cur_word = prev[e];
            for (;;) {
                const uint32_t field = cur_word & (inc[e] * maxv);
                if (field == inc[e] * maxv) break;
                const uint32_t seen = atomicCAS(&lds[widx[e]], cur_word, cur_word + inc[e]);
                if (seen == cur_word) { fresh += field == 0 ? 1u : 0u; break; }
                cur_word = seen;
            }
        }
    }
    return fresh;
}

// Four weighted saturating adds (fine items offset | increment << 16), same structure as lds_inc8: all words
// read, all compare-and-swaps issued back to back, only lost races loop.  min(max, x + c) applied once equals c
// single increments, so the tables come out bit-identical to the unweighted path.
template <int STORAGE>
__device__ __forceinline__ uint32_t lds_addw4(uint32_t *lds, const uint32_t (&w)[4], uint32_t n)
{
    uint32_t fresh = 0;
    if (STORAGE == ST_BIT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t off = w[e] & 0xffffu;
            if ((uint32_t)e < n) {
                const uint32_t bit = 1u << (off & 31);
                fresh += (atomicOr(&lds[off >> 5], bit) & bit) == 0 ? 1u : 0u;
            }
        }
        return fresh;
    }
    constexpr uint32_t maxv = STORAGE == ST_BYTE ? 255u : 15u;
    uint32_t widx[4], shift[4], add[4], old[4], prev[4];
    bool live[4];
    uint32_t retry = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t off = w[e] & 0xffffu;
        add[e] = w[e] >> 16;
        counter_slot<STORAGE>(off, widx[e], shift[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) old[e] = lds[widx[e]];               // absent items (e >= n) read a harmless word
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t field = (old[e] >> shift[e]) & maxv;
        const uint32_t nf = min(maxv, field + add[e]);
        live[e] = (uint32_t)e < n && nf != field;
        prev[e] = atomicCAS(&lds[widx[e]], old[e], old[e] + (live[e] ? (nf - field) << shift[e] : 0u));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool won = prev[e] == old[e];
        fresh += (live[e] && won && ((old[e] >> shift[e]) & maxv) == 0) ? 1u : 0u;
        retry |= (live[e] && !won) ? (1u << e) : 0u;
    }
    if (retry) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!(retry & (1u << e))) continue;
            uint32_t cur_word = prev[e];
            for (;;) {
                const uint32_t field = (cur_word >> shift[e]) & maxv;
                if (field == maxv) break;
                const uint32_t nf = min(maxv, field + add[e]);
                const uint32_t seen = atomicCAS(&lds[widx[e]], cur_word, cur_word + ((nf - field) << shift[e]));
                if (seen == cur_word) { fresh += field == 0 ? 1u : 0u; break; }
                cur_word = seen;
            }
        }
    }
    return fresh;
}

// A workgroup lives for a few dependent round trips to HBM and little else (PMC: 73 % of its wave cycles parked), and a
// CU holds two of them, so the kernel's time is (round trips per workgroup) x (latency under load): the chain is kept
// short.  Table sizes and pointers come by value; the segment counts, the overflow flag and -- unless the tables are
// zero by decree -- the slice itself are requested together; every thread then requests ALL its item vectors at once
// (up to MAXV; slices with more fall back to the pipelined loop for the rest) before it applies the first.
template <int STORAGE, bool W>
__global__ __launch_bounds__(BIN_C_THREADS) void k_bin_apply(const SketchDev *__restrict__ sk, BinGeom g)
{
    typedef typename std::conditional<W, uint32_t, uint16_t>::type Item;
    constexpr uint32_t VEC = 16u / sizeof(Item);                  // items per 16-byte vector
    constexpr uint32_t SB = BIN_SLICE_BITS, SLICE = 1u << SB;
    constexpr uint32_t THREADS = BIN_C_THREADS;
    constexpr int MAXV = W ? 4 : 3;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SLICE / 4];   // one slice: 65536 counters of <= 8 bits
    const int t = blockIdx.y;
    const uint32_t slice = blockIdx.x;
    if (slice >= g.nslices[t]) return;
    const uint32_t c = slice / (uint32_t)g.F, fidx = slice % (uint32_t)g.F;
    const uint64_t stream = ((uint64_t)t * g.C + c) * g.F + fidx;
    constexpr int storage = STORAGE;
    const uint64_t bin0 = (uint64_t)slice << SB;
    const uint64_t left = g.tsize[t] - bin0, nb = left < SLICE ? left : SLICE;
    // byte range of the slice inside the table (the allocation is padded to 16 B)
    const uint64_t byte0 = storage == ST_BYTE ? bin0 : (storage == ST_NIBBLE ? bin0 >> 1 : bin0 >> 3);
    const uint64_t nbytes = storage == ST_BYTE ? nb : (storage == ST_NIBBLE ? (nb + 1) / 2 : (nb + 7) / 8);
    const uint32_t nvec = (uint32_t)((nbytes + 15) / 16);
    uint4 *tab = (uint4 *)(g.ttab[t] + byte0);
    uint4 *l4 = (uint4 *)lds;
    // the slice's items sit in nwgB private segments of cap2 slots (cap2 % 64 == 0: 128-B aligned, so a
    // 16-byte vector never leaves its segment).  Their vectors are enumerated compactly through a
    // prefix sum over the segments (LDS), so every thread has work whatever the segment fill levels.
    __shared__ uint32_t seg_cnt[BIN_MAX_SEG], vpre[BIN_MAX_SEG];
    __shared__ uint16_t segof[MAXV * THREADS];       // the segment every one of the first MAXV x THREADS vectors lies in (below)
    __shared__ uint32_t wsum[THREADS / 64];
    __shared__ uint32_t total_vec_sh, flag_sh, fresh_sh;
    const Item *items = (const Item *)g.gbuf2 + stream * g.nwgB * g.cap2;
    const uint32_t *counts = g.gcnt2 + stream * g.nwgB;
    {
        uint32_t myc = 0;
        if (threadIdx.x < g.nwgB) myc = counts[threadIdx.x];
        unsigned long long flag = 0;
        if (threadIdx.x == THREADS - 1) flag = g.ctr[1];          // overflow flag: leave the tables untouched for the fallback
        if (!g.zero_tables)
            for (uint32_t j = threadIdx.x; j < nvec; j += THREADS) l4[j] = tab[j];
        if (threadIdx.x < g.nwgB) seg_cnt[threadIdx.x] = myc;
        const uint32_t myv = (myc + VEC - 1) / VEC;
        const uint32_t incl = wave_incl_scan(myv);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 63) wsum[wave] = incl;
        if (threadIdx.x == THREADS - 1) { flag_sh = flag != 0 ? 1u : 0u; fresh_sh = 0; }
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (threadIdx.x < g.nwgB) vpre[threadIdx.x] = before + incl - myv;
        if (threadIdx.x == THREADS - 1) total_vec_sh = before + incl;
        __syncthreads();
        // which segment a vector lies in, looked up instead of searched for: every wave writes the number of a few segments over
        // their vectors' entries (a thread's MAXV fetches used to be MAXV binary searches over the ~30 segments, five dependent LDS
        // reads and as many branches each: a fifth of the kernel's instructions)
        for (uint32_t sgi = (uint32_t)wave; sgi < g.nwgB; sgi += THREADS / 64) {
            const uint32_t first = vpre[sgi], nv = (seg_cnt[sgi] + VEC - 1) / VEC;
            for (uint32_t i = (uint32_t)lane; i < nv && first + i < (uint32_t)MAXV * THREADS; i += 64) segof[first + i] = (uint16_t)sgi;
        }
        __syncthreads();
    }
    if (flag_sh) return;
    const uint32_t total_vec = total_vec_sh;
    if (total_vec == 0) {                                          // untouched slice: no table traffic at all ...
        if (g.zero_tables)                                         // ... unless this pass is also the table's zeroing
            for (uint32_t j = threadIdx.x; j < nvec; j += THREADS) tab[j] = make_uint4(0, 0, 0, 0);
        return;
    }
    // a vector: its items (always loaded whole) and how many of them are real
    struct Vec { uint4 q; uint32_t n; };
    auto fetch = [&](uint32_t v) {
        Vec r;
        r.q = make_uint4(0, 0, 0, 0); r.n = 0;
        if (v >= total_vec) return r;
        uint32_t lo = 0, hi = g.nwgB;      // largest segment with vpre[seg] <= v (empty segments share their successor's prefix)
        if (v < (uint32_t)MAXV * THREADS) {
            lo = segof[v];
        } else {
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (vpre[mid] <= v) lo = mid; else hi = mid;
            }
        }
        const uint32_t j0 = (v - vpre[lo]) * VEC;
        r.n = min(VEC, seg_cnt[lo] - j0);
        r.q = *(const uint4 *)(items + (uint64_t)lo * g.cap2 + j0);
        return r;
    };
    Vec first[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) first[i] = fetch(threadIdx.x + (uint32_t)i * THREADS);
    if (g.zero_tables)
        for (uint32_t j = threadIdx.x; j < nvec; j += THREADS) l4[j] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    uint32_t fresh = 0;
    auto apply = [&](const Vec &v) {
        const uint32_t w[4] = {v.q.x, v.q.y, v.q.z, v.q.w};
        return W ? lds_addw4<STORAGE>(lds, w, v.n) : lds_inc8<STORAGE>(lds, w, v.n);
    };
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (first[i].n) fresh += apply(first[i]);   // (an absent vector would still issue its compare-and-swaps, all on word 0: same-address LDS atomics serialise)
    if (total_vec > (uint32_t)MAXV * THREADS) {
        // a fuller slice: the rest through a software pipeline, two vectors ahead
        const uint32_t v_start = (uint32_t)MAXV * THREADS + threadIdx.x;
        Vec v0 = fetch(v_start), v1 = fetch(v_start + THREADS);
        for (uint32_t v = v_start; v < total_vec; v += THREADS) {
            const Vec v2 = fetch(v + 2 * THREADS);
            fresh += apply(v0);
            v0 = v1; v1 = v2;
        }
    }
    // table 0's newly occupied bins: ONE update of the device-wide counter per workgroup.  (It is one address for the whole
    // chip and takes ~90 updates per microsecond however they are issued: an update per wave -- 16 x 7630 of them for a
    // 2 GB sketch -- held this kernel at 1.4 ms whatever else it did.)
    if (t == 0) {
        const uint32_t tot = (uint32_t)wave_sum_u64(fresh);
        if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&fresh_sh, tot);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nvec; j += THREADS) tab[j] = l4[j];
    if (t == 0 && threadIdx.x == 0 && fresh_sh) atomicAdd(&g.ctr[3], (unsigned long long)fresh_sh);
}

// saturating add of `weight` to one bin with global atomics; true if the bin was zero before
__device__ __forceinline__ bool table_add_bin(const SketchDev *s, int t, uint64_t bin, uint32_t weight)
{
    uint8_t *tab = s->tab[t];
    if (s->storage == ST_BIT) {
        const uint32_t bit = 1u << (bin & 31);
        return (atomicOr((uint32_t *)tab + (bin >> 5), bit) & bit) == 0;
    }
    uint64_t word; uint32_t shift;
    if (s->storage == ST_BYTE) counter_slot<ST_BYTE>(bin, word, shift);
    else counter_slot<ST_NIBBLE>(bin, word, shift);
    const uint32_t maxv = s->storage == ST_BYTE ? 255u : 15u;
    uint32_t *w = (uint32_t *)tab + word;
    uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t cur = (old >> shift) & maxv;
        if (cur == maxv) return false;
        const uint32_t nf = min(maxv, cur + weight);
        const uint32_t prev = atomicCAS(w, old, old + ((nf - cur) << shift));
        if (prev == old) return cur == 0;
        old = prev;
    }
}

__global__ void k_bin_spill(const SketchDev *__restrict__ sk, BinGeom g)
{
    if (g.ctr[1] != 0) return;
    unsigned long long n = g.ctr[0];
    if (n > g.spill_cap) n = g.spill_cap;
    uint64_t fresh = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long e = g.spill[i];
        const int t = (int)((e >> 32) & 0xffu);
        const bool was_zero = table_add_bin(sk, t, e & 0xffffffffull, (uint32_t)((e >> 40) & 0xffu) + 1u);
        fresh += (was_zero && t == 0) ? 1 : 0;
    }
    fresh = wave_sum_u64(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&g.ctr[3], (unsigned long long)fresh);
}

// one grow-only arena per stream, so host threads counting different samples do not share buffers
KvPerStream<KvArena> g_scratch;
}
void kv_bin_scratch_release()
{
    g_scratch.for_each([](KvArena &a) { a.release(); });
}
namespace {

template <typename K>
void ensure_dynamic_lds(K kernel, size_t bytes) { kv_ensure_dynamic_lds((const void *)kernel, bytes); }

// Which instance a launch site chose, by name (KvInst, kv_binned.h): BIN_INST(k_bin_apply<ST_BIT, true>) is the pointer and the text
// of that very expression, bin_launching() hands the pointer to the launch and notes the name in the stream's list.  kv_bin_plan, the
// first step of every partitioned count, empties the list and keeps its plan; kv_bin_last_instances and kv_bin_last_plan report both
// (tests/bin_instances_common.py holds every instance and every edge of the planner's arithmetic to a case by them).
template <typename F> KvInst<F> bin_inst(F *fn, const char *name) { return kv_inst(fn, name); }
#define BIN_INST(...) bin_inst(__VA_ARGS__, #__VA_ARGS__)
enum { BIN_PLAN_NUMBERS = 13 };
struct BinLaunched { KvLaunched list; uint64_t plan[BIN_PLAN_NUMBERS] = {}; };
KvPerStream<BinLaunched> g_bin_launched;
template <typename F> F *bin_launching(const KvInst<F> &k, hipStream_t st)
{
    g_bin_launched.get(st).list.note(k.name);
    return k.fn;
}

}  // namespace

int kv_device_cus()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 256;
        kv_thread_device();
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        cus = n;
    }
    return cus;
}

// linear-counting estimate of the distinct k-mers behind an occupancy of table 0
double kv_estimate_distinct(uint64_t occupied, uint64_t size)
{
    if (occupied >= size) return (double)size * std::log((double)size);
    return -(double)size * std::log1p(-(double)occupied / (double)size);
}

// can stage A hash this batch from its 2-bit form (k_bin_hash_2bit)?  Reads of one length, murmur kinds, 16 <= k <= 64.  KV_BIN_2BIT=0: never
bool kv_bin_two_bit(const kv_sketch *s, const kv_reads *reads)
{
    const char *e = kv_knob("KV_BIN_2BIT");
    if (e && atoi(e) == 0) return false;
    return reads && reads->uni_len != 0 && reads->uni_per_tile != 0 && s->h.hashfam == HF_MURMUR && s->h.ksize >= SKM_MIN_K && s->h.ksize <= SKM_MAX_K &&
           reads->uni_len >= (uint32_t)s->h.ksize && reads->n_tiles > 0;
}

bool kv_binned_eligible(const kv_sketch *s, const kv_reads *reads, uint64_t n_kmers, int nbands)
{
    // reads == nullptr: the items come from a hash list (kv_consume_hashes)
    const char *force = kv_knob("KV_COUNT_PATH");
    if (force && strcmp(force, "atomic") == 0) return false;
    if (s->h.ntables > BIN_MAX_T) return false;
    uint64_t pmin = UINT64_MAX, pmax = 0;
    for (int t = 0; t < s->h.ntables; ++t) { pmin = std::min(pmin, s->h.size[t]); pmax = std::max(pmax, s->h.size[t]); }
    if (pmax > (uint64_t)BIN_C * BIN_MAX_F * 65536ull) return false;      // <= 2^31 bins per table
    if (force && (strcmp(force, "binned") == 0 || strcmp(force, "skm") == 0)) return reads ? reads->n_tiles > 0 : n_kmers > 0;
    const uint64_t expected = nbands > 0 ? n_kmers / (uint64_t)nbands : n_kmers;
    // worth it once the batch touches the tables about as densely as streaming them costs.  With the 2-bit stage A the hashing costs
    // half as much, and what is left to compare is T global compare-and-swaps per k-mer that reaches the tables (~27 G/s device-wide)
    // against streaming the tables once (read + write at ~4.7 TB/s) plus the split: even at one k-mer per 32 bins -- config 4's
    // 0.6x batches under 8-fold banding: 164 M k-mers into 2 G bins -- the atomics cost 24 ms and the streamed tables 3.4 + 7
    // (a hash list has no hashing left to pay at all: 164 M hashes into a band's 2 G-bin tables -- config 4 with every band resident,
    // scratch/cfg4_whole.py -- took 30.9 ms through the atomics)
    const uint64_t density = !reads || kv_bin_two_bit(s, reads) ? 32 : 8;
    return pmin >= (1ull << 20) && expected >= (1ull << 22) && expected * density >= pmax;
}

int kv_bin_plan(kv_sketch *s, uint64_t n_items_max, int nbands, bool use_mask, uint64_t work_units, uint32_t lds_front,
                uint32_t nwgA_fixed, bool weighted, BinPlan *plan)
{
    hipStream_t st = kv_stream();
    KvArena &scratch = g_scratch.get(st);
    BinLaunched &launched = g_bin_launched.get(st);
    launched.list.begin();
    { std::lock_guard<std::mutex> lk(launched.list.mu); memset(launched.plan, 0, sizeof(launched.plan)); }   // (a plan that fails leaves none)
    BinGeom &g = plan->g;
    memset(&g, 0, sizeof(g));
    plan->weighted = weighted;
    g.zero_tables = s->lazy_zero ? 1 : 0; g.T = s->h.ntables;
    g.tile_lds = lds_front; g.sbits = BIN_SLICE_BITS;
    // shape and sizes: the arithmetic is kv_bin_plan.h's
    const BinShape sh = bin_shape(s->h.size, g.T, weighted);
    const BinSizes z = bin_sizes(sh, n_items_max, nbands, use_mask, work_units, nwgA_fixed, weighted, kv_device_cus());
    plan->maxsl = sh.maxsl; plan->cmax = sh.cmax; plan->threadsA = sh.threadsA;
    g.F = sh.F; g.C = sh.C; g.recipF = sh.recipF; g.ringB = sh.ringB;
    for (int t = 0; t < g.T && t < BIN_MAX_T; ++t) {
        g.tsize[t] = s->h.size[t]; g.ttab[t] = s->h.tab[t]; g.nslices[t] = sh.nslices[t]; g.tmagic[t] = kv_fastmod_magic(s->h.size[t]);
    }
    g.nwgA = z.nwgA; g.nwgB = z.nwgB; g.quotaA = z.quotaA;
    g.cap1 = z.cap1; g.cap2 = z.cap2; g.spill_cap = z.spill_cap; g.fast4 = z.fast4;
    // (no memory for the staging buffers is a CAPACITY answer: the caller has a path that needs less -- in the end the atomic kernel, which needs none)
    if (scratch.need(z.b_total) != hipSuccess) {
        (void)hipGetLastError();
        kv_set_error("no device memory for the partitioned count's staging buffers (%.1f GB)", (double)z.b_total / 1e9);
        return KV_ERR_CAPACITY;
    }
    unsigned char *base = (unsigned char *)scratch.p;
    g.gbuf1 = (uint32_t *)base; base += z.b_buf1;
    g.gbuf2 = (uint16_t *)base; base += z.b_buf2;
    g.gcnt1 = (uint32_t *)base; base += z.b_cnt1;
    g.gcnt2 = (uint32_t *)base; base += z.b_cnt2;
    g.spill = (unsigned long long *)base; base += z.b_spill;
    g.ctr = (unsigned long long *)base;
    {
        // the order kv_bin_last_plan documents (include/kvsketch.h)
        const uint64_t numbers[BIN_PLAN_NUMBERS] = {(uint64_t)g.T, sh.maxsl, (uint64_t)sh.cmax, (uint64_t)g.F, (uint64_t)g.C, g.ringB, sh.threadsA, g.nwgA, g.nwgB,
                                                    g.cap1, g.cap2, weighted ? 1u : 0u, (uint64_t)g.fast4};
        std::lock_guard<std::mutex> lk(launched.list.mu);
        memcpy(launched.plan, numbers, sizeof(numbers));
    }
    KV_HIP(hipMemsetAsync(g.ctr, 0, z.b_ctr, st));   // every segment count is written by its owner: no other memset
    return KV_OK;
}

int kv_bin_finish(kv_sketch *s, BinPlan &plan, bool added_from_ctr, uint64_t n_added_fixed, uint64_t *n_added)
{
    hipStream_t st = kv_stream();
    BinGeom &g = plan.g;
    const uint64_t ns = (uint64_t)g.T * g.C;
    {
        KvProfScope prof(plan.weighted ? "k_bin_split_w" : "k_bin_split");
        const size_t lds = bin_split_lds((uint32_t)g.F, g.ringB, plan.weighted ? 4 : 2).total;
        const auto kernel = plan.weighted ? BIN_INST(k_bin_split<true>) : BIN_INST(k_bin_split<false>);
        ensure_dynamic_lds(kernel.fn, lds);
        hipLaunchKernelGGL(bin_launching(kernel, st), dim3(g.nwgB, (unsigned)ns), dim3(BIN_B_THREADS), lds, st, g);
    }
    {
        KvProfScope prof(plan.weighted ? "k_bin_apply_w" : "k_bin_apply");
        const dim3 gridC(plan.maxsl, (unsigned)g.T);
        const SketchDev *d = (const SketchDev *)s->d_desc;
        const int storage = s->h.storage;
        auto kernel = storage == ST_BYTE ? BIN_INST(k_bin_apply<ST_BYTE, false>) : storage == ST_NIBBLE ? BIN_INST(k_bin_apply<ST_NIBBLE, false>) : BIN_INST(k_bin_apply<ST_BIT, false>);
        if (plan.weighted) kernel = storage == ST_BYTE ? BIN_INST(k_bin_apply<ST_BYTE, true>) : storage == ST_NIBBLE ? BIN_INST(k_bin_apply<ST_NIBBLE, true>) : BIN_INST(k_bin_apply<ST_BIT, true>);
        hipLaunchKernelGGL(bin_launching(kernel, st), gridC, dim3(BIN_C_THREADS), 0, st, d, g);
    }
    {
        KvProfScope prof("k_bin_spill");   // usually a handful of items; the kernels check the overflow flag themselves
        hipLaunchKernelGGL(bin_launching(BIN_INST(k_bin_spill), st), dim3(256), dim3(256), 0, st, (const SketchDev *)s->d_desc, g);
    }
    KV_HIP(hipGetLastError());
    unsigned long long ctr[4] = {0, 0, 0, 0};
    KV_HIP(hipMemcpyAsync(ctr, g.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    if (ctr[1] != 0) {
        kv_set_error("partitioned count: spill list overflow (%llu items)", ctr[0]);
        return KV_ERR_CAPACITY;
    }
    *n_added = added_from_ctr ? ctr[2] : n_added_fixed;
    s->lazy_zero = false;          // stage C has written every slice
    // exact occupancy bookkeeping; n_unique_kmers as a linear-counting estimate
    if (s->occ_dirty) {
        int rc = kv_sketch_refresh_occupancy(s);   // recount includes this batch
        if (rc != KV_OK) return rc;
        s->n_unique = (uint64_t)(kv_estimate_distinct(s->n_occupied, s->h.size[0]) + 0.5);
    } else {
        const double before = kv_estimate_distinct(s->n_occupied, s->h.size[0]);
        s->n_occupied += ctr[3];
        const double after = kv_estimate_distinct(s->n_occupied, s->h.size[0]);
        s->n_unique += (uint64_t)(after - before + 0.5);
    }
    return KV_OK;
}

// returns KV_OK, or KV_ERR_CAPACITY when the spill list overflowed (tables untouched: caller falls back)
int kv_consume_binned(kv_sketch *s, const kv_reads *reads, const uint64_t *d_list, uint32_t list_stride,
                      const ConsumeFilter &filter, const kv_sketch *mask, uint64_t n_kmers, int nbands, uint64_t *n_added,
                      bool weighted_list)
{
    // source: the packed reads (hash in stage A) or, when reads == nullptr, n_kmers hashes at d_list[i * list_stride]
    hipStream_t st = kv_stream();
    BinPlan plan;
    const bool two_bit = reads && kv_bin_two_bit(s, reads);
    const uint32_t n_units2 = two_bit ? (reads->n_tiles + BIN2_TILES - 1u) / BIN2_TILES : 0u;
    {
        // a list's work units depend on the stage-A workgroup size, which the table sizes alone decide
        const uint32_t threadsA = bin_shape(s->h.size, s->h.ntables, weighted_list).threadsA;
        const uint64_t work_units = two_bit ? n_units2 : reads ? reads->n_tiles
                                          : (n_kmers + (uint64_t)threadsA * BIN_LIST_ROUNDS - 1) / ((uint64_t)threadsA * BIN_LIST_ROUNDS);
        const int rc = kv_bin_plan(s, n_kmers, nbands, filter.use_mask != 0, work_units, reads && !two_bit ? reads->tile_lds_bytes : 0u, 0u, weighted_list, &plan);
        if (rc != KV_OK) return rc;
    }
    BinGeom &g = plan.g;
    const bool small = plan.cmax <= 32;            // 512-thread stage-A workgroups; else 1024 (plan.threadsA)
    const unsigned threadsA = plan.threadsA;
    const SketchDev *d_mask = mask ? mask->d_desc : nullptr;
    if (two_bit) {
        KvProfScope prof("k_bin_hash_2bit");
        const SketchDev *d = (const SketchDev *)s->d_desc;
        const bool kw2 = s->h.ksize > 32;
        const bool k31 = !kw2 && s->h.ksize == 31 && !kv_knob("KV_SKM_ANY_K");
        auto kernel = k31 ? BIN_INST(k_bin_hash_2bit<512, 1, 31>) : !kw2 ? BIN_INST(k_bin_hash_2bit<512, 1>) : BIN_INST(k_bin_hash_2bit<512, 2>);
        if (!small) kernel = k31 ? BIN_INST(k_bin_hash_2bit<1024, 1, 31>) : !kw2 ? BIN_INST(k_bin_hash_2bit<1024, 1>) : BIN_INST(k_bin_hash_2bit<1024, 2>);
        hipLaunchKernelGGL(bin_launching(kernel, st), dim3(g.nwgA), dim3(threadsA), 0, st, reads_dev(reads), n_units2, d, d_mask, filter, g);
    } else if (reads) {
        KvProfScope prof("k_bin_hash_direct");
        const int k = s->h.ksize;
        const int nw = s->h.hashfam == HF_MURMUR ? (k <= 32 ? 8 : (k <= 64 ? 16 : 0)) : 0;
        auto kernel = nw == 8 ? BIN_INST(k_bin_hash_direct<512, 8>) : nw == 16 ? BIN_INST(k_bin_hash_direct<512, 16>) : BIN_INST(k_bin_hash_direct<512, 0>);
        if (!small) kernel = nw == 8 ? BIN_INST(k_bin_hash_direct<1024, 8>) : nw == 16 ? BIN_INST(k_bin_hash_direct<1024, 16>) : BIN_INST(k_bin_hash_direct<1024, 0>);
        ensure_dynamic_lds(kernel.fn, (size_t)g.tile_lds);
        hipLaunchKernelGGL(bin_launching(kernel, st), dim3(g.nwgA), dim3(threadsA), g.tile_lds, st,
                           reads_dev(reads), reads->n_tiles, (const SketchDev *)s->d_desc, d_mask, filter, g);
    } else {
        KvProfScope prof(weighted_list ? "k_bin_list_w" : "k_bin_list");
        const SketchDev *d = (const SketchDev *)s->d_desc;
        auto kernel = weighted_list ? BIN_INST(k_bin_list<512, true>) : BIN_INST(k_bin_list<512, false>);
        if (!small) kernel = weighted_list ? BIN_INST(k_bin_list<1024, true>) : BIN_INST(k_bin_list<1024, false>);
        hipLaunchKernelGGL(bin_launching(kernel, st), dim3(g.nwgA), dim3(threadsA), 0, st, d_list, n_kmers, list_stride, d, g);
    }
    return kv_bin_finish(s, plan, reads != nullptr || weighted_list, n_kmers, n_added);
}

// the k_bin_* instances the last partitioned count launched on the calling thread's stream, and the numbers of its plan (include/kvsketch.h)
extern "C" int kv_bin_last_instances(char *out, uint64_t cap)
{
    KV_REQUIRE(g_bin_launched.get(kv_stream()).list.report(out, cap), KV_ERR_CAPACITY, "kv_bin_last_instances: buffer too small");
    return KV_OK;
}

extern "C" int kv_bin_last_plan(uint64_t *out, uint64_t n)
{
    KV_REQUIRE(out && n >= BIN_PLAN_NUMBERS, KV_ERR_CAPACITY, "kv_bin_last_plan: room for %d numbers needed", (int)BIN_PLAN_NUMBERS);
    BinLaunched &l = g_bin_launched.get(kv_stream());
    std::lock_guard<std::mutex> lk(l.list.mu);
    memcpy(out, l.plan, sizeof(l.plan));
    return KV_OK;
}
