// kv_skm.hip -- super-k-mer front end of count and novel: every DISTINCT k-mer of a batch is hashed, filtered,
// counted and evaluated once, however many reads contain it (kv_skm_device.h says why that is bit-identical).
//
//   S1  k_skm_emit    a workgroup per tile: the minimizer value of every k-mer (smallest mixed canonical m-mer
//                     among its w = k - m + 1, by log-step window minima in LDS), the reads cut into runs of
//                     consecutive k-mers of one minimizer bucket, each run stored as a record of 2-bit bases in
//                     the coarse bucket's stream (private segment per workgroup, cursor in LDS, direct stores).
//   S2  k_skm_split   every coarse stream is split into its F2 fine buckets (again private segments, direct stores);
//                     a fine bucket holds ~8 k k-mer instances, all occurrences of ~2 k distinct k-mers.
//   S3  k_skm_count   persistent workgroups take fine buckets: the canonical 2-bit k-mers are combined in an LDS hash
//                     table (key -> count), then each distinct k-mer is expanded to ASCII (both strands), hashed
//                     with the two murmurs, band/mask filtered, reduced modulo the T table sizes and appended as T
//                     WEIGHTED items to the coarse buckets of the partitioned count (kv_binned.hip stages B and C).
//   S6  k_skm_novel   same buckets of the case sample: combine, evaluate kmer_is_interesting() once per distinct
//                     k-mer, then walk the records again and set the hit-mask bit of every occurrence of an
//                     interesting k-mer; k_tile_hits + the ordinary emit kernels do the rest.
//
// This file is the host half: geometry planning, arenas, launches, the C entry points.  The kernels are in two headers that
// only this translation unit includes: kv_skm_emit_device.h (S1, S2) and kv_skm_bucket_device.h (the LDS table, the bucket
// walk, S3, S3', S6, the owner's scan and the loose-list kernels).
//
// Nothing here can lose a k-mer: a full segment, a full LDS table or an uncacheable key diverts single records to a
// "loose" list that is processed one occurrence at a time (k_skm_loose_*); if that list overflows too, a flag makes
#include <algorithm>
#include <cmath>

#include "kv_binned.h"
#include "kv_novel_device.h"
#include "kv_skm_device.h"
#include "kv_skm_emit_device.h"
#include "kv_skm_bucket_device.h"

namespace {

// ---- host ----------------------------------------------------------------------------------------------
// A kernel instance together with its name.  SKM_INST(k_skm_emit<16>) yields the function pointer and the text of that very
// expression, so the name cannot drift from the kernel; skm_launching() hands the pointer to the launch and notes the name in the
// stream's list, which kv_skm_last_instances reports (tests/instances_common.py holds every instance to a case by that report).
// Every entry point of this file that can launch a super-k-mer kernel empties the list first (skm_launched_begin).  (KvInst and
// KvLaunched are kv_binned.h's: the partitioned count keeps the same books through BIN_INST.)
template <typename F> KvInst<F> skm_inst(F *fn, const char *name) { return kv_inst(fn, name); }
#define SKM_INST(...) skm_inst(__VA_ARGS__, #__VA_ARGS__)
KvPerStream<KvLaunched> g_skm_launched;
void skm_launched_begin(hipStream_t st) { g_skm_launched.get(st).begin(); }
template <typename F> F *skm_launching(const KvInst<F> &k, hipStream_t st)
{
    g_skm_launched.get(st).note(k.name);
    return k.fn;
}

// Bump pointer over an arena, every part rounded up to 256 bytes.  Without a base it only adds up: a layout written once as a function
// of an SkmCarve gives the total for KvArena::need and then the pointers, and the two cannot drift apart.
struct SkmCarve {
    unsigned char *base;
    size_t total = 0;
    explicit SkmCarve(void *arena = nullptr) : base((unsigned char *)arena) {}
    template <typename T> T *take(size_t bytes) { T *p = (T *)base; bytes = kv_round_up(bytes, 256); total += bytes; if (base) base += bytes; return p; }
};

// the parts of a list the count pass writes: `entries` keys of kw words, a V beside each, first entry and entry count of every bucket
template <typename V> size_t skm_list_lay(SkmCarve c, uint64_t entries, int kw, uint32_t n_buckets, uint64_t **keys, V **vals, uint32_t **bstart, uint32_t **bcount)
{
    *keys = c.take<uint64_t>(entries * 8 * kw); *vals = c.take<V>(entries * sizeof(V));
    *bstart = c.take<uint32_t>((uint64_t)n_buckets * 4); *bcount = c.take<uint32_t>((uint64_t)n_buckets * 4);
    return c.total;
}
// (the two bucket arrays lie one behind the other)
hipError_t skm_list_zero(uint32_t *bstart, uint32_t *bcount, hipStream_t st) { return hipMemsetAsync(bstart, 0, (size_t)((unsigned char *)bcount - (unsigned char *)bstart) * 2, st); }

// The distinct list as the host holds it; SkmGeom::dl_* is the copy a kernel receives while the list is attached.
struct SkmDistinctList {
    uint64_t *keys = nullptr, *hash = nullptr;
    uint32_t *bstart = nullptr, *bcount = nullptr;
    uint32_t cap_wg = 0, chunk = 0, nchunks = 0;
    static size_t bytes(uint64_t entries, int kw, uint32_t n_buckets) { SkmDistinctList l; return skm_list_lay(SkmCarve(), entries, kw, n_buckets, &l.keys, &l.hash, &l.bstart, &l.bcount); }
    // room for `entries` k-mers in `arena`, the bucket arrays zeroed; KV_ERR_CAPACITY: the arena cannot grow to it
    int carve(KvArena &arena, uint64_t entries, int kw, uint32_t n_buckets, uint32_t cap_wg_, uint32_t chunk_, uint32_t nchunks_, hipStream_t st)
    {
        if (arena.need(bytes(entries, kw, n_buckets)) != hipSuccess) return KV_ERR_CAPACITY;
        skm_list_lay(SkmCarve(arena.p), entries, kw, n_buckets, &keys, &hash, &bstart, &bcount);
        cap_wg = cap_wg_; chunk = chunk_; nchunks = nchunks_;
        KV_HIP(skm_list_zero(bstart, bcount, st));
        return KV_OK;
    }
    void attach(SkmGeom &g) const { g.dl_keys = keys; g.dl_hash = hash; g.dl_bstart = bstart; g.dl_bcount = bcount; g.dl_cap_wg = cap_wg; g.dl_chunk = chunk; g.dl_nchunks = nchunks; }
    static void detach(SkmGeom &g) { g.dl_keys = nullptr; g.dl_hash = nullptr; g.dl_bstart = nullptr; g.dl_bcount = nullptr; }
};
// the abundance list a sketch keeps (KvAbundList, which owns its memory) goes to the kernels the same way
void skm_abl_attach(const KvAbundList &al, SkmGeom &g) { g.abl_keys = al.keys; g.abl_cnts = al.cnts; g.abl_bstart = al.bstart; g.abl_bcount = al.bcount; g.abl_cap_wg = (uint32_t)al.cap_wg; }
void skm_abl_detach(SkmGeom &g) { g.abl_keys = nullptr; g.abl_cnts = nullptr; g.abl_bstart = nullptr; g.abl_bcount = nullptr; }

// The bucketed form of the last batch consumed on a stream stays in that stream's arena, so a scan of the same
// batch (the case sample: count, then novel) does not cut its reads again.
struct SkmIndex {
    KvArena arena;
    uint64_t reads_uid = 0;
    int k = 0;
    bool valid = false;
    double distinct_hint = 0.0;     // distinct / all k-mers of the last batch routed on this stream (kv_skm_route_distinct)
    SkmGeom g;
    // distinct list of the batch (kv_sketch::scan_hint): key + hash of every distinct k-mer the count pass drained, bucket by bucket
    KvArena dl;
    size_t dl_refused = SIZE_MAX;    // the smallest list kv_skm_mex_route asked for and did not get since the arena was last empty (a refused
                                     // allocation of tens of gigabytes takes a third of a second, and the arena is given up for the attempt)
    SkmDistinctList list;
    bool dl_valid = false;
    bool mex_scan_ready = false;     // the arena holds an owner's combined buckets with their distinct list (kv_skm_mex_route, keep_scan): kv_skm_mex_scan_set
    uint64_t builds = 0;             // batches bucketed on this stream so far
    KvArena bits;                    // NovelParams::case0_bits of the scan in flight
    std::mutex mu;
    // what a later call on the stream may reuse (valid, mex_scan_ready, dl_valid): a function that writes over one of them drops it first
    enum { BATCH = 1, MEX_SCAN = 2, LIST = 4, ALL = 7 };
    void drop(int what) { valid &= !(what & BATCH); mex_scan_ready &= !(what & MEX_SCAN); dl_valid &= !(what & LIST); }
    // nothing to reuse, and the bucket and list arenas go back to the device
    void give_back() { drop(ALL); arena.release(); dl.release(); list = SkmDistinctList(); }
};
std::map<hipStream_t, SkmIndex> g_skm;
std::mutex g_skm_mu;
int g_skm_pref_k = 0;                    // bucket count of the last build that chose its own (guarded by g_skm_mu), see skm_build
uint64_t g_skm_pref_nfine = 0;
double g_skm_last_distinct = 0.0;        // distinct share of the batch counted last on any stream (guarded by g_skm_mu): a scan
                                          // that has to bucket its batch itself sizes the buckets by it

SkmIndex &skm_index_for(hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_skm_mu);
    return g_skm[kv_stream_key(st)];
}
}
void kv_skm_scratch_release()
{
    std::lock_guard<std::mutex> lk(g_skm_mu);
    for (auto &kv : g_skm) {
        SkmIndex &idx = kv.second;
        std::lock_guard<std::mutex> ilk(idx.mu);
        idx.give_back();
        idx.bits.release();
    }
}
namespace {

inline uint32_t skm_nwg3(const SkmGeom &g)
{
    // persistent workgroups of the bucket kernels: three per CU fill its LDS (two, which leave a third of it -- and of the wave slots -- to
    // whatever another stream has queued, measured slower: DESIGN.md section 4.1, "samples on separate streams")
    return (uint32_t)std::min<uint64_t>((g.n_buckets + g.bpt - 1) / g.bpt, 3u * (uint32_t)kv_device_cus());
}

// Buckets per ticket of the work counter.  A ticket costs a returning atomic on a word every workgroup asks for -- ~10 per microsecond
// device-wide, measured: a sample's 64 k buckets one per ticket took k_skm_count from 3.1 to 6.9 ms, two per ticket to 3.7 -- and a big
// ticket leaves a tail (16: +0.08 ms, 32: +0.13).  8 for a whole sample; fewer where the buckets are few (a rank's share of the exchange:
// 7 936 buckets for 768 workgroups -- tickets of 8 give a quarter of them two and the rest one), down to 2.
// A workgroup takes at most quota3 buckets: one and a half even shares, in whole tickets.
static void skm_plan_tickets(SkmGeom &g)
{
    g.bpt = SKM_BUCKETS_PER_TICKET;
    while (g.bpt > 2u && g.n_buckets / g.bpt < 4u * 768u) g.bpt /= 2u;
    const uint32_t nwg3 = skm_nwg3(g);
    const uint64_t avg = (g.n_buckets + nwg3 - 1) / nwg3;
    g.quota3 = (uint32_t)kv_round_up(avg + avg / 2 + 1, g.bpt);
}

inline uint32_t pow2_ceil(uint64_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

// nfine fine buckets as C1 coarse buckets of F2 = 2^fbits each.  At most 255 x 4096 buckets (a bucket id travels as 20 bits through
// S1): 8.5 G k-mers at 8192 per bucket; bigger batches get bigger buckets, which only costs deduplication efficiency
static void skm_bucket_grid(uint64_t nfine, uint32_t *C1, uint32_t *F2, uint32_t *fbits)
{
    *F2 = std::min<uint32_t>(512u, pow2_ceil((uint64_t)std::ceil(std::sqrt((double)nfine))));
    if (nfine > 255ull * *F2) *F2 = std::min<uint32_t>(SKM_MAX_F2, pow2_ceil((nfine + 254) / 255));
    *fbits = 0;
    while ((1u << *fbits) < *F2) ++*fbits;
    *C1 = (uint32_t)std::min<uint64_t>(255, std::max<uint64_t>(1, (nfine + *F2 - 1) / *F2));
}

// records: one run per ~ (w + 1) / 2 k-mers, one more per read, a few cuts at ncap
static double skm_rec_est(uint64_t n_kmers, double n_reads, int w) { return (double)n_kmers * 2.2 / (double)(w + 1) + n_reads + 1024.0; }
// records per private segment for a mean of `mean`: `slack` times that and eight standard deviations
static uint32_t skm_seg_cap(double mean, double slack, uint64_t floor) { return (uint32_t)kv_round_up((uint64_t)(mean * slack + 8.0 * std::sqrt(mean)) + floor, 16); }
// loose records: segment overflow (whole records) and occurrences that missed a full LDS table (one k-mer each)
static uint64_t skm_loose_cap(double rec_est, uint64_t n_kmers) { return (uint64_t)(rec_est / 8.0) + n_kmers / 16 + (1u << 20); }
// words of record-start bits per wave in the bucket walk
static uint32_t skm_sbw(int ncap) { return ((64u * (uint32_t)ncap) >> 5) + 2u; }
// 16-byte records without positions (kv_skm_device.h): shorter records, fewer k-mers in each
static void skm_make_compact(SkmGeom &g) { g.compact = 1u; g.recw = 2; g.ncap = std::min(g.ncap, SKM_C_BASES + 1 - g.k); g.sbw = skm_sbw(g.ncap); }

int skm_minimizer_len(int k) { return k >= 24 ? 12 : k / 2; }

// reads per wave and chunk size of the wave kernel for batches of equal-length reads (0: use the tile kernel).  One packed
// word and one chunk per lane, and about as many runs as lanes: a run per (w + 1) / 2 k-mers, one more per read.
// threads per workgroup of the wave kernel (512 | 1024)
static thread_local uint32_t tl_s1_threads = 0;       // a caller's choice for the launch it is about to make (kv_skm_mex_emit)
static uint32_t skm_wave_threads() { return tl_s1_threads ? tl_s1_threads : SKM_S1_WAVE_THREADS_DEFAULT; }

static uint32_t skm_wave_plan(const SkmGeom &g, const kv_reads *reads, int *ch)
{
    const uint32_t L = reads->uni_len;
    if (!L || L < (uint32_t)g.k || g.w <= 8) return 0;
    const uint32_t wpr = (L + 15) / 16, nk = L - (uint32_t)g.k + 1;
    const double runs = 1.0 + (nk - 1) * 2.0 / (g.w + 1) + (double)nk / g.ncap * 0.5;
    uint32_t best = 0;
    for (int c : {16, 8}) {
        if (g.w <= c) continue;
        const uint32_t cpr = (nk + c - 1) / c;
        uint32_t R = std::min<uint32_t>(64 / wpr, 64 / cpr);
        R = std::min<uint32_t>(R, (uint32_t)(58.0 / runs));
        if (R >= best && R > 0) { best = R; *ch = c; }       // equal R: the smaller chunk keeps more lanes busy
    }
    if (best < 2) return 0;
    const uint32_t threads = skm_wave_threads();
    // three workgroups of 512 per CU, or one of 1024 -- or the tile kernel
    if ((size_t)skm_wave_slice_words(best, L, nk, *ch) * 4 * (threads / 64) + 2048 > (threads == 1024 ? 160000u : 54000u)) return 0;
    return best;
}

// the lane-per-read kernel takes batches of equal-length reads with w = 20 or 40 (k = 31, 51: m = 12) and up to 256 bases
// workgroups of the lane-per-read cut a CU holds at once, by their LDS (0: not even two -- other kernels cut such reads)
static uint32_t skm_lane_wgs_per_cu(uint32_t L)
{
    const size_t need = (size_t)skm_lane_slice_words((L + 15u) / 16u) * 4 * (SKM_LANE_THREADS / 64) + 1200;
    if (need <= 160000u / (SKM_LANE_WAVES / 2)) return 3u;
    return need <= 160000u / 2u ? 2u : 0u;
}
// (by the read length alone: kv_mex_plan_short, which sees no reads, asks this way)
static bool skm_lane_fits_len(const SkmGeom &g, uint32_t L)
{
    if (!L || L < (uint32_t)g.k || g.m != 12 || (g.w != SKM_LANE_B && g.w != 2 * SKM_LANE_B) || L > 256u) return false;
    // (w = 40, k = 51: two arrays of suffix minima; that instance is compiled for 4 waves per SIMD and skm_build starts two workgroups
    // per CU for it -- at six waves it spilled and measured slower than the wave kernel, 5.5 against 4.1 ms per step of config 5)
    // three workgroups per CU for reads of up to 112 bases (seven packed words and their reverse complement per lane), two up to 224
    return skm_lane_wgs_per_cu(L) >= 2u;
}
static bool skm_lane_fits(const SkmGeom &g, const kv_reads *reads) { return skm_lane_fits_len(g, reads->uni_len); }

void skm_launch_emit(const SkmGeom &g, const kv_reads *reads, hipStream_t st)
{
    KvProfScope prof("k_skm_emit");
    int ch = 16;
    if (skm_lane_fits(g, reads)) {
        const uint32_t wpr = (reads->uni_len + 15u) / 16u;
        const size_t lds = (size_t)skm_lane_slice_words(wpr) * 4 * (SKM_LANE_THREADS / 64);
        const uint64_t n_groups = (reads->n_reads + 63) / 64;
        auto kernel = wpr <= 8 ? SKM_INST(k_skm_emit_lane<1, 8>) : SKM_INST(k_skm_emit_lane<1, 16>);
        if (g.w != SKM_LANE_B) kernel = wpr <= 8 ? SKM_INST(k_skm_emit_lane<2, 8>) : SKM_INST(k_skm_emit_lane<2, 16>);
        kv_ensure_dynamic_lds((const void *)kernel.fn, lds);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(g.nwg1), dim3(SKM_LANE_THREADS), lds, st, reads_dev(reads), g, (uint32_t)n_groups, SKM_LANE_FLUSH_BLOCKS);
        return;
    }
    if (const uint32_t R = skm_wave_plan(g, reads, &ch)) {
        const uint32_t L = reads->uni_len, nk = L - (uint32_t)g.k + 1;
        const uint32_t threads = skm_wave_threads(), nwaves = threads / 64;
        const size_t lds = (size_t)skm_wave_slice_words(R, L, nk, ch) * 4 * nwaves;
        const uint64_t n_mt = (reads->n_reads + R - 1) / R;
        // the same share of the batch per workgroup as the tile kernel's quota, dealt to its waves
        // a ticket is SKM_MT_PER_TICKET groups for a whole sample; small batches (a shard of a sample, a test) get smaller
        // tickets so that every wave of the grid still finds two
        const uint64_t waves = (uint64_t)g.nwg1 * nwaves;
        const uint32_t per_ticket = (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(SKM_MT_PER_TICKET, n_mt / (2 * waves)));
        const uint64_t per_wave = (uint64_t)g.quota1 * reads->uni_per_tile / R / nwaves + per_ticket;
        const uint32_t quota_mt = (uint32_t)std::min<uint64_t>(kv_round_up(per_wave, per_ticket), 0xfffffff0ull);
        auto kernel = ch == 16 ? SKM_INST(k_skm_emit_wave<16, 512>) : SKM_INST(k_skm_emit_wave<8, 512>);
        if (threads == 1024) kernel = ch == 16 ? SKM_INST(k_skm_emit_wave<16, 1024>) : SKM_INST(k_skm_emit_wave<8, 1024>);
        kv_ensure_dynamic_lds((const void *)kernel.fn, lds);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(g.nwg1), dim3(threads), lds, st, reads_dev(reads), g, R, (uint32_t)n_mt, quota_mt, per_ticket);
        return;
    }
    const size_t lds = ((size_t)g.np_max / 16 + KV_TILE_MAX_READS + 8 + (size_t)g.np_max + 96) * 4 + (((size_t)g.np_max + 96 + 1) & ~(size_t)1) * 2;
    const auto kernel = g.w > 16 ? SKM_INST(k_skm_emit<16>) : SKM_INST(k_skm_emit<8>);
    kv_ensure_dynamic_lds((const void *)kernel.fn, lds);
    hipLaunchKernelGGL(skm_launching(kernel, st), dim3(g.nwg1), dim3(SKM_THREADS1), lds, st, reads_dev(reads), reads->n_tiles, g);
}

void skm_launch_split(const SkmGeom &g, hipStream_t st)
{
    KvProfScope prof("k_skm_split");
    // sorted scatter while a chunk of the instance holds 2 records per fine bucket or more (KV_SKM_S2=plain|sorted overrides)
    const char *s2 = kv_knob("KV_SKM_S2");
    const bool fits = skm_s2_sorted_fits(g.recw, g.F2);
    const bool sorted = s2 ? strcmp(s2, "sorted") == 0 && fits : fits;
    if (sorted) {
        const size_t lds = skm_s2_lds(g.recw, g.F2);
        auto kernel = g.recw == 2 ? SKM_INST(k_skm_split_sorted<2>) : SKM_INST(k_skm_split_sorted<3>);
        if (g.recw > 3) kernel = SKM_INST(k_skm_split_sorted<4>);
        kv_ensure_dynamic_lds((const void *)kernel.fn, lds);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(g.nwg2, g.C1), dim3(SKM_THREADS2), lds, st, g);
    } else {
        const auto kernel = g.recw == 2 ? SKM_INST(k_skm_split<true>) : SKM_INST(k_skm_split<false>);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(g.nwg2, g.C1), dim3(SKM_THREADS2), 0, st, g);
    }
}

// a loose-list kernel, grid-stride over the list: its instance for one-word or two-word keys
template <typename... A>
void skm_launch_loose(KvInst<void(SkmGeom, A...)> one, KvInst<void(SkmGeom, A...)> two, hipStream_t st, const SkmGeom &g, typename std::common_type<A>::type... args)
{
    hipLaunchKernelGGL(skm_launching(g.kw == 1 ? one : two, st), dim3(SKM_LOOSE_WGS), dim3(256), 0, st, g, args...);
}

// occurrences the bucket kernels sent through the loose list (they missed a full LDS table), from a host copy of the counters
double skm_outside_tables(const unsigned long long *c) { return (double)(c[SKM_CTR_LOOSE] > c[SKM_CTR_LOOSE_S12] ? c[SKM_CTR_LOOSE] - c[SKM_CTR_LOOSE_S12] : 0); }

// Exclusive prefix of n counts, off[n] = total -- n is the number of exchange segments, a couple of hundred thousand: chunks of 1024
// scanned side by side (k_mex_scan_chunks), the chunk totals by one workgroup (k_mex_scan_parts), the bases added (k_mex_scan_add).
// (One workgroup walking all of it took 0.15 ms, a third of a rank's packing at N = 8.)  `part` holds n / 1024 + 2 values.
__global__ __launch_bounds__(1024) void k_mex_scan_chunks(const uint32_t *cnt, uint64_t n, uint32_t cap1, uint64_t *off, uint64_t *part)
{
    __shared__ uint64_t wsum[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    const uint64_t v = i < n ? (uint64_t)min(cnt[i], cap1) : 0ull;
    const uint64_t incl = wave_incl_scan(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    const uint64_t before = waves_before(wsum, wave);
    if (i < n) off[i] = before + incl - v;
    if (threadIdx.x == 1023) part[blockIdx.x] = before + incl;
}

__global__ __launch_bounds__(1024) void k_mex_scan_parts(uint64_t *part, uint64_t n_parts)
{
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry_sh;
    if (threadIdx.x == 0) carry_sh = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t first = 0; first < n_parts; first += 1024) {
        const uint64_t i = first + threadIdx.x;
        const uint64_t v = i < n_parts ? part[i] : 0ull;
        const uint64_t incl = wave_incl_scan(v);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        const uint64_t before = waves_before(wsum, wave, (uint64_t)carry_sh);
        if (i < n_parts) part[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_sh = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) part[n_parts] = carry_sh;
}

__global__ __launch_bounds__(1024) void k_mex_scan_add(uint64_t *off, uint64_t n, const uint64_t *part, uint64_t n_parts)
{
    const uint64_t i = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    if (i < n) off[i] += part[blockIdx.x];
    if (i == 0) off[n] = part[n_parts];
}

static inline size_t mex_scan_bytes(uint64_t n) { return kv_round_up((n + 1 + n / 1024 + 3) * 8, 256); }     // off[n + 1] and the chunk totals behind it
static void mex_scan_launch(const uint32_t *cnt, uint64_t n, uint32_t cap1, uint64_t *off, hipStream_t st)
{
    const uint64_t n_parts = (n + 1023) / 1024;
    uint64_t *part = off + n + 1;
    if (n_parts) hipLaunchKernelGGL(k_mex_scan_chunks, dim3((unsigned)n_parts), dim3(1024), 0, st, cnt, n, cap1, off, part);
    hipLaunchKernelGGL(k_mex_scan_parts, dim3(1), dim3(1024), 0, st, part, n_parts);
    hipLaunchKernelGGL(k_mex_scan_add, dim3((unsigned)std::max<uint64_t>(n_parts, 1)), dim3(1024), 0, st, off, n, (const uint64_t *)part, n_parts);
}

// the filled part of every segment, one after the other: a wavefront per segment (a segment of a shard at N = 8 holds ~40 records)
__global__ __launch_bounds__(256) void k_mex_gather(const uint64_t *seg, const uint32_t *cnt, const uint64_t *off, uint64_t n_segments, uint32_t cap1,
                                                    uint32_t recw, uint64_t *out, uint64_t out_cap_records)
{
    if (off[n_segments] > out_cap_records) return;            // does not fit: nothing is written, the caller sees the total and packs into a bigger buffer
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t sgi = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); sgi < n_segments; sgi += (uint64_t)gridDim.x * 4u) {
        const uint64_t words = (uint64_t)min(cnt[sgi], cap1) * recw;
        const uint64_t *src = seg + sgi * cap1 * recw;
        uint64_t *dst = out + off[sgi] * recw;
        for (uint64_t i = lane; i < words; i += 64) dst[i] = src[i];
    }
}

// k-dependent part of the geometry
void skm_geom_k(SkmGeom &g, int k)
{
    memset(&g, 0, sizeof(g));
    g.k = k;
    g.m = skm_minimizer_len(k);
    g.w = k - g.m + 1;
    g.wpow = 1;
    while (g.wpow * 2 <= g.w) g.wpow *= 2;
    g.kw = k <= 32 ? 1 : 2;
    g.nbw = g.kw + 1;
    g.recw = 1 + g.nbw;
    g.lrecw = g.recw;
    g.ncap = 32 * g.nbw - k + 1;
    g.sbw = skm_sbw(g.ncap);
    g.bpt = SKM_BUCKETS_PER_TICKET;
}

__global__ void k_mex_sum_kmers(const uint64_t *seg, const uint32_t *cnt, const uint64_t *off, uint64_t n_segments, uint32_t cap1, uint32_t recw,
                                unsigned long long *out)
{
    unsigned long long mine = 0;
    for (uint64_t sgi = blockIdx.x; sgi < n_segments; sgi += gridDim.x) {
        const uint32_t n = min(cnt[sgi], cap1);
        const uint64_t first = off ? off[sgi] : sgi * cap1;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) mine += recw == 2u ? skm_c_n(seg[(first + i) * 2u + 1u]) : skm_hdr_n(seg[(first + i) * recw]);
    }
    mine = wave_sum_u64(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

// cut `reads` into super-k-mers and bucket them (S1 + S2); idx.mu held by the caller
// distinct_frac: the share of distinct k-mers the caller expects (0: sequencing coverage of a whole sample, ~0.3)
int skm_build(SkmIndex &idx, const kv_reads *reads, int k, uint64_t n_kmers, hipStream_t st, double distinct_frac = 0.0, bool want_pos = true)
{
    SkmGeom &g = idx.g;
    idx.drop(SkmIndex::ALL);
    idx.builds += 1;
    skm_geom_k(g, k);
    g.force_loose = kv_knob("KV_SKM_FORCE_LOOSE") ? 1u : 0u;
    const uint32_t table_slots = g.kw == 1 ? 4096u : 2048u;
    const char *tgt_env = kv_knob("KV_SKM_BUCKET_KMERS");      // tests shrink the buckets to exercise many of them on small inputs
    // k-mers per fine bucket: as many as leave the LDS table ~0.4 full (0.29 for two-word keys, whose longer windows put
    // fewer, bigger minimizer loci into a bucket: more variance) given the share of distinct k-mers the previous batch
    // into the same sketch -- or routed on the same stream -- showed; without one, a whole 30x sample is assumed
    // (~0.2 distinct).  Fuller tables overflow in the larger buckets: 34 % distinct k-mers in 8192-k-mer buckets (a
    // quarter of a 30x sample per batch) put 2.1 % of the occurrences on the slow path.
    const double frac = std::min(1.0, std::max(0.05, distinct_frac > 0.0 ? distinct_frac : 0.2));
    // (two-word keys at 0.35: 2.2 M occurrences per 30x sample missed the tables and took the spill path, 67 ms per step of config 5; 0.29: 62 ms)
    uint64_t target = (uint64_t)((g.kw == 1 ? 0.4 : 0.29) * table_slots / frac);
    target = std::max<uint64_t>(table_slots / 2, std::min<uint64_t>(target, g.kw == 1 ? 2ull * table_slots : table_slots + table_slots / 2));
    if (tgt_env) target = std::max<uint64_t>(64, strtoull(tgt_env, nullptr, 10));
    uint64_t nfine = std::max<uint64_t>(1, (n_kmers + target - 1) / target);
    {
        // samples of one family are about the same size but not exactly: a batch whose own bucket count lies within a
        // quarter of the previous build's takes that one, so that the buckets of the controls and of the case sample
        // are the same buckets (the scan can then use the controls' abundance lists, KvAbundList)
        std::lock_guard<std::mutex> glk(g_skm_mu);
        if (g_skm_pref_k == k && g_skm_pref_nfine && nfine * 4 >= g_skm_pref_nfine * 3 && nfine * 4 <= g_skm_pref_nfine * 5) nfine = g_skm_pref_nfine;
        else { g_skm_pref_k = k; g_skm_pref_nfine = nfine; }
    }
    skm_bucket_grid(nfine, &g.C1, &g.F2, &g.fbits);
    g.n_buckets = g.C1 * g.F2;
    // 16-byte records without positions (kv_skm_device.h) when nobody will ask where a k-mer was: the count of a sample that is not
    // scanned from this very batch.  The lane-per-read S1 writes them, the sorted S2 moves them, k_skm_count reads them
    const char *s2 = kv_knob("KV_SKM_S2");
    if (!want_pos && g.kw == 1 && k + 1 <= SKM_C_BASES && skm_lane_fits(g, reads) && g.F2 <= SKM_S2_MAXF && !(s2 && strcmp(s2, "sorted") != 0)) skm_make_compact(g);
    const int cus = kv_device_cus();
    // at least one whole ticket per workgroup: the per-writer capacities below assume even shares
    g.nwg1 = (uint32_t)std::min<uint64_t>((std::max<uint32_t>(reads->n_tiles, 1u) + SKM_TILES_PER_TICKET - 1) / SKM_TILES_PER_TICKET,
                                          std::min<uint32_t>(768u, 3u * (uint32_t)cus));
    // (the w = 40 lane kernel, and reads whose LDS slices fit a CU only twice: two workgroups per CU)
    if (skm_lane_fits(g, reads) && (g.w == 2 * SKM_LANE_B || skm_lane_wgs_per_cu(reads->uni_len) < 3u)) g.nwg1 = std::min<uint32_t>(g.nwg1, 2u * (uint32_t)cus);
    {
        // the wave kernel with 1024-thread workgroups runs one workgroup per CU (fewer writers: see k_skm_emit_wave)
        int ch_unused = 16;
        if (skm_wave_threads() == 1024 && skm_wave_plan(g, reads, &ch_unused)) g.nwg1 = std::min<uint32_t>(g.nwg1, (uint32_t)cus);
    }
    const uint64_t avg1 = (reads->n_tiles + g.nwg1 - 1) / g.nwg1;
    g.quota1 = (uint32_t)std::min<uint64_t>(kv_round_up(avg1 + avg1 / 2 + 1, SKM_TILES_PER_TICKET), 0xfffffff0ull);
    g.nwg2 = std::max<uint32_t>(1u, std::min<uint32_t>(16u, 1024u / g.C1));
    g.nwg2 = std::min<uint32_t>(g.nwg2, g.nwg1);
    g.np_max = std::max<uint32_t>(reads->tile_max_bases, 64u);
    g.stride = reads->max_len >= (uint32_t)k ? reads->max_len - (uint32_t)k + 1 : 1;
    const double rec_est = skm_rec_est(n_kmers, (double)reads->n_reads, g.w);
    g.cap1 = skm_seg_cap(rec_est / ((double)g.C1 * g.nwg1), 1.5, 64);
    g.cap2 = skm_seg_cap(rec_est / ((double)g.n_buckets * g.nwg2), 1.3, 32);
    g.loose_cap = skm_loose_cap(rec_est, n_kmers);
    if (const char *pct = kv_knob("KV_SKM_CAP_PCT")) {       // tests: undersized segments push records through the loose list
        g.cap1 = std::max<uint32_t>(16u, (uint32_t)((uint64_t)g.cap1 * (uint64_t)atoi(pct) / 100));
        g.cap2 = std::max<uint32_t>(16u, (uint32_t)((uint64_t)g.cap2 * (uint64_t)atoi(pct) / 100));
    }
    if (const char *lc = kv_knob("KV_SKM_LOOSE_CAP")) g.loose_cap = strtoull(lc, nullptr, 10);
    const size_t rb = (size_t)g.recw * 8, b_ctr = 256;
    auto lay = [&](SkmCarve c) {
        g.seg1 = c.take<uint64_t>((uint64_t)g.C1 * g.nwg1 * g.cap1 * rb);
        g.cnt1 = c.take<uint32_t>((uint64_t)g.C1 * g.nwg1 * 4);
        g.seg2 = c.take<uint64_t>((uint64_t)g.n_buckets * g.nwg2 * g.cap2 * rb);
        g.cnt2 = c.take<uint32_t>((uint64_t)g.n_buckets * g.nwg2 * 4);
        g.loose = c.take<uint64_t>(g.loose_cap * (size_t)g.lrecw * 8);
        g.ctr = c.take<unsigned long long>(b_ctr);
        return c.total;
    };
    const size_t b_all = lay(SkmCarve());
    // (no memory for the buckets -- three samples cut side by side in batches of tens of millions of reads -- is a CAPACITY answer: the batch
    // takes the plain partition, or the tile scan, as it does when a buffer runs over)
    if (idx.arena.need(b_all) != hipSuccess) {
        (void)hipGetLastError();
        kv_set_error("no device memory for the super-k-mer buckets (%.1f GB)", (double)b_all / 1e9);
        return KV_ERR_CAPACITY;
    }
    lay(SkmCarve(idx.arena.p));
    g.seg1_wmajor = 1u;
    KV_HIP(hipMemsetAsync(g.ctr, 0, b_ctr, st));
    g.bucket_kmers = std::max<uint64_t>(1, n_kmers / g.n_buckets);
    skm_launch_emit(g, reads, st);
    skm_launch_split(g, st);
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(&g.ctr[SKM_CTR_LOOSE_S12], &g.ctr[SKM_CTR_LOOSE], 8, hipMemcpyDeviceToDevice, st));   // loose records S1/S2 left behind
    skm_plan_tickets(g);
    idx.reads_uid = reads->uid;
    idx.k = k;
    idx.valid = true;
    return KV_OK;
}

}  // namespace

// can (and should) the super-k-mer front end take this batch?  -1 no; 0 yes if the sketch agrees; 1 yes, asked for by name
static int skm_fits(int hashfam, int ksize, const kv_reads *reads, uint64_t n_kmers, bool for_scan)
{
    const char *force = kv_knob(for_scan ? "KV_NOVEL_PATH" : "KV_COUNT_PATH");
    if (force && strcmp(force, "skm") != 0) return -1;        // another path was asked for by name
    if (hashfam != HF_MURMUR || ksize < SKM_MIN_K || ksize > SKM_MAX_K) return -1;
    if (reads->n_tiles == 0 || n_kmers == 0) return -1;
    const uint64_t min_stride = reads->max_len >= (uint32_t)ksize ? reads->max_len - (uint32_t)ksize + 1 : 1;
    if ((double)reads->n_reads * (double)min_stride >= (double)(1ull << SKM_POS_BITS)) return -1;
    if (reads->tile_max_bases == 0 || reads->tile_max_bases > 8192u) return -1;
    if (force) return 1;
    return n_kmers >= (1ull << 22) ? 0 : -1;
}

bool kv_skm_eligible(const kv_sketch *s, const kv_reads *reads, uint64_t n_kmers, bool for_scan)
{
    const int fits = skm_fits(s->h.hashfam, s->h.ksize, reads, n_kmers, for_scan);
    // skm_off: the previous batch into this sketch did not deduplicate (kv_consume_skm); skm_off_kmers: nor did a batch of this size
    // before the sketch was cleared (within a tenth)
    const bool same_shape = !for_scan && s->skm_off_kmers != 0 && n_kmers * 10 >= s->skm_off_kmers * 9 && n_kmers * 10 <= s->skm_off_kmers * 11;
    return fits > 0 || (fits == 0 && !s->skm_off && !same_shape);
}

bool kv_skm_eligible_kind(int hashfam, int ksize, const kv_reads *reads, uint64_t n_kmers, bool for_scan)
{
    return skm_fits(hashfam, ksize, reads, n_kmers, for_scan) >= 0;
}

int kv_consume_skm(kv_sketch *s, const kv_reads *reads, const ConsumeFilter &filter, const kv_sketch *mask,
                   uint64_t n_kmers, int nbands, uint64_t *n_added)
{
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    const int k = s->h.ksize;
    // (a sketch with the scan hint keeps positions: the scan that follows marks occurrences from these very buckets)
    // no memory for the buckets, or for the staging of the bin stages beside them (three samples cut side by side in batches of tens of
    // millions of reads): the batch takes the plain partition, this sketch does not ask again -- nor after a clear, for a batch of this
    // size -- and what the attempt holds goes back at once so that the plain partition finds room for its own staging
    auto no_memory = [&](int rc) {
        s->skm_off = true;
        s->skm_off_kmers = n_kmers;
        idx.give_back();
        if (kv_knob("KV_SKM_VERBOSE")) fprintf(stderr, "[kv_skm] no memory for the bucketed count of this batch: the plain partition, and the stream's bucket buffers are given back\n");
        return rc;
    };
    {
        const int rc = skm_build(idx, reads, k, n_kmers, st, s->skm_distinct, s->scan_hint != 0);
        if (rc == KV_ERR_CAPACITY) return no_memory(rc);
        if (rc != KV_OK) return rc;
    }
    SkmGeom &sg = idx.g;
    const uint32_t nwg3 = skm_nwg3(sg);
    BinPlan plan;
    // the bin stages receive one item per DISTINCT k-mer and table: their buffers are sized for 60 % of the k-mers being
    // distinct (sequencing coverage leaves 20-35 %); a batch with more spills over, raises the flag, and is redone by
    // the one-item-per-k-mer partition -- which is where a batch that does not deduplicate belongs anyway
    const uint64_t n_items = std::max<uint64_t>(n_kmers * 3 / 5, std::min<uint64_t>(n_kmers, 1u << 22));
    {
        const int rc = kv_bin_plan(s, n_items, nbands, filter.use_mask != 0, sg.n_buckets, 0u, nwg3, true, &plan);
        if (rc == KV_ERR_CAPACITY) return no_memory(rc);
        if (rc != KV_OK) return rc;
    }
    const SketchDev *d_mask = mask ? mask->d_desc : nullptr;
    // abundance list of this batch (KvAbundList): the first super-k-mer count after a clear writes one
    bool abl_new = false;
    {
        KvAbundList &al = s->abl;
        if (!al.valid && !s->scan_hint) {            // (a case sample's list would never be asked for: it is scanned, not scanned against)
            const uint64_t cap_total = std::min<uint64_t>(std::max<uint64_t>(n_kmers / 8, 1u << 16), 0xfffffff0ull);
            const uint64_t cap_wg = std::max<uint64_t>(64, cap_total / nwg3);
            const size_t need = skm_list_lay(SkmCarve(), cap_wg * nwg3, sg.kw, sg.n_buckets, &al.keys, &al.cnts, &al.bstart, &al.bcount);
            if (al.bytes < need) {
                if (al.mem) (void)hipFree(al.mem);
                al.mem = nullptr; al.bytes = 0;
                if (kv_hip_malloc(&al.mem, need) == hipSuccess) al.bytes = need;
                else (void)hipGetLastError();              // no room: no list, nothing else changes
            }
            if (al.mem) {
                skm_list_lay(SkmCarve(al.mem), cap_wg * nwg3, sg.kw, sg.n_buckets, &al.keys, &al.cnts, &al.bstart, &al.bcount);
                KV_HIP(skm_list_zero(al.bstart, al.bcount, st));
                al.k = k; al.m = sg.m; al.kw = sg.kw; al.C1 = sg.C1; al.F2 = sg.F2; al.fbits = sg.fbits; al.n_buckets = sg.n_buckets;
                al.nwg = nwg3; al.cap_wg = cap_wg; al.cap_total = cap_wg * nwg3;
                skm_abl_attach(al, sg);
                abl_new = true;
            }
        }
    }
    // distinct list (kv_sketch_scan_hint): the batch is a case sample's and will be scanned next.  A workgroup takes up to
    // quota3 of the buckets, so its stretch holds one and a half average shares of the distinct k-mers the batch is expected
    // to have (what the previous batch showed, or 30 %); a stretch that runs out drops the list (SKM_CTR_DL_RAN_OUT), nothing else.
    // The first batch a stream ever buckets gets no list unless the room is there already: allocating a gigabyte or two costs
    // tens of milliseconds, more than the list saves once -- a one-shot `kevlar novel` is exactly that case -- while a process
    // that counts and scans sample after sample pays it once (KV_SKM_DL=1: always, =0: never).
    bool dl_new = false;
    const char *dl_env = kv_knob("KV_SKM_DL");
    if (s->scan_hint && !(dl_env && atoi(dl_env) == 0)) {
        const double frac = std::min(1.0, std::max(0.3, s->skm_distinct * 1.15));
        const uint64_t cap_wg = std::min<uint64_t>((uint64_t)((double)n_kmers * frac * 1.6 / nwg3) + 4096, 0xfffffff0ull / nwg3);
        const bool worth = (dl_env && atoi(dl_env) == 1) || s->scan_steady || idx.builds > 1 || idx.dl.bytes >= SkmDistinctList::bytes(cap_wg * nwg3, sg.kw, sg.n_buckets);
        const int lrc = worth ? idx.list.carve(idx.dl, cap_wg * nwg3, sg.kw, sg.n_buckets, (uint32_t)cap_wg, 0, 0, st) : KV_ERR_CAPACITY;
        if (lrc != KV_OK && lrc != KV_ERR_CAPACITY) return lrc;
        if (lrc == KV_OK) { idx.list.attach(sg); dl_new = true; }
        else (void)hipGetLastError();                   // no room: no list
    }
    {
        KvProfScope prof("k_skm_count");
        const uint32_t ns = (uint32_t)(plan.g.T * plan.g.C);
        // the fixed-k instances count a key's occurrences in 16 bits (k_skm_count, PL): only for buckets that cannot hold 65536 of them
        const bool fixed_k = !sg.force_loose && !kv_knob("KV_SKM_ANY_K") && (uint64_t)sg.nwg2 * sg.cap2 * (uint64_t)sg.ncap < 65536ull;
        auto kernel = sg.kw == 1 ? (sg.force_loose ? SKM_INST(k_skm_count<1, 4096, true, 0>) : SKM_INST(k_skm_count<1, 4096, false, 0>))
                                 : (sg.force_loose ? SKM_INST(k_skm_count<2, 2048, true, 0>) : SKM_INST(k_skm_count<2, 2048, false, 0>));
        bool pl = false;         // a fixed-k instance: 4 KB of product tables where the others keep 1 KB of ASCII
        if (sg.k == 31 && sg.recw == 3 && fixed_k) { kernel = SKM_INST(k_skm_count<1, SKM_TS31, false, 31>); pl = true; }
        if (sg.compact) {       // 16-byte records (sg.recw == 2): their own instances
            kernel = sg.force_loose ? SKM_INST(k_skm_count<1, 4096, true, 0, true>) : SKM_INST(k_skm_count<1, 4096, false, 0, true>);
            pl = false;
            if (sg.k == 31 && fixed_k) { kernel = SKM_INST(k_skm_count<1, SKM_TS31, false, 31, true>); pl = true; }
        }
        // (BASELINE.json configs[4]: k = 51 -- two-word keys, three murmur blocks + a 3-byte tail)
        if (sg.k == 51 && sg.recw == 4 && fixed_k) { kernel = SKM_INST(k_skm_count<2, SKM_TS51, false, 51>); pl = true; }
        const size_t lds = ((pl ? 1024 : 256) + ((ns + 3u) & ~3u) + (size_t)(SKM_THREADS3 / 64) * skm_wave_scratch_words(sg.sbw)) * 4;
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(nwg3), dim3(SKM_THREADS3), lds, st, sg, (const SketchDev *)s->d_desc, d_mask, filter, plan.g);
    }
    {
        KvProfScope prof("k_skm_loose_count");
        skm_launch_loose(SKM_INST(k_skm_loose_count<1>), SKM_INST(k_skm_loose_count<2>), st, sg, s->d_desc, d_mask, filter, plan.g);
    }
    KV_HIP(hipGetLastError());
    // a lost record (loose list overflow) must stop the apply stage, which looks at the partition's own flag
    hipLaunchKernelGGL(k_skm_forward_flag, dim3(1), dim3(1), 0, st, sg.ctr, plan.g.ctr);
    KV_HIP(hipGetLastError());
    skm_abl_detach(sg);
    SkmDistinctList::detach(sg);
    const int rc = kv_bin_finish(s, plan, true, 0, n_added);     // synchronises the stream
    if (abl_new) s->abl.valid = rc == KV_OK;
    {
        // what the batch looked like: if most k-mers are distinct (low coverage per batch) cutting and bucketing the
        // reads buys nothing, and if many occurrences missed the LDS tables the buckets were too full; either way
        // the next batches into this sketch take the one-item-per-k-mer partition (until the sketch is cleared)
        unsigned long long sc[SKM_CTR_DL_RAN_OUT + 1] = {0};
        const bool got = hipMemcpy(sc, sg.ctr, sizeof(sc), hipMemcpyDeviceToHost) == hipSuccess;
        idx.dl_valid = dl_new && got && rc == KV_OK && sc[SKM_CTR_DL_RAN_OUT] == 0;
        if (dl_new && kv_knob("KV_SKM_VERBOSE")) fprintf(stderr, "[kv_skm] distinct list: %s (%llu workgroups ran out of %u entries)\n", idx.dl_valid ? "kept" : "dropped", sc[SKM_CTR_DL_RAN_OUT], idx.list.cap_wg);
        if (got && n_kmers) {
            const double alone = skm_outside_tables(sc) / (double)n_kmers;
            const double distinct = (double)sc[SKM_CTR_DISTINCT] / (double)n_kmers + alone;
            s->skm_off = rc != KV_OK || alone > 0.03 || distinct > 0.45;
            // (what the batch itself showed -- or buffers sized for sequencing coverage running over, which is how a batch without repeats ends:
            // its figures are then those of an aborted count -- not an error of another kind)
            s->skm_off_kmers = (distinct > 0.45 || rc == KV_ERR_CAPACITY) ? n_kmers : 0;
            s->skm_distinct = distinct;
            { std::lock_guard<std::mutex> glk(g_skm_mu); g_skm_last_distinct = distinct; }
            if (kv_knob("KV_SKM_VERBOSE"))
                fprintf(stderr, "[kv_skm] batch of %llu k-mers: %.1f%% distinct, %.2f%% outside the LDS tables, %llu of %llu records (%d bytes each) outside their segments%s\n",
                        (unsigned long long)n_kmers, 100 * distinct, 100 * alone, sc[SKM_CTR_LOOSE_S12], sc[SKM_CTR_RECORDS], 8 * sg.recw,
                        s->skm_off ? " -> next batches take the plain partition" : "");
        }
    }
    if (rc != KV_OK) {
        idx.drop(SkmIndex::BATCH | SkmIndex::MEX_SCAN);
        if (kv_knob("KV_SKM_VERBOSE")) {
            unsigned long long sc[SKM_CTR_DISTINCT + 1] = {0}, bc[4] = {0};
            (void)hipMemcpy(sc, sg.ctr, sizeof(sc), hipMemcpyDeviceToHost);
            (void)hipMemcpy(bc, plan.g.ctr, sizeof(bc), hipMemcpyDeviceToHost);
            fprintf(stderr, "[kv_skm] count fell back: rc %d, loose %llu of %llu (flag %llu), records %llu, spill %llu of %llu (flag %llu); C1 %u F2 %u nwg1 %u nwg2 %u cap1 %u cap2 %u\n",
                    rc, sc[SKM_CTR_LOOSE], (unsigned long long)sg.loose_cap, sc[SKM_CTR_FAIL], sc[SKM_CTR_RECORDS], bc[0], (unsigned long long)plan.g.spill_cap, bc[1],
                    sg.C1, sg.F2, sg.nwg1, sg.nwg2, sg.cap1, sg.cap2);
        }
    }
    if (s->skm_off && idx.arena.bytes + idx.dl.bytes >= ((size_t)1 << 30)) {
        // The batches of this sketch will not come this way again, and what was bucketed here is of no use to a scan of a batch with
        // nothing to combine: the gigabytes the attempt took (records twice over with their slack: 30 GB per stream for a 37.5 M-read
        // batch of config 4, which is what kept batches of twice the size from fitting beside the resident reads) go back now instead of
        // waiting for kv_scratch_trim.
        idx.give_back();
        if (kv_knob("KV_SKM_VERBOSE")) fprintf(stderr, "[kv_skm] the stream's bucket buffers are given back\n");
    }
    return rc;
}

// bits[w] bit j = (table[32 w + j] >= case_min) for a table of byte counters (k_case_bits): the first probe of a scan as a bit map
void kv_case_bits_launch(const uint8_t *d_table, uint64_t size, int case_min, uint32_t *d_bits, hipStream_t st)
{
    KvProfScope prof("k_case_bits");
    hipLaunchKernelGGL(k_case_bits, dim3(4096), dim3(256), 0, st, d_table, size, case_min, d_bits);
}

void kv_tile_hits_launch(const kv_reads *reads, const NovelParams &p, hipStream_t st)
{
    KvProfScope prof("k_tile_hits");
    hipLaunchKernelGGL(k_tile_hits, dim3(reads->n_tiles), dim3(64), 0, st, reads_dev(reads), p);
}

bool kv_skm_list_ready(const kv_reads *reads, int ksize)
{
    if (kv_knob("KV_SKM_NO_REUSE") || (kv_knob("KV_SKM_DL") && atoi(kv_knob("KV_SKM_DL")) == 0)) return false;
    std::lock_guard<std::mutex> lk(g_skm_mu);
    for (auto &kv : g_skm)
        if (kv.second.valid && kv.second.dl_valid && kv.second.reads_uid == reads->uid && kv.second.k == ksize) return true;
    return false;
}

int kv_skm_novel_mark(const kv_reads *reads, const NovelParams &p, uint64_t n_kmers)
{
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    const int k = p.hp.k;
    // the bucketed batch may sit in the arena of whichever stream counted it
    SkmIndex *idx = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_skm_mu);
        for (auto &kv : g_skm)
            if (kv.second.valid && kv.second.reads_uid == reads->uid && kv.second.k == k) { idx = &kv.second; break; }
        if (!idx) idx = &g_skm[kv_stream_key(st)];
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    const bool reuse = idx->valid && idx->reads_uid == reads->uid && idx->k == k && !idx->g.compact && !kv_knob("KV_SKM_NO_REUSE");
    if (!reuse) {
        double hint;
        { std::lock_guard<std::mutex> glk(g_skm_mu); hint = g_skm_last_distinct; }
        const int rc = skm_build(*idx, reads, k, n_kmers, st, hint);
        if (rc != KV_OK) return rc;
    }
    SkmGeom &sg = idx->g;
    // the count pass of this very batch left key + hash of every distinct k-mer (kv_sketch_scan_hint): scan from that list
    const bool from_list = reuse && idx->dl_valid && !p.set_keys && !(kv_knob("KV_SKM_DL") && atoi(kv_knob("KV_SKM_DL")) == 0);
    if (reuse) {
        // records that did not fit their S1/S2 segment are the first SKM_CTR_LOOSE_S12 entries of the loose list; the entries the
        // count pass added behind them (single occurrences that missed its LDS tables) are re-created by the scan's
        // own pass 0, so the list is cut back to what S1/S2 left -- unless the scan goes by the distinct list, which does
        // not hold those k-mers: then they stay, and k_skm_loose_novel evaluates them
        if (!from_list) KV_HIP(hipMemcpyAsync(&sg.ctr[SKM_CTR_LOOSE], &sg.ctr[SKM_CTR_LOOSE_S12], 8, hipMemcpyDeviceToDevice, st));
        KV_HIP(hipMemsetAsync(&sg.ctr[SKM_CTR_TICKET_SCAN], 0, 8, st));
    }
    const uint32_t nwg3 = skm_nwg3(sg);
    const ReadsDev rd = reads_dev(reads);
    SkmAblSet abls;
    memset(&abls, 0, sizeof(abls));
    abls.ctrl_max = p.ctrl_max;
    if (p.host_ctrls && !p.set_keys) {
        const kv_sketch *const *ctrls = (const kv_sketch *const *)p.host_ctrls;
        for (int c = 0; c < p.host_nctrl && abls.n < SKM_MAX_ABL; ++c) {
            const KvAbundList &al = ctrls[c]->abl;
            if (!al.valid || al.k != k || al.m != sg.m || al.C1 != sg.C1 || al.F2 != sg.F2 || al.n_buckets != sg.n_buckets) continue;
            const int a = abls.n++;
            abls.keys[a] = al.keys; abls.cnts[a] = al.cnts; abls.bstart[a] = al.bstart; abls.bcount[a] = al.bcount;
            abls.maxv[a] = ctrls[c]->h.storage == ST_BYTE ? 255u : (ctrls[c]->h.storage == ST_NIBBLE ? 15u : 1u);
        }
    }
    if (kv_knob("KV_SKM_VERBOSE")) fprintf(stderr, "[kv_skm] scan: %d of %d controls bring an abundance list in this bucket geometry\n", abls.n, p.host_nctrl);
    if (kv_knob("KV_SKM_VERBOSE")) fprintf(stderr, "[kv_skm] scan: %s\n", from_list ? "from the count pass's distinct list" : "by walking the buckets");
    NovelParams pl = p;
    pl.case0_bits = nullptr;
    // (KV_NOVEL_BITS=0: probe the table.  Measured at config 2: the bit map costs 0.135 ms, the list scan goes from 2.57-2.77 to 2.34 ms)
    if (from_list && p.host_case0 && !(kv_knob("KV_NOVEL_BITS") && atoi(kv_knob("KV_NOVEL_BITS")) == 0)) {
        const kv_sketch *c0 = (const kv_sketch *)p.host_case0;
        if (c0->h.storage == ST_BYTE && !c0->lazy_zero && idx->bits.need(kv_round_up(((c0->h.size[0] + 31) >> 5) * 4, 256)) == hipSuccess) {
            kv_case_bits_launch((const uint8_t *)c0->h.tab[0], (uint64_t)c0->h.size[0], p.case_min, (uint32_t *)idx->bits.p, st);
            pl.case0_bits = (const uint32_t *)idx->bits.p;
        } else {
            (void)hipGetLastError();
        }
    }
    if (from_list) {
        KvProfScope prof("k_skm_novel_list");
        idx->list.attach(sg);
        const size_t lds = (size_t)(SKM_THREADS3 / 64) * skm_wave_scratch_words(sg.sbw) * 4;
        const auto kernel = sg.kw == 1 ? SKM_INST(k_skm_novel_list<1, 2048>) : SKM_INST(k_skm_novel_list<2, 1024>);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(nwg3), dim3(SKM_THREADS3), lds, st, sg, rd, pl, abls);
        if (p.ab_keys) hipLaunchKernelGGL(k_ab_fill, dim3(2048), dim3(256), 0, st, p);
        if (p.ab_list && kv_knob("KV_SKM_VERBOSE")) {
            unsigned int claimed = 0;
            if (hipMemcpyAsync(&claimed, p.ab_count, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
                fprintf(stderr, "[kv_skm] scan: %u interesting k-mers hold a slot for their abundances (the list takes %u)\n", claimed, p.ab_list_cap);
        }
        SkmDistinctList::detach(sg);
    } else {
        KvProfScope prof("k_skm_novel");
        const size_t lds = (256 + (size_t)(SKM_THREADS3 / 64) * skm_wave_scratch_words(sg.sbw)) * 4;
        const auto kernel = sg.kw == 1 ? SKM_INST(k_skm_novel<1, 4096>) : SKM_INST(k_skm_novel<2, 2048>);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(nwg3), dim3(SKM_THREADS3), lds, st, sg, rd, p, abls);
    }
    {
        KvProfScope prof("k_skm_loose_novel");
        skm_launch_loose(SKM_INST(k_skm_loose_novel<1>), SKM_INST(k_skm_loose_novel<2>), st, sg, rd, p);
    }
    kv_tile_hits_launch(reads, p, st);
    KV_HIP(hipGetLastError());
    unsigned long long sctr[SKM_CTR_FAIL + 1] = {0, 0};
    KV_HIP(hipMemcpyAsync(sctr, sg.ctr, sizeof(sctr), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    idx->drop(SkmIndex::BATCH | SkmIndex::LIST);     // one scan per build: the loose list now holds this scan's entries
    if (sctr[SKM_CTR_FAIL] != 0) {
        kv_set_error("super-k-mer scan: loose record list overflow (%llu records)", sctr[SKM_CTR_LOOSE]);
        return KV_ERR_CAPACITY;
    }
    return KV_OK;
}

static void skm_launch_route(KvInst<void(SkmGeom, HashParams, KvRouteSink)> kernel, const SkmGeom &g, int k, const KvRouteSink &rs, hipStream_t st);

int kv_skm_route_distinct(const kv_reads *reads, int ksize, uint64_t n_kmers, int ndest,
                          int (*alloc)(void *ctx, uint32_t nwg, KvRouteSink *sink), void *ctx)
{
    KV_REQUIRE(ndest >= 1 && ndest <= SKM_ROUTE_MAX_DEST, KV_ERR_ARG, "kv_skm_route_distinct: 1..%d destinations", SKM_ROUTE_MAX_DEST);
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    { const int rc = skm_build(idx, reads, ksize, n_kmers, st, idx.distinct_hint); if (rc != KV_OK) return rc; }
    SkmGeom &sg = idx.g;
    const uint32_t nwg3 = skm_nwg3(sg);
    KvRouteSink rs;
    memset(&rs, 0, sizeof(rs));
    { const int rc = alloc(ctx, nwg3, &rs); if (rc != KV_OK) return rc; }
    skm_launch_route(sg.kw == 1 ? SKM_INST(k_skm_route<1, 4096>) : SKM_INST(k_skm_route<2, 2048>), sg, ksize, rs, st);
    KV_HIP(hipGetLastError());
    unsigned long long sctr[SKM_CTR_DISTINCT + 1] = {0};
    KV_HIP(hipMemcpyAsync(sctr, sg.ctr, sizeof(sctr), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    // the next shard routed on this stream (same sample or a sibling: same coverage) gets buckets sized for what this one held
    const double alone = skm_outside_tables(sctr) / (double)n_kmers;
    idx.distinct_hint = std::min(1.0, (double)sctr[SKM_CTR_DISTINCT] / (double)n_kmers + alone);
    if (kv_knob("KV_SKM_VERBOSE"))
        fprintf(stderr, "[kv_skm] routed %llu k-mers: %.1f%% distinct, %.2f%% outside the LDS tables, %u buckets\n",
                (unsigned long long)n_kmers, 100 * idx.distinct_hint, 100 * alone, sg.n_buckets);
    if (sctr[SKM_CTR_FAIL] != 0) {
        idx.drop(SkmIndex::BATCH | SkmIndex::MEX_SCAN);
        kv_set_error("super-k-mer route: loose record list overflow (%llu records)", sctr[SKM_CTR_LOOSE]);
        return KV_ERR_CAPACITY;
    }
    return KV_OK;
}

// the buckets' distinct k-mers through `kernel`, the instance of k_skm_route for the geometry, then the loose list's
static void skm_launch_route(KvInst<void(SkmGeom, HashParams, KvRouteSink)> kernel, const SkmGeom &g, int k, const KvRouteSink &rs, hipStream_t st)
{
    const HashParams hp = make_hash_params(k, HF_MURMUR);
    {
        KvProfScope prof("k_skm_route");
        const size_t lds = (256 + (size_t)(SKM_THREADS3 / 64) * skm_wave_scratch_words(g.sbw)) * 4;
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(skm_nwg3(g)), dim3(SKM_THREADS3), lds, st, g, hp, rs);
    }
    KvProfScope prof("k_skm_loose_route");
    skm_launch_loose(SKM_INST(k_skm_loose_route<1>), SKM_INST(k_skm_loose_route<2>), st, g, hp, rs);
}

// ---- minimizer-sharded exchange (kevlar_amd/shardrun.py) ------------------------------------------------
// N ranks each hold 1/N of a sample's reads.  Deduplicating a shard on its own finds little to combine at 1/8 of the
// coverage, so the shards are cut into super-k-mers first (S1, here), the RECORDS travel to the rank that owns their
// minimizer bucket -- every occurrence of a k-mer, from whichever shard, meets there -- and that rank combines them at the
// sample's full coverage (S2 + the distinct route below) before (hash, occurrences) pairs go on to the band owners.
int kv_skm_mex_plan(int ksize, uint64_t n_reads_global, uint32_t read_len, int ndest, kv_mex_plan *plan)
{
    KV_REQUIRE(plan && ndest >= 1 && ndest <= SKM_ROUTE_MAX_DEST && ksize >= SKM_MIN_K && ksize <= SKM_MAX_K && read_len >= (uint32_t)ksize,
               KV_ERR_ARG, "kv_mex_plan: k in %d..%d, 1..%d destinations, reads of at least k bases", SKM_MIN_K, SKM_MAX_K, SKM_ROUTE_MAX_DEST);
    memset(plan, 0, sizeof(*plan));
    SkmGeom g;
    skm_geom_k(g, ksize);
    const uint64_t nk_read = read_len - (uint32_t)ksize + 1u;
    const uint64_t n_kmers = n_reads_global * nk_read;
    const uint32_t table_slots = g.kw == 1 ? 4096u : 2048u;
    const uint64_t target = g.kw == 1 ? 2ull * table_slots : table_slots + table_slots / 2;       // a whole sample at sequencing coverage (~0.2 distinct)
    const uint64_t nfine = std::max<uint64_t>(1, (n_kmers + target - 1) / target);
    uint32_t C1, F2, fbits;
    skm_bucket_grid(nfine, &C1, &F2, &fbits);
    C1 = (uint32_t)kv_round_up(C1, (uint64_t)ndest);
    if (C1 > 255u) C1 = 255u / (uint32_t)ndest * (uint32_t)ndest;
    const uint64_t shard_reads = (n_reads_global + ndest - 1) / ndest;
    const uint64_t tiles = (shard_reads + KV_TILE_MAX_READS - 1) / KV_TILE_MAX_READS;
    // Writers per shard; every one owns a segment of every coarse bucket.  One per CU, 1024 threads each: a shard is an N-th of a
    // sample, and with the 768 writers of a whole sample its ~190 000 segments held ~40 records each at N = 8 -- the cut, the packing
    // and the owner's split all pay per segment (per rank of config 2, N = 8 / N = 2: 8.58 / 25.07 ms with 768 writers of 512 threads,
    // 7.73 / 23.10 with 256 of 1024).
    const uint64_t nwg1_max = 256;
    const uint32_t nwg1 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tiles + SKM_TILES_PER_TICKET - 1) / SKM_TILES_PER_TICKET, nwg1_max));
    const double rec_est = skm_rec_est(shard_reads * nk_read, (double)shard_reads, g.w);
    const uint32_t cap1 = skm_seg_cap(rec_est / ((double)C1 * nwg1), 2.0, 64);
    plan->ksize = ksize; plan->ndest = ndest; plan->C1 = C1; plan->F2 = F2; plan->fbits = fbits; plan->nwg1 = nwg1; plan->cap1 = cap1;
    plan->recw = (uint32_t)g.recw; plan->m = (uint32_t)g.m;
    plan->seg_words = (uint64_t)C1 * nwg1 * cap1 * g.recw;
    plan->cnt_entries = (uint64_t)C1 * nwg1;
    for (int d = 0; d <= ndest; ++d) plan->c_lo[d] = (uint32_t)((uint64_t)C1 * d / ndest);
    plan->n_kmers_global = n_kmers; plan->n_reads_global = n_reads_global; plan->read_len = read_len;
    return KV_OK;
}

// the plan with 16-byte records (compact: kv_skm_device.h): the lane-per-read S1 writes them, the sorted S2 moves them
int kv_skm_mex_plan_short(kv_mex_plan *plan)
{
    SkmGeom g;
    skm_geom_k(g, plan->ksize);
    // (the owner's S2 takes 16-byte records in either form: the sorted split up to 1024 fine buckets, the plain one up to 4096 -- the 12
    // bits the record has for its fine bucket)
    KV_REQUIRE(g.kw == 1 && g.w == SKM_LANE_B && skm_lane_fits_len(g, plan->read_len) &&
               plan->F2 <= 4096u,
               KV_ERR_NOTIMPL, "kv_mex_plan_short: no 16-byte records for k = %d, reads of %u bases, %u fine buckets", plan->ksize, plan->read_len, plan->F2);
    if (plan->flags & 1u) return KV_OK;
    plan->flags |= 1u;
    plan->seg_words = plan->seg_words / plan->recw * 2u;
    plan->recw = 2u;
    return KV_OK;
}
// what a plan fixes of the geometry, for C1 of its coarse buckets: all of them where a shard is cut, the owner's share where they are combined
static void skm_geom_plan(SkmGeom &g, const kv_mex_plan *plan, uint32_t C1)
{
    skm_geom_k(g, plan->ksize);
    if (plan->flags & 1u) skm_make_compact(g);
    g.C1 = C1; g.F2 = plan->F2; g.fbits = plan->fbits; g.n_buckets = C1 * g.F2;
    g.nwg1 = plan->nwg1; g.cap1 = plan->cap1; g.stride = plan->read_len - (uint32_t)plan->ksize + 1u;
}

// S1 of one shard into the caller's buffers ([C1][nwg1][cap1] records, [C1][nwg1] counts: what the plan says).
// d_out != NULL: the filled part of the segments is packed into it as well, destination after destination (kv_skm_mex_pack), if it
// holds out_cap_words; *packed says whether it did.  One stream synchronisation either way.
int kv_skm_mex_emit(const kv_reads *reads, const kv_mex_plan *plan, uint64_t read_base, uint64_t *d_seg, uint32_t *d_cnt,
                    uint64_t *d_out, uint64_t out_cap_words, uint64_t *records_per_dest, int *packed)
{
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    idx.drop(SkmIndex::BATCH | SkmIndex::MEX_SCAN);
    SkmGeom &g = idx.g;
    skm_geom_plan(g, plan, plan->C1);
    g.quota1 = 0xfffffff0u;                                   // tiles are dealt dynamically; the plan's capacity has the slack
    g.np_max = std::max<uint32_t>(reads->tile_max_bases, 64u);
    KV_REQUIRE(reads->max_len <= plan->read_len, KV_ERR_ARG, "kv_mex_emit: a read of %u bases in a plan for %u", reads->max_len, plan->read_len);
    // (a rank whose shard holds no read -- fewer reads than ranks -- still takes part: it sends empty segments)
    KV_REQUIRE(reads->n_tiles == 0 || (reads->tile_max_bases > 0 && reads->tile_max_bases <= 8192u), KV_ERR_ARG, "kv_mex_emit: reads too long for the super-k-mer front end");
    g.read_base = read_base;
    // (the exchange's records are oriented like a single GPU's: every rank cuts with the same rule, so the owner of a bucket finds a
    // k-mer under one key whichever shard it came from)
    g.seg1 = d_seg; g.cnt1 = d_cnt;
    g.loose_cap = 1u << 16;
    const size_t b_ctr = 256;
    const uint64_t n_seg = plan->cnt_entries;
    // (a shard without reads cuts nothing and fits any plan)
    KV_REQUIRE(!g.compact || reads->n_tiles == 0 || skm_lane_fits(g, reads), KV_ERR_NOTIMPL, "kv_mex_emit: 16-byte records need a shard of equal-length reads (the lane-per-read cut)");
    uint64_t *d_off = nullptr;
    auto lay = [&](SkmCarve c) {
        g.loose = c.take<uint64_t>(g.loose_cap * (size_t)g.lrecw * 8);
        g.ctr = c.take<unsigned long long>(b_ctr);
        if (d_out) d_off = c.take<uint64_t>(mex_scan_bytes(n_seg));
        return c.total;
    };
    KV_HIP(idx.arena.need(lay(SkmCarve())));
    lay(SkmCarve(idx.arena.p));
    KV_HIP(hipMemsetAsync(g.ctr, 0, b_ctr, st));
    // a workgroup that takes no tile still writes its counts; workgroups beyond the grid never run: zero them
    KV_HIP(hipMemsetAsync(d_cnt, 0, plan->cnt_entries * 4, st));
    if (reads->n_tiles) {
        tl_s1_threads = plan->nwg1 <= 256u ? 1024u : 0u;
        skm_launch_emit(g, reads, st);
        tl_s1_threads = 0;
    }
    KV_HIP(hipGetLastError());
    if (d_out) {
        KvProfScope prof("k_mex_pack");
        mex_scan_launch(d_cnt, n_seg, plan->cap1, d_off, st);
        hipLaunchKernelGGL(k_mex_gather, dim3((unsigned)std::min<uint64_t>((n_seg + 3) / 4, 1u << 20)), dim3(256), 0, st, d_seg, d_cnt, d_off, n_seg, plan->cap1,
                           plan->recw, d_out, out_cap_words / plan->recw);
        KV_HIP(hipGetLastError());
    }
    KvReadback rb;
    hipError_t rb_err = hipSuccess;
    const unsigned long long *ctr = rb.add(g.ctr, SKM_CTR_FAIL + 1, st, &rb_err);
    std::vector<const uint64_t *> bounds(plan->ndest + 1, nullptr);
    if (d_out)
        for (int d = 0; d <= plan->ndest; ++d) bounds[d] = rb.add(d_off + (uint64_t)plan->c_lo[d] * plan->nwg1, 1, st, &rb_err);
    KV_HIP(rb_err);
    KV_HIP(rb.wait(st));
    if (d_out) {
        for (int d = 0; d < plan->ndest; ++d) records_per_dest[d] = *bounds[d + 1] - *bounds[d];
        *packed = (*bounds[plan->ndest] - *bounds[0]) * (uint64_t)plan->recw <= out_cap_words ? 1 : 0;
    }
    // records that miss their segment have nowhere to travel in: the plan's capacity is twice the expected fill, so this
    // means a pathological input (one minimizer everywhere); no silent change of layout
    KV_REQUIRE(ctr[SKM_CTR_LOOSE] == 0 && ctr[SKM_CTR_FAIL] == 0, KV_ERR_CAPACITY, "kv_mex_emit: %llu records did not fit their exchange segment", ctr[SKM_CTR_LOOSE]);
    // a later scan of this shard against the set of interesting k-mers buckets the shard on its own: 1 / ndest of the coverage
    // leaves more of its k-mers distinct than the sample's ~20 % (measured: 30 / 33 / 49 % at 1/2, 1/4, 1/8 of 30x)
    { std::lock_guard<std::mutex> glk(g_skm_mu); g_skm_last_distinct = std::min(0.9, 0.2 * std::sqrt((double)plan->ndest)); }
    return KV_OK;
}

// the records n_src ranks sent for this rank's Cl coarse buckets -> S2 -> every distinct k-mer once as a (hash, occurrences)
// pair for its band's owner (the callback allocates the sink, as for kv_skm_route_distinct)
int kv_skm_mex_route(const kv_mex_plan *plan, int my_dest, const uint64_t *d_recv_seg, const uint32_t *d_recv_cnt, int n_src, int compact, int keep_scan,
                     int (*alloc)(void *ctx, uint32_t nwg, KvRouteSink *sink), int (*after)(void *ctx), void *ctx, uint64_t *n_kmers_in)
{
    KV_REQUIRE(plan && my_dest >= 0 && my_dest < plan->ndest && n_src >= 1, KV_ERR_ARG, "kv_mex_route: bad argument");
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    idx.drop(SkmIndex::BATCH | SkmIndex::MEX_SCAN);
    SkmGeom &g = idx.g;
    const uint32_t Cl = plan->c_lo[my_dest + 1] - plan->c_lo[my_dest];
    skm_geom_plan(g, plan, Cl);
    KV_REQUIRE(!(g.compact && keep_scan), KV_ERR_ARG, "kv_mex_route: the sample the scan is answered from needs records with positions (not a short-record plan)");
    g.n_src = (uint32_t)n_src;
    g.seg1 = const_cast<uint64_t *>(d_recv_seg); g.cnt1 = const_cast<uint32_t *>(d_recv_cnt);
    if (Cl == 0) { *n_kmers_in = 0; KvRouteSink rs; memset(&rs, 0, sizeof(rs)); return alloc(ctx, 1, &rs); }
    const uint32_t nseg = g.nwg1 * g.n_src;
    g.nwg2 = std::max<uint32_t>(std::max<uint32_t>(1u, std::min<uint32_t>(16u, 1024u / Cl)), (nseg + 767u) / 768u);
    g.nwg2 = std::min<uint32_t>(g.nwg2, nseg);
    KV_REQUIRE((nseg + g.nwg2 - 1) / g.nwg2 <= 768u, KV_ERR_ARG, "kv_mex_route: %u segments per bucket", nseg);
    // this rank's share of the sample: its buckets hold 1 / ndest of the k-mers, give or take the hash's evenness
    const uint64_t n_kmers_exp = plan->n_kmers_global / (uint64_t)plan->ndest + 1;
    const double rec_est = skm_rec_est(n_kmers_exp, (double)plan->n_reads_global / plan->ndest, g.w);
    // (a geometry at its limit -- 4096 fine buckets per coarse one: a handful of distinct 12-base minimizers per bucket -- has buckets of
    // very different sizes: at 248 x 4096 buckets a tenth of the records missed segments of 2 x the even share)
    const double slack2 = plan->F2 > SKM_S2_MAXF ? 3.0 : 1.4;
    g.cap2 = skm_seg_cap(rec_est / ((double)g.n_buckets * g.nwg2), slack2, 32);
    g.loose_cap = skm_loose_cap(rec_est, n_kmers_exp);
    const size_t rb = (size_t)g.recw * 8, b_ctr = 256;
    uint64_t *d_off = nullptr;
    auto lay = [&](SkmCarve c) {
        g.seg2 = c.take<uint64_t>((uint64_t)g.n_buckets * g.nwg2 * g.cap2 * rb);
        g.cnt2 = c.take<uint32_t>((uint64_t)g.n_buckets * g.nwg2 * 4);
        g.loose = c.take<uint64_t>(g.loose_cap * (size_t)g.lrecw * 8);
        if (compact) d_off = c.take<uint64_t>(mex_scan_bytes((uint64_t)Cl * nseg));
        g.ctr = c.take<unsigned long long>(b_ctr);
        return c.total;
    };
    KV_HIP(idx.arena.need(lay(SkmCarve())));
    lay(SkmCarve(idx.arena.p));
    KV_HIP(hipMemsetAsync(g.ctr, 0, b_ctr, st));
    g.bucket_kmers = std::max<uint64_t>(1, n_kmers_exp / g.n_buckets);
    {
        // buckets the geometry could not make small enough (plan->F2 at its limit): k_skm_route combines them in passes, each taking
        // the k-mers of one hash class -- as many passes as bring a pass's distinct k-mers (a fifth of the occurrences at sequencing
        // coverage) under 0.65 of the LDS table.  KV_MEX_PASSES=n (tests): at least that many whatever the size.
        const double distinct = (double)g.bucket_kmers * 0.2, room = 0.5 * (g.kw == 1 ? 4096.0 : 2048.0);
        // (the least any bucket gets -- k_skm_route goes by a bucket's own record count: what the average bucket needs at 0.65 of the table)
        g.passes = distinct > room ? std::min<uint32_t>(16u, std::max<uint32_t>(2u, (uint32_t)std::ceil(distinct / (0.65 * 2.0 * room)))) : 1u;
        if (const char *e = kv_knob("KV_MEX_PASSES")) { const int v = atoi(e); if (v >= 1 && v <= 16) g.passes = (uint32_t)v; }
    }
    if (compact) {
        // the sources sent only the filled part of their segments, in segment order: a segment starts where the counts in
        // front of it end
        mex_scan_launch(g.cnt1, (uint64_t)Cl * nseg, g.cap1, d_off, st);
        g.seg1_off = d_off;
    }
    // how many k-mer occurrences arrived (the caller's buffer must hold a pair for each in the worst case)
    hipLaunchKernelGGL(k_mex_sum_kmers, dim3(1024), dim3(256), 0, st, g.seg1, g.cnt1, g.seg1_off, (uint64_t)Cl * nseg, g.cap1, (uint32_t)g.recw, &g.ctr[SKM_CTR_ARRIVED]);
    skm_launch_split(g, st);
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(&g.ctr[SKM_CTR_LOOSE_S12], &g.ctr[SKM_CTR_LOOSE], 8, hipMemcpyDeviceToDevice, st));
    skm_plan_tickets(g);
    const uint32_t nwg3 = skm_nwg3(g);
    KvRouteSink rs;
    memset(&rs, 0, sizeof(rs));
    { const int rc = alloc(ctx, nwg3, &rs); if (rc != KV_OK) return rc; }
    // keep_scan (the case sample): key + hash of every distinct k-mer stay, bucket by bucket, and the buckets themselves stay where
    // they are -- this rank will answer the scan for its buckets (kv_skm_mex_scan_set).  A stretch holds one and a half average shares
    // of 0.45 distinct k-mers per occurrence; one that runs out drops the list (SKM_CTR_DL_RAN_OUT) and the scan goes the other way.
    bool dl_new = false;
    const char *dl_why = "not asked for";
    // Room: 0.72 entries per occurrence in one stretch per workgroup covers a shard's 4-15 x with slack for uneven shares.  An owner of
    // config 4 holds 7.9 G occurrences at 30 x, a fifth of them distinct, and 16 bytes for each of 0.72 x 7.9 G entries is memory it does
    // not have: half of that next, and last a POOL with room for 0.22 -- chunks the workgroups draw one after the other (SKM_CTR_POOL_CHUNKS), so that
    // what one workgroup needs beyond its even share comes out of what another leaves (a quarter more than the even share per workgroup
    // was not enough there: 12-base minimizers make a million buckets far from even).  KV_MEX_DL_POOL=1 (tests): the pool at once.
    static const double dl_room[3] = {0.72, 0.36, 0.22};
    const bool pool_first = kv_knob("KV_MEX_DL_POOL") && atoi(kv_knob("KV_MEX_DL_POOL")) != 0;
    for (int attempt = pool_first ? 2 : 0; keep_scan && attempt < 3 && !dl_new; ++attempt) {
        const bool pool = attempt == 2;
        const double room = pool && pool_first ? dl_room[0] : dl_room[attempt];
        uint64_t cap_wg = std::min<uint64_t>((uint64_t)((double)n_kmers_exp * room / nwg3) + 4096, 0xfffffff0ull / nwg3);
        uint64_t entries = cap_wg * nwg3, chunk = 0, nchunks = 0;
        if (pool) {
            // a chunk holds any bucket's list (a table's worth per pass) four times over and is an eighth of a workgroup's even share
            // where that is more; every workgroup leaves its last chunk part empty: one chunk each on top
            chunk = std::min<uint64_t>(std::max<uint64_t>(entries / ((uint64_t)nwg3 * 8), 4ull * std::max<uint32_t>(g.passes, 2u) * 4096ull), 1ull << 20) & ~255ull;
            nchunks = std::min<uint64_t>(entries / chunk + nwg3, 0xfffffff0ull / chunk);
            entries = nchunks * chunk;
            cap_wg = 0;
        }
        const size_t b_all = SkmDistinctList::bytes(entries, g.kw, g.n_buckets);
        if (idx.dl.bytes == 0) idx.dl_refused = SIZE_MAX;
        if (b_all > idx.dl.bytes) {
            // not worth asking: refused before, or more than the device has left beside what the arena itself would give back
            size_t mem_free = 0, mem_total = 0;
            if (b_all >= idx.dl_refused || (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && b_all > mem_free + idx.dl.bytes)) {
                dl_why = "no memory for it";
                continue;
            }
        }
        const int lrc = idx.list.carve(idx.dl, entries, g.kw, g.n_buckets, (uint32_t)cap_wg, (uint32_t)chunk, (uint32_t)nchunks, st);
        if (lrc != KV_OK && lrc != KV_ERR_CAPACITY) return lrc;
        if (lrc == KV_OK) {
            idx.list.attach(g);      // (and stays attached: kv_skm_mex_scan_set works on a copy of this geometry)
            dl_new = true;
            dl_why = attempt == 0 ? "kept" : attempt == 1 ? "kept (room for 0.36 entries per occurrence)" : "kept (a pool of chunks the workgroups draw from)";
        } else {
            (void)hipGetLastError();                    // no room: no list, the scan goes the other way
            dl_why = "no memory for it";
            idx.dl_refused = std::min(idx.dl_refused, b_all);
        }
    }
    skm_launch_route(g.compact ? SKM_INST(k_skm_route<1, 4096, true>) : g.kw == 1 ? SKM_INST(k_skm_route<1, 4096>) : SKM_INST(k_skm_route<2, 2048>), g, plan->ksize, rs, st);
    KV_HIP(hipGetLastError());
    // the packing of the pairs (the caller's `after`) is queued behind the route kernels and everything is waited for once: its
    // kernels bound what they write by the output's capacity, so what the counters say can be judged afterwards
    if (after) { const int rc = after(ctx); if (rc != KV_OK) return rc; }
    KvReadback back;
    hipError_t rb_err = hipSuccess;
    const unsigned long long *sctr = back.add(g.ctr, SKM_CTR_COUNT, st, &rb_err);
    KV_HIP(rb_err);
    KV_HIP(back.wait(st));
    const unsigned long long arrived = sctr[SKM_CTR_ARRIVED];
    *n_kmers_in = arrived;
    idx.mex_scan_ready = dl_new && sctr[SKM_CTR_DL_RAN_OUT] == 0 && sctr[SKM_CTR_FAIL] == 0;
    idx.k = plan->ksize;
    if (kv_knob("KV_SKM_VERBOSE"))
        fprintf(stderr, "[kv_skm] exchange owner: %llu k-mers arrived in %u buckets (%u passes, segments of %u records), %.1f%% distinct, %.2f%% outside the LDS tables, "
                        "%llu records outside their bucket's segments\n",
                arrived, g.n_buckets, g.passes, g.cap2, arrived ? 100.0 * (double)sctr[SKM_CTR_DISTINCT] / (double)arrived : 0.0,
                arrived ? 100.0 * skm_outside_tables(sctr) / (double)arrived : 0.0, sctr[SKM_CTR_LOOSE_S12]);
    if (keep_scan && kv_knob("KV_SKM_VERBOSE")) {
        fprintf(stderr, "[kv_skm] exchange owner: the distinct list its scan answers from: %s\n",
                !dl_new ? dl_why : sctr[SKM_CTR_DL_RAN_OUT] != 0 ? (g.dl_chunk ? "dropped (the pool of chunks ran out)" : "dropped (a workgroup's stretch ran out)")
                                 : sctr[SKM_CTR_FAIL] != 0 ? "dropped (loose list overflow)" : dl_why);
        if (dl_new && g.dl_chunk)
            fprintf(stderr, "[kv_skm] exchange owner: %llu of %u chunks of %u entries drawn for %llu distinct k-mers\n", sctr[SKM_CTR_POOL_CHUNKS], g.dl_nchunks, g.dl_chunk, sctr[SKM_CTR_DISTINCT]);
    }
    if (sctr[SKM_CTR_FAIL] != 0) {
        kv_set_error("kv_mex_route: loose record list overflow (%llu records)", sctr[SKM_CTR_LOOSE]);
        return KV_ERR_CAPACITY;
    }
    return KV_OK;
}

// The hits of this rank's minimizer buckets against the gathered set of interesting hashes (p.set_*): see k_skm_set_hits.  Needs the
// state kv_skm_mex_route(keep_scan) left on this stream; KV_ERR_CAPACITY when it is not there (or a bucket holds more members than its
// table takes, or the hits do not fit): the caller then scans its shard against the set (kv_novel_scan_set) as before.
int kv_skm_mex_scan_set(const NovelParams &p, int ksize, uint64_t *d_tags, uint8_t *d_abund, uint64_t cap, uint64_t *n_hits)
{
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    if (!idx.mex_scan_ready || idx.k != ksize) {
        kv_set_error("kv_mex_scan_set: no combined buckets with a distinct list on this stream (kv_mex_route with keep_scan, nothing bucketed since)");
        return KV_ERR_CAPACITY;
    }
    SkmGeom sg = idx.g;
    idx.list.attach(sg);
    KV_HIP(hipMemsetAsync(&sg.ctr[SKM_CTR_TICKET_SCAN], 0, 8, st));
    KV_HIP(hipMemsetAsync(&sg.ctr[SKM_CTR_SET_HITS], 0, 8, st));
    SetHitSink out;
    out.tags = (unsigned long long *)d_tags; out.abund = d_abund; out.count = &sg.ctr[SKM_CTR_SET_HITS]; out.cap = cap;
    const uint32_t nwg3 = skm_nwg3(sg);
    {
        KvProfScope prof("k_skm_set_hits");
        const size_t lds = (size_t)(SKM_THREADS3 / 64) * skm_wave_scratch_words(sg.sbw) * 4;
        const auto kernel = sg.kw == 1 ? SKM_INST(k_skm_set_hits<1, 2048>) : SKM_INST(k_skm_set_hits<2, 1024>);
        hipLaunchKernelGGL(skm_launching(kernel, st), dim3(nwg3), dim3(SKM_THREADS3), lds, st, sg, p, out);
        skm_launch_loose(SKM_INST(k_skm_loose_set_hits<1>), SKM_INST(k_skm_loose_set_hits<2>), st, sg, p, out);
    }
    KV_HIP(hipGetLastError());
    KvReadback back;
    hipError_t rb_err = hipSuccess;
    const unsigned long long *c = back.add(sg.ctr, SKM_CTR_SET_HITS + 1, st, &rb_err);
    KV_HIP(rb_err);
    KV_HIP(back.wait(st));
    if (c[SKM_CTR_FAIL] != 0) {
        idx.drop(SkmIndex::MEX_SCAN);
        kv_set_error("kv_mex_scan_set: a bucket holds more members of the set than its table takes");
        return KV_ERR_CAPACITY;
    }
    KV_REQUIRE(c[SKM_CTR_SET_HITS] <= cap, KV_ERR_CAPACITY, "kv_mex_scan_set: %llu hits exceed the buffer of %llu", c[SKM_CTR_SET_HITS], (unsigned long long)cap);
    *n_hits = c[SKM_CTR_SET_HITS];
    return KV_OK;
}

// the filled part of a shard's exchange segments, destination after destination (what actually travels): d_out receives the
// records, records_per_dest[d] how many go to rank d.  The counts slab travels as it is.
int kv_skm_mex_pack(const kv_mex_plan *plan, const uint64_t *d_seg, const uint32_t *d_cnt, uint64_t *d_out, uint64_t *records_per_dest)
{
    hipStream_t st = kv_stream();
    skm_launched_begin(st);
    SkmIndex &idx = skm_index_for(st);
    std::lock_guard<std::mutex> lk(idx.mu);
    const uint64_t n_seg = plan->cnt_entries;
    // the offsets go where the stream's bucketed batch lies: whatever that was -- a batch a scan could reuse, an owner's combined
    // buckets kept for kv_skm_mex_scan_set, a distinct list -- is gone after this call
    idx.drop(SkmIndex::ALL);
    KV_HIP(idx.arena.need(mex_scan_bytes(n_seg)));
    uint64_t *d_off = (uint64_t *)idx.arena.p;
    mex_scan_launch(d_cnt, n_seg, plan->cap1, d_off, st);
    hipLaunchKernelGGL(k_mex_gather, dim3((unsigned)std::min<uint64_t>((n_seg + 3) / 4, 1u << 20)), dim3(256), 0, st, d_seg, d_cnt, d_off, n_seg, plan->cap1,
                       plan->recw, d_out, ~0ull);
    KV_HIP(hipGetLastError());
    KvReadback rb;
    hipError_t rb_err = hipSuccess;
    std::vector<const uint64_t *> bounds(plan->ndest + 1, nullptr);
    for (int d = 0; d <= plan->ndest; ++d) bounds[d] = rb.add(d_off + (uint64_t)plan->c_lo[d] * plan->nwg1, 1, st, &rb_err);
    KV_HIP(rb_err);
    KV_HIP(rb.wait(st));
    for (int d = 0; d < plan->ndest; ++d) records_per_dest[d] = *bounds[d + 1] - *bounds[d];
    return KV_OK;
}

// the instances the last call into this file launched on the calling thread's stream (include/kvsketch.h)
extern "C" int kv_skm_last_instances(char *out, uint64_t cap)
{
    KV_REQUIRE(g_skm_launched.get(kv_stream()).report(out, cap), KV_ERR_CAPACITY, "kv_skm_last_instances: buffer too small");
    return KV_OK;
}
