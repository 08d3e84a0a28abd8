// kv_varfilter.hip -- `kevlar varfilter` (kevlar/varfilter.py, kevlar/intervalforest.py, kevlar.parse_bed): calls that overlap a
// region of a BED file get the UserFilter.  The reference puts every call into an interval tree and looks every BED line up in it,
// one Python iteration per line.  Here it is a join between a small sorted set of calls and a streamed text:
//   (1) create: the calls sorted by (chromosome, start) with rocPRIM's stable radix sort, per chromosome the running maximum of
//       `end` over that order, an open-addressing table of the chromosome names, one flag byte per call;
//   (2) scan: BED text chunk by chunk.  A workgroup stages its tile of the text in LDS, lists the starts of the tile's lines and
//       deals them to its lanes; a lane parses its line (kv_varfilter_plan.h has the byte rules), finds the chromosome -- a slot is
//       picked by a hash of the name, a hit is the name's bytes compared in full -- and joins;
//   (3) regions: the same join for regions that are already numbers.
// The join (vf_join): binary search of the first call that starts at or behind the region's end, then backwards while the running
// maximum says that a call in front still ends behind the region's start.  That walk is exact and ends early whatever the longest
// call is.  Flags are plain byte stores of 1: every writer writes the same value.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan_by_key.hpp>

#include "kv_device.h"
#include "kv_varfilter_plan.h"

namespace {

enum { VF_LINES = 0, VF_SKIPPED, VF_PARSED, VF_KNOWN, VF_OVERLAPS, VF_FLAGGED, VF_BAD, VF_NCTR };

// the calls in (chromosome, start) order and the names they are on; what both entry points join against
struct VfIndex {
    const uint8_t *names;          // the distinct chromosome names, one after the other
    const uint64_t *name_off;      // name c = names[name_off[c] .. name_off[c + 1])
    const uint32_t *table;         // slot -> chromosome id or VF_NO_CHROM
    uint64_t capmask;
    const uint64_t *seg;           // calls of chromosome c = sorted calls seg[c] .. seg[c + 1]
    const long long *start, *end;  // 0-based half-open, sorted order
    const long long *runmax;       // max of end over the calls of the same chromosome up to and including this one
    uint8_t *flags;                // sorted order
};

// flag every call of `chrom` that (s, e) hits; the number of them
__device__ __forceinline__ uint64_t vf_join(const VfIndex &ix, uint32_t chrom, long long s, long long e)
{
    if (!(s < e)) return 0;
    const uint64_t first = ix.seg[chrom];
    uint64_t lo = first, hi = ix.seg[chrom + 1];
    while (lo < hi) {                                       // the first call with start >= e: nothing from there on is hit
        const uint64_t mid = (lo + hi) >> 1;
        if (ix.start[mid] < e) lo = mid + 1; else hi = mid;
    }
    uint64_t found = 0;
    for (uint64_t j = lo; j > first && ix.runmax[j - 1] > s; --j)
        if (ix.end[j - 1] > s) { ix.flags[j - 1] = 1; ++found; }
    return found;
}

__device__ __forceinline__ void vf_count(unsigned long long *ctr, int which, uint64_t mine)
{
    const uint64_t all = wave_sum_u64(mine);
    if ((threadIdx.x & 63u) == 0 && all) atomicAdd(&ctr[which], (unsigned long long)all);
}

// ---- create -----------------------------------------------------------------------------------------------------------------
__global__ void k_vf_start_keys(const long long *start, uint64_t n, unsigned long long *keys, uint32_t *idx)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        keys[i] = (unsigned long long)start[i] ^ (1ull << 63);      // signed order as unsigned order
        idx[i] = (uint32_t)i;
    }
}

__global__ void k_vf_gather_u32(const uint32_t *src, const uint32_t *idx, uint64_t n, uint32_t *dst)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}

__global__ void k_vf_gather_calls(const long long *start, const long long *end, const uint32_t *perm, uint64_t n, long long *start_s,
                                  long long *end_s)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        start_s[i] = start[perm[i]];
        end_s[i] = end[perm[i]];
    }
}

// seg[c] = the first sorted call on a chromosome >= c (c = n_chroms: all of them)
__global__ void k_vf_segments(const uint32_t *chrom_s, uint64_t n_calls, uint64_t n_chroms, uint64_t *seg)
{
    for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c <= n_chroms; c += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n_calls;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (chrom_s[mid] < c) lo = mid + 1; else hi = mid;
        }
        seg[c] = lo;
    }
}

// ---- scan -------------------------------------------------------------------------------------------------------------------
struct VfScan {
    const uint8_t *text;           // the chunk: `alloc` readable bytes (a multiple of 16), `n` of them text
    uint64_t n, alloc, goff;       // goff: offset of text[0] in the file
    VfIndex ix;
    unsigned long long *ctr;       // VF_LINES ..: running totals; [VF_BAD]: least offset of a bad line of this call
};

// the chunk as the parser reads it: a byte of the staged window comes out of LDS, any other one out of memory, and the text is
// followed by line ends without number (a last line without '\n' ends like the others)
struct VfText {
    const uint8_t *lds;            // lds[i] = text[base - VF_LDS_BEFORE + i], i < window
    const uint8_t *text;
    uint64_t n, base;
    uint32_t window;
    __device__ __forceinline__ uint32_t get(uint64_t pos) const
    {
        if (pos >= n) return '\n';
        const uint64_t i = pos + VF_LDS_BEFORE - base;      // (wraps to something huge in front of the window)
        return i < window ? lds[i] : text[pos];
    }
};

enum { VF_LINE_SKIP, VF_LINE_REGION, VF_LINE_BAD };

// one line from its first byte: comment, blank, (name, start, end), or outside the grammar
__device__ int vf_parse_line(const VfText &tx, uint64_t p, uint64_t &name_at, uint64_t &name_len, uint64_t &name_hash, long long &s,
                             long long &e)
{
    uint32_t c = tx.get(p);
    if (c == '#') return VF_LINE_SKIP;
    while (c != '\n' && vf_is_sep(c)) c = tx.get(++p);
    if (c == '\n') return VF_LINE_SKIP;
    name_at = p;
    uint64_t h = vf_hash_init();
    while (!vf_is_sep(c)) { h = vf_hash_step(h, c); c = tx.get(++p); }
    name_len = p - name_at;
    name_hash = vf_hash_finish(h);
    for (int field = 0; field < 2; ++field) {
        while (c != '\n' && vf_is_sep(c)) c = tx.get(++p);
        if (c == '\n') return VF_LINE_BAD;                  // fewer than three tokens
        VfNumber v;
        bool first = true;
        while (!vf_is_sep(c)) { v.feed(c, first); first = false; c = tx.get(++p); }
        if (!v.ok()) return VF_LINE_BAD;
        if (field) e = v.value(); else s = v.value();
    }
    return VF_LINE_REGION;
}

// vf_table_find of the plan header on the bytes of a token
__device__ uint32_t vf_find_chrom(const VfIndex &ix, const VfText &tx, uint64_t at, uint64_t len, uint64_t hash)
{
    for (uint64_t slot = hash & ix.capmask;; slot = (slot + 1) & ix.capmask) {
        const uint32_t id = ix.table[slot];
        if (id == VF_NO_CHROM) return VF_NO_CHROM;
        const uint64_t o = ix.name_off[id];
        if (ix.name_off[id + 1] - o != len) continue;
        bool same = true;
        for (uint64_t i = 0; i < len && same; ++i) same = ix.names[o + i] == tx.get(at + i);
        if (same) return id;
    }
}

template <uint32_t TILE>
__global__ __launch_bounds__(VF_THREADS) void k_vf_scan(VfScan p)
{
    constexpr uint32_t WINDOW = VF_LDS_BEFORE + TILE + VF_LDS_AFTER;        // bytes, a multiple of 16
    constexpr uint32_t MAX_LINES = TILE / 2 + 1;                            // vf_tile_lines
    __shared__ uint4 s_text[WINDOW / 16];
    __shared__ uint16_t s_line[MAX_LINES];                                  // tile-local starts of the lines that are not empty
    __shared__ uint32_t s_nlines;
    const uint64_t tile_base = (uint64_t)blockIdx.x * TILE;
    for (uint32_t v = threadIdx.x; v < WINDOW / 16; v += VF_THREADS) {
        uint4 q = make_uint4(0, 0, 0, 0);
        const uint64_t byte0 = tile_base + 16ull * v - VF_LDS_BEFORE;       // (v = 0 of tile 0 lies in front of the text)
        if ((tile_base != 0 || v != 0) && byte0 + 16 <= p.alloc) q = *reinterpret_cast<const uint4 *>(p.text + byte0);
        s_text[v] = q;
    }
    if (threadIdx.x == 0) s_nlines = 0;
    __syncthreads();

    VfText tx;
    tx.lds = reinterpret_cast<const uint8_t *>(s_text); tx.text = p.text; tx.n = p.n; tx.base = tile_base; tx.window = WINDOW;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(s_text);
    uint64_t n_lines = 0, n_skipped = 0, n_parsed = 0, n_known = 0, n_overlaps = 0;

    // a line starts behind a '\n' and at the chunk's first byte; a lane looks at four bytes a round, the whole workgroup at 1 KiB
    for (uint32_t w = threadIdx.x; w < TILE / 4; w += VF_THREADS) {
        const uint32_t cur = words[VF_LDS_BEFORE / 4 + w], prev = words[VF_LDS_BEFORE / 4 + w - 1];
        const uint32_t before = (cur << 8) | (prev >> 24);                  // byte i: the byte in front of byte i of `cur`
        uint32_t mine[4], n_mine = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint64_t pos = tile_base + 4ull * w + i;
            if (pos < p.n && (pos == 0 || ((before >> (8 * i)) & 0xFFu) == '\n')) {
                ++n_lines;
                if (((cur >> (8 * i)) & 0xFFu) == '\n') ++n_skipped;        // an empty line
                else mine[n_mine++] = 4 * w + i;
            }
        }
        if (n_mine) {
            const uint32_t at = atomicAdd(&s_nlines, n_mine);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < n_mine && at + i < MAX_LINES) s_line[at + i] = (uint16_t)mine[i];
        }
    }
    __syncthreads();

    const uint32_t nl = s_nlines < MAX_LINES ? s_nlines : MAX_LINES;
    for (uint32_t k = threadIdx.x; k < nl; k += VF_THREADS) {
        const uint64_t pos = tile_base + s_line[k];
        uint64_t name_at = 0, name_len = 0, name_hash = 0;
        long long s = 0, e = 0;
        const int kind = vf_parse_line(tx, pos, name_at, name_len, name_hash, s, e);
        if (kind == VF_LINE_SKIP) { ++n_skipped; continue; }
        if (kind == VF_LINE_BAD) { atomicMin(&p.ctr[VF_BAD], (unsigned long long)(p.goff + pos)); continue; }
        ++n_parsed;
        const uint32_t chrom = vf_find_chrom(p.ix, tx, name_at, name_len, name_hash);
        if (chrom == VF_NO_CHROM) continue;
        ++n_known;
        n_overlaps += vf_join(p.ix, chrom, s, e);
    }
    vf_count(p.ctr, VF_LINES, n_lines);
    vf_count(p.ctr, VF_SKIPPED, n_skipped);
    vf_count(p.ctr, VF_PARSED, n_parsed);
    vf_count(p.ctr, VF_KNOWN, n_known);
    vf_count(p.ctr, VF_OVERLAPS, n_overlaps);
}

// ---- regions ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VF_THREADS) void k_vf_regions(VfIndex ix, const uint32_t *chrom, const long long *start, const long long *end,
                                                           uint64_t n, uint64_t n_known, unsigned long long *ctr)
{
    uint64_t n_overlaps = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (chrom[i] != VF_NO_CHROM) n_overlaps += vf_join(ix, chrom[i], start[i], end[i]);
    vf_count(ctr, VF_OVERLAPS, n_overlaps);
    if (blockIdx.x == 0 && threadIdx.x == 0) {              // the caller parsed them, and knows which chromosomes it found
        atomicAdd(&ctr[VF_PARSED], (unsigned long long)n);
        atomicAdd(&ctr[VF_KNOWN], (unsigned long long)n_known);
    }
}

// ---- results ----------------------------------------------------------------------------------------------------------------
__global__ void k_vf_unsort_flags(const uint8_t *flags, const uint32_t *perm, uint64_t n, uint8_t *out)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[perm[i]] = flags[i];
}

__global__ __launch_bounds__(VF_THREADS) void k_vf_count_flags(const uint8_t *flags, uint64_t n, unsigned long long *ctr)
{
    uint64_t mine = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) mine += flags[i] != 0;
    vf_count(ctr, VF_FLAGGED, mine);
}

inline unsigned vf_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + VF_THREADS - 1) / VF_THREADS, 4096)); }

}  // namespace

struct kv_varfilter {
    uint64_t n_calls = 0, n_chroms = 0, capmask = 0;
    uint8_t *d_names = nullptr, *d_flags = nullptr;
    uint64_t *d_name_off = nullptr, *d_seg = nullptr;
    uint32_t *d_table = nullptr, *d_perm = nullptr;
    long long *d_start = nullptr, *d_end = nullptr, *d_runmax = nullptr;
    unsigned long long *d_ctr = nullptr;
    KvArena text;                           // the chunk being scanned; bytes, a multiple of 16
    KvArena regions;                        // the regions being joined: chromosome ids, starts, ends
    VfIndex index() const
    {
        VfIndex ix;
        ix.names = d_names; ix.name_off = d_name_off; ix.table = d_table; ix.capmask = capmask; ix.seg = d_seg;
        ix.start = d_start; ix.end = d_end; ix.runmax = d_runmax; ix.flags = d_flags;
        return ix;
    }
    ~kv_varfilter()
    {
        void *all[] = {d_names, d_flags, d_name_off, d_seg, d_table, d_perm, d_start, d_end, d_runmax, d_ctr, text.p, regions.p};
        for (void *p : all)
            if (p) (void)hipFree(p);
    }
};

// the stable order of the calls by (chromosome, start): by start first, then by chromosome, the second pass keeping the first's order
static int vf_sort_calls(const uint32_t *d_chrom, const long long *d_start, uint64_t n, uint32_t *d_perm, hipStream_t st)
{
    KvDevBuf keys_a, keys_b, idx_a, chrom_a, chrom_b, tmp;
    KV_HIP(keys_a.alloc(n * 8)); KV_HIP(keys_b.alloc(n * 8)); KV_HIP(idx_a.alloc(n * 4)); KV_HIP(chrom_a.alloc(n * 4)); KV_HIP(chrom_b.alloc(n * 4));
    const dim3 grid(vf_grid(n)), block(VF_THREADS);
    hipLaunchKernelGGL(k_vf_start_keys, grid, block, 0, st, d_start, n, keys_a.as<unsigned long long>(), d_perm);
    KV_HIP(hipGetLastError());
    size_t need1 = 0, need2 = 0;
    KV_HIP(rocprim::radix_sort_pairs(nullptr, need1, keys_a.as<unsigned long long>(), keys_b.as<unsigned long long>(), d_perm, idx_a.as<uint32_t>(),
                                     (size_t)n, 0, 64, st));
    KV_HIP(rocprim::radix_sort_pairs(nullptr, need2, chrom_a.as<uint32_t>(), chrom_b.as<uint32_t>(), idx_a.as<uint32_t>(), d_perm, (size_t)n, 0, 32, st));
    KV_HIP(tmp.alloc(std::max(need1, need2)));
    KV_HIP(rocprim::radix_sort_pairs(tmp.p, need1, keys_a.as<unsigned long long>(), keys_b.as<unsigned long long>(), d_perm, idx_a.as<uint32_t>(),
                                     (size_t)n, 0, 64, st));
    hipLaunchKernelGGL(k_vf_gather_u32, grid, block, 0, st, d_chrom, idx_a.as<uint32_t>(), n, chrom_a.as<uint32_t>());
    KV_HIP(hipGetLastError());
    KV_HIP(rocprim::radix_sort_pairs(tmp.p, need2, chrom_a.as<uint32_t>(), chrom_b.as<uint32_t>(), idx_a.as<uint32_t>(), d_perm, (size_t)n, 0, 32, st));
    KV_HIP(hipStreamSynchronize(st));       // the scoped buffers go
    return KV_OK;
}

extern "C" int kv_varfilter_create(const char *names, const uint64_t *name_off, uint64_t n_chroms, const uint32_t *call_chrom,
                                   const int64_t *call_start, const int64_t *call_end, uint64_t n_calls, kv_varfilter **out)
{
    KV_REQUIRE(out, KV_ERR_ARG, "kv_varfilter_create: null argument");
    std::vector<uint32_t> table;
    KV_STEP(vf_table_build((const uint8_t *)names, name_off, n_chroms, table));
    KV_STEP(vf_check_calls(call_chrom, call_start, call_end, n_calls, n_chroms));
    hipStream_t st = kv_stream();
    kv_varfilter *h = new kv_varfilter;
    struct Guard { kv_varfilter *h; ~Guard() { delete h; } } guard{h};
    h->n_calls = n_calls;
    h->n_chroms = n_chroms;
    h->capmask = table.size() - 1;
    const uint64_t name_bytes = n_chroms ? name_off[n_chroms] : 0, nc = std::max<uint64_t>(n_calls, 1);
    const uint64_t zero_off = 0;
    KvDevBuf in_chrom, in_start, in_end, chrom_s, tmp;
    hipError_t e = kv_hip_malloc(&h->d_names, std::max<uint64_t>(name_bytes, 16));
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_name_off, (n_chroms + 1) * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_seg, (n_chroms + 1) * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_table, table.size() * 4);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_perm, nc * 4);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_start, nc * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_end, nc * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_runmax, nc * 8);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_flags, nc);
    if (e == hipSuccess) e = kv_hip_malloc(&h->d_ctr, VF_NCTR * 8);
    if (e == hipSuccess) e = in_chrom.alloc(nc * 4);
    if (e == hipSuccess) e = in_start.alloc(nc * 8);
    if (e == hipSuccess) e = in_end.alloc(nc * 8);
    if (e == hipSuccess) e = chrom_s.alloc(nc * 4);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "call index allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemsetAsync(h->d_flags, 0, nc, st));
    KV_HIP(hipMemsetAsync(h->d_ctr, 0, VF_NCTR * 8, st));
    KV_HIP(hipMemsetAsync(h->d_ctr + VF_BAD, 0xFF, 8, st));
    if (name_bytes) KV_HIP(hipMemcpyAsync(h->d_names, names, name_bytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(h->d_name_off, n_chroms ? name_off : &zero_off, (n_chroms + 1) * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(h->d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, st));
    if (n_calls) {
        KV_HIP(hipMemcpyAsync(in_chrom.p, call_chrom, n_calls * 4, hipMemcpyHostToDevice, st));
        KV_HIP(hipMemcpyAsync(in_start.p, call_start, n_calls * 8, hipMemcpyHostToDevice, st));
        KV_HIP(hipMemcpyAsync(in_end.p, call_end, n_calls * 8, hipMemcpyHostToDevice, st));
        KvProfScope prof("k_vf_create");
        KV_STEP(vf_sort_calls(in_chrom.as<uint32_t>(), in_start.as<long long>(), n_calls, h->d_perm, st));
        const dim3 grid(vf_grid(n_calls)), block(VF_THREADS);
        hipLaunchKernelGGL(k_vf_gather_u32, grid, block, 0, st, in_chrom.as<uint32_t>(), h->d_perm, n_calls, chrom_s.as<uint32_t>());
        hipLaunchKernelGGL(k_vf_gather_calls, grid, block, 0, st, in_start.as<long long>(), in_end.as<long long>(), h->d_perm, n_calls, h->d_start,
                           h->d_end);
        KV_HIP(hipGetLastError());
        size_t need = 0;
        KV_HIP(rocprim::inclusive_scan_by_key(nullptr, need, chrom_s.as<uint32_t>(), h->d_end, h->d_runmax, (size_t)n_calls,
                                              rocprim::maximum<long long>(), rocprim::equal_to<uint32_t>(), st));
        KV_HIP(tmp.alloc(need));
        KV_HIP(rocprim::inclusive_scan_by_key(tmp.p, need, chrom_s.as<uint32_t>(), h->d_end, h->d_runmax, (size_t)n_calls,
                                              rocprim::maximum<long long>(), rocprim::equal_to<uint32_t>(), st));
    }
    hipLaunchKernelGGL(k_vf_segments, dim3(vf_grid(n_chroms + 1)), dim3(VF_THREADS), 0, st, chrom_s.as<uint32_t>(), n_calls, n_chroms, h->d_seg);
    KV_HIP(hipGetLastError());
    KV_HIP(hipStreamSynchronize(st));       // the host arrays and the scoped buffers go
    guard.h = nullptr;
    *out = h;
    return KV_OK;
}

extern "C" int kv_varfilter_plan(uint64_t n_bytes, uint64_t *plan_out)
{
    KV_REQUIRE(plan_out, KV_ERR_ARG, "kv_varfilter_plan: null argument");
    const uint32_t tile = vf_tile_bytes(n_bytes);
    plan_out[0] = tile; plan_out[1] = vf_n_tiles(n_bytes, tile);
    plan_out[2] = VF_TILE_SMALL; plan_out[3] = VF_TILE_LARGE; plan_out[4] = VF_LARGE_FROM;
    return KV_OK;
}

extern "C" int kv_varfilter_chunk_cut(const char *buf, uint64_t n_bytes, int at_eof, uint64_t *cut)
{
    KV_REQUIRE(cut && (buf || n_bytes == 0), KV_ERR_ARG, "kv_varfilter_chunk_cut: null argument");
    *cut = vf_chunk_cut((const uint8_t *)buf, n_bytes, at_eof);
    return KV_OK;
}

extern "C" int kv_varfilter_scan(kv_varfilter *h, const char *text, uint64_t n_bytes, uint64_t text_offset)
{
    KV_REQUIRE(h && (text || n_bytes == 0), KV_ERR_ARG, "kv_varfilter_scan: null argument");
    KV_REQUIRE(n_bytes < VF_MAX_CHUNK, KV_ERR_ARG, "kv_varfilter_scan: chunk of %llu bytes", (unsigned long long)n_bytes);
    hipStream_t st = kv_stream();
    KV_HIP(hipMemsetAsync(h->d_ctr + VF_BAD, 0xFF, 8, st));
    if (n_bytes == 0) { KV_HIP(hipStreamSynchronize(st)); return KV_OK; }
    const hipError_t e = h->text.need_exact(((n_bytes + 15) & ~15ull) + 16);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "scan buffer allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemcpyAsync(h->text.p, text, n_bytes, hipMemcpyDefault, st));    // (the text may be on the device already)
    VfScan p;
    p.text = (const uint8_t *)h->text.p; p.n = n_bytes; p.alloc = h->text.bytes & ~15ull; p.goff = text_offset; p.ix = h->index(); p.ctr = h->d_ctr;
    const uint32_t tile = vf_tile_bytes(n_bytes);
    const uint64_t n_tiles = vf_n_tiles(n_bytes, tile);
    KV_REQUIRE(n_tiles < 0x7FFFFFFFull, KV_ERR_ARG, "kv_varfilter_scan: chunk too large");
    {
        KvProfScope prof("k_vf_scan");
        const dim3 grid((unsigned)n_tiles), block(VF_THREADS);
        if (tile == VF_TILE_LARGE) hipLaunchKernelGGL(k_vf_scan<VF_TILE_LARGE>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(k_vf_scan<VF_TILE_SMALL>, grid, block, 0, st, p);
    }
    KV_HIP(hipGetLastError());
    hipError_t re = hipSuccess;
    KvReadback rb;
    const unsigned long long *bad = rb.add((const unsigned long long *)h->d_ctr + VF_BAD, 1, st, &re);
    KV_HIP(re);
    KV_HIP(rb.wait(st));
    KV_REQUIRE(*bad == VF_NO_OFFSET, KV_ERR_ARG, "kv_varfilter_scan: the line at byte %llu is not `chromosome start end`", *bad);
    return KV_OK;
}

extern "C" int kv_varfilter_bad_line(kv_varfilter *h, uint64_t *offset)
{
    KV_REQUIRE(h && offset, KV_ERR_ARG, "kv_varfilter_bad_line: null argument");
    hipStream_t st = kv_stream();
    unsigned long long bad = 0;
    KV_HIP(hipMemcpyAsync(&bad, h->d_ctr + VF_BAD, 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    *offset = bad;
    return KV_OK;
}

extern "C" int kv_varfilter_regions(kv_varfilter *h, const uint32_t *chrom_id, const int64_t *start, const int64_t *end, uint64_t n)
{
    KV_REQUIRE(h && (n == 0 || (chrom_id && start && end)), KV_ERR_ARG, "kv_varfilter_regions: null argument");
    uint64_t n_known = 0;
    KV_STEP(vf_check_regions(chrom_id, n, h->n_chroms, &n_known));
    if (n == 0) return KV_OK;
    hipStream_t st = kv_stream();
    const size_t sizes[3] = {(size_t)n * 4, (size_t)n * 8, (size_t)n * 8};
    KvCarve<3> carve(sizes);
    const hipError_t e = carve.from(h->regions);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "region buffers allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemcpyAsync(carve.at<uint32_t>(0), chrom_id, n * 4, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(carve.at<long long>(1), start, n * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(carve.at<long long>(2), end, n * 8, hipMemcpyHostToDevice, st));
    {
        KvProfScope prof("k_vf_regions");
        hipLaunchKernelGGL(k_vf_regions, dim3(vf_grid(n)), dim3(VF_THREADS), 0, st, h->index(), carve.at<uint32_t>(0), carve.at<long long>(1),
                           carve.at<long long>(2), n, n_known, h->d_ctr);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipStreamSynchronize(st));       // the host arrays go
    return KV_OK;
}

extern "C" int kv_varfilter_hits(kv_varfilter *h, uint8_t *flags_out, uint64_t n_calls)
{
    KV_REQUIRE(h && (flags_out || n_calls == 0), KV_ERR_ARG, "kv_varfilter_hits: null argument");
    KV_REQUIRE(n_calls == h->n_calls, KV_ERR_ARG, "kv_varfilter_hits: the index has %llu calls, not %llu", (unsigned long long)h->n_calls,
               (unsigned long long)n_calls);
    if (n_calls == 0) return KV_OK;
    hipStream_t st = kv_stream();
    KvDevBuf unsorted;
    KV_HIP(unsorted.alloc(n_calls));
    hipLaunchKernelGGL(k_vf_unsort_flags, dim3(vf_grid(n_calls)), dim3(VF_THREADS), 0, st, h->d_flags, h->d_perm, n_calls, unsorted.as<uint8_t>());
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(flags_out, unsorted.p, n_calls, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}

extern "C" int kv_varfilter_stats(kv_varfilter *h, uint64_t *stats_out)
{
    KV_REQUIRE(h && stats_out, KV_ERR_ARG, "kv_varfilter_stats: null argument");
    hipStream_t st = kv_stream();
    KV_HIP(hipMemsetAsync(h->d_ctr + VF_FLAGGED, 0, 8, st));
    if (h->n_calls) {
        hipLaunchKernelGGL(k_vf_count_flags, dim3(vf_grid(h->n_calls)), dim3(VF_THREADS), 0, st, h->d_flags, h->n_calls, h->d_ctr);
        KV_HIP(hipGetLastError());
    }
    unsigned long long c[VF_NCTR];
    KV_HIP(hipMemcpyAsync(c, h->d_ctr, sizeof(c), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    for (int i = 0; i <= VF_FLAGGED; ++i) stats_out[i] = c[i];
    return KV_OK;
}

extern "C" int kv_varfilter_destroy(kv_varfilter *h)
{
    if (h) {
        (void)hipStreamSynchronize(kv_stream());
        delete h;
    }
    return KV_OK;
}
