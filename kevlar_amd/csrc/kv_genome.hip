// kv_genome.hip -- the reference genome of `kevlar localize` / `kevlar alac` parsed on the device and kept there (DESIGN.md
// section 9).  The host path reads the FASTA line by line in Python (kevlar_amd/seqio.py parse_seq_dict), a .gz through Python's
// gzip, and holds the genome twice before the first chunk is uploaded.  Here the file image is uploaded as it is -- plain, blocked
// gzip (kv_inflate.hip) or one gzip stream (kv_gunzip.hip) --, inflated where it is compressed, and split by kernels; what comes
// back to the host is the id of every sequence and where it starts.  The text is taken a segment at a time:
//
//   k_gn_check      a flag for every byte the host's text layer would treat differently (the file is then declined: KV_ERR_TYPE)
//   k_count_lines   newlines per 16-KB chunk                 \  kv_lines_device.h,
//   k_line_starts   byte offset of every line start          /  shared with the FASTQ reader
//   k_gn_classify   one item per line: defline or not, payload without the trailing blanks, id bytes
//   (scan)          deflines in front of every line = its record
//   k_gn_out        bytes of joined text every line owns: its payload, or the separator in front of its record
//   (scan, scan)    where every line's payload goes in the joined text; where every id goes in the id blob
//   k_gn_place      separators, the record table (sequence start, id offset), the destination of every line
//   k_gn_copy       a workgroup per 16 KB of INPUT: the payload parts of the lines that cross it, 16 bytes at a time
//
// The rules -- byte classes, what a line contributes, what travels from one segment to the next -- are kv_genome_plan.h.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kv_device.h"
#include "kv_internal.h"
#include "kv_lines_device.h"
#include "kv_genome_plan.h"

static_assert(GN_CHUNK == LN_CHUNK && GN_THREADS == LN_THREADS, "the splitter deals its work by the line kernels' chunks");

namespace {

#define GN_DST_ID (1ull << 63)               // a line's destination lies in the id blob, not in the joined text
// d_ctr of a segment: [0] decline flags, [1] raw length of the last line, [2] it is (part of) a defline, [3] ... with an open id,
// [4] strippable bytes on its end
#define GN_NCTR 8

__device__ __forceinline__ uint32_t gn_byte_of(const uint32_t (&w)[4], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 0xFFu; }

// every byte once: the classes that decline, and CR with its successor
__global__ __launch_bounds__(GN_THREADS) void k_gn_check(const uint8_t *__restrict__ text, uint64_t n, unsigned long long *ctr)
{
    const uint64_t c0 = (uint64_t)blockIdx.x * GN_CHUNK;
    uint32_t flags = 0;
    for (uint32_t i = threadIdx.x * 16u; i < GN_CHUNK; i += GN_THREADS * 16u) {
        const uint64_t at = c0 + i;
        if (at >= n) break;
        if (at + 16 <= n) {
            const uint4 v = *(const uint4 *)(text + at);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            // nothing at or above 0x80 and nothing below 0x20 in the 16 (sequence bytes): nothing to look at
            uint32_t odd = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t lowbits = w[q] & 0xE0E0E0E0u;                                   // zero in a byte below 0x20
                odd |= (w[q] & 0x80808080u) | ((lowbits - 0x01010101u) & ~lowbits & 0x80808080u);
            }
            if (odd == 0) continue;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const uint32_t c = gn_byte_of(w, b);
                flags |= gn_byte_flags(c);
                if (c == 0x0du) {
                    const bool has = at + (uint64_t)b + 1 < n;
                    const uint32_t nx = b < 15 ? gn_byte_of(w, (b + 1) & 15) : (has ? (uint32_t)text[at + 16] : 0u);
                    flags |= gn_cr_flag(has, nx);
                }
            }
        } else {
            for (uint64_t j = at; j < n; ++j) {
                const uint32_t c = text[j];
                flags |= gn_byte_flags(c);
                if (c == 0x0du) flags |= gn_cr_flag(j + 1 < n, j + 1 < n ? (uint32_t)text[j + 1] : 0u);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) flags |= __shfl_down(flags, d);
    if ((threadIdx.x & 63) == 0 && flags) atomicOr(ctr, (unsigned long long)flags);
}

// line l = text[ls[l], ls[l + 1] - 1) (the last one: up to n).  info[l] = kind | pay_off << 2 | is_def << 3
__global__ void k_gn_classify(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ ls, uint64_t n_lines, uint32_t cont,
                              uint32_t cont_def, uint32_t cont_id, uint32_t *__restrict__ info, uint32_t *__restrict__ pay_len,
                              uint32_t *__restrict__ cnt_def, uint32_t *__restrict__ cnt_id, unsigned long long *ctr)
{
    for (uint64_t l = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; l < n_lines; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = ls[l], b = l + 1 < n_lines ? ls[l + 1] - 1 : n;
        const bool first = l == 0 && cont;
        const GnLine r = gn_classify(text, a, b, first, first && cont_def, first && cont_id);
        info[l] = r.kind | (r.pay_off << 2) | (r.is_def << 3);
        pay_len[l] = r.pay_len;
        cnt_def[l] = r.is_def;
        cnt_id[l] = r.kind == GN_ID ? r.pay_len : 0u;
        if (r.flags) atomicOr(ctr, (unsigned long long)r.flags);
        if (l + 1 == n_lines) { ctr[1] = b - a; ctr[2] = r.defline; ctr[3] = r.id_open; ctr[4] = r.held; }
    }
}

__global__ void k_gn_out(uint64_t n_lines, const uint32_t *__restrict__ info, const uint32_t *__restrict__ pay_len,
                         const uint64_t *__restrict__ def_base, uint64_t records0, uint32_t *__restrict__ cnt_out)
{
    for (uint64_t l = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; l < n_lines; l += (uint64_t)gridDim.x * blockDim.x)
        cnt_out[l] = gn_out_bytes(info[l] & 3u, (info[l] >> 3) & 1u, pay_len[l], records0 + def_base[l]);
}

// dst[l]: where line l's payload goes (GN_DST_ID | offset in the segment's id blob, or offset in the joined text); a sequence
// line in front of the first defline loses its payload.  A defline writes its record's separator and its row of the record table.
__global__ void k_gn_place(uint64_t n_lines, const uint32_t *__restrict__ info, uint32_t *__restrict__ pay_len, const uint64_t *__restrict__ def_base,
                           const uint64_t *__restrict__ id_base, const uint64_t *__restrict__ out_base, uint64_t records0, uint64_t out_off0,
                           uint64_t id_off0, uint8_t *__restrict__ text_out, uint64_t *__restrict__ rec_seq_start, uint64_t *__restrict__ rec_id_off,
                           uint64_t *__restrict__ dst)
{
    for (uint64_t l = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; l < n_lines; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t kind = info[l] & 3u, is_def = (info[l] >> 3) & 1u;
        const uint64_t before = records0 + def_base[l];
        uint64_t d = 0;
        if (is_def) {
            const uint64_t sep = before > 0 ? 1 : 0;
            if (sep) text_out[out_off0 + out_base[l]] = (uint8_t)GN_SEPARATOR;
            rec_seq_start[def_base[l]] = out_off0 + out_base[l] + sep;
            rec_id_off[def_base[l]] = id_off0 + id_base[l];
        }
        if (kind == GN_ID) d = GN_DST_ID | id_base[l];
        else if (kind == GN_SEQ) {
            if (before > 0) d = out_off0 + out_base[l];
            else pay_len[l] = 0;
        }
        dst[l] = d;
    }
}

// 16 bytes held in v to d, by the widest stores d's alignment allows
__device__ __forceinline__ void gn_store16(uint8_t *d, const uint4 v)
{
    const uint32_t mis = (uint32_t)(uintptr_t)d & 15u;
    if (mis == 0) { *(uint4 *)d = v; return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if ((mis & 3u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ((uint32_t *)d)[q] = w[q];
        return;
    }
#pragma unroll
    for (int b = 0; b < 16; ++b) d[b] = (uint8_t)gn_byte_of(w, b);
}

// A workgroup takes chunk c of the input; a lane 16 bytes of it at a time.  The lines that cross the chunk are lines base[c] ..
// base[c + 1] (newlines in front of the chunk's first and of its end); a lane finds the line of its 16 bytes' first byte by a
// search over their starts and goes on from line to line inside the 16.  The part of a line's payload that lies in the 16 bytes
// goes to the line's destination: all 16 at once where they lie inside one payload, else byte by byte.  The work per lane does
// not depend on how long a line is: one line of 250 Mb and lines of 60 bytes fill the machine alike.
__global__ __launch_bounds__(GN_THREADS) void k_gn_copy(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ base,
                                                        const uint64_t *__restrict__ ls, uint64_t n_lines, const uint32_t *__restrict__ info,
                                                        const uint32_t *__restrict__ pay_len, const uint64_t *__restrict__ dst,
                                                        uint8_t *__restrict__ text_out, uint8_t *__restrict__ ids_out)
{
    const uint64_t c0 = (uint64_t)blockIdx.x * GN_CHUNK;
    const uint64_t first = base[blockIdx.x], last = std::min<uint64_t>(base[blockIdx.x + 1], n_lines - 1);
    for (uint32_t i = threadIdx.x * 16u; i < GN_CHUNK; i += GN_THREADS * 16u) {
        const uint64_t p = c0 + i;
        if (p >= n) break;
        const uint64_t uend = std::min<uint64_t>(p + 16, n);
        const bool whole = p + 16 <= n;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (whole) v = *(const uint4 *)(text + p);
        uint64_t lo = first, hi = last + 1;             // the last l in [first, last] with ls[l] <= p (ls[first] <= c0)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ls[mid] <= p) lo = mid; else hi = mid;
        }
        uint64_t l = lo, q = p;
        while (q < uend && l < n_lines) {
            const uint64_t lf = l + 1 < n_lines ? ls[l + 1] - 1 : n;       // where the line's LF is (or the text ends)
            const uint32_t in = info[l], kind = in & 3u;
            const uint64_t ps = ls[l] + ((in >> 2) & 1u), pe = ps + pay_len[l];
            const uint64_t s = std::max(q, ps), e = std::min(uend, pe);
            if (kind != GN_NONE && s < e) {
                const uint64_t d = dst[l];
                uint8_t *to = ((d & GN_DST_ID) ? ids_out : text_out) + (d & ~GN_DST_ID) + (s - ps);
                if (whole && s == p && e == p + 16) gn_store16(to, v);
                else
                    for (uint64_t j = s; j < e; ++j) to[j - s] = text[j];
            }
            q = lf + 1;
            ++l;
        }
    }
}

inline unsigned gn_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

}  // namespace

struct kv_genome {
    uint64_t uid = kv_next_uid();
    KvArena out;                          // the joined text, `total` bytes of it; readable up to out.bytes (a multiple of 16)
    uint64_t total = 0, text_seen = 0, n_segments = 0;
    int container = 0;                    // 0 plain, 1 blocked gzip, 2 one gzip stream
    std::string ids;
    std::vector<uint64_t> id_off, seq_start, seq_len;
    KvArena fetch;
    std::mutex mu;
    ~kv_genome() { out.release(); fetch.release(); }
};

int kv_genome_view(const kv_genome *g, KvGenomeView *view)
{
    KV_REQUIRE(g && view, KV_ERR_ARG, "kv_genome_view: null argument");
    view->text = (const uint8_t *)g->out.p; view->n = g->total; view->alloc = g->out.bytes & ~15ull; view->uid = g->uid;
    return KV_OK;
}

namespace {

// everything kv_genome_open needs and its result does not
struct GnWork {
    int fd = -1;
    const uint8_t *image = nullptr;
    size_t image_size = 0;
    std::vector<KvBgzfMember> members;
    std::vector<uint32_t> isize;
    KvGunzip *gz = nullptr;
    KvGunzipArenas gz_arenas;
    KvArena text[2], comp, scratch, lines, chunks, recs;
    int cur = 0;
    ~GnWork()
    {
        if (gz) kv_gunzip_close(gz);
        gz_arenas.release();
        for (KvArena *a : {&text[0], &text[1], &comp, &scratch, &lines, &chunks, &recs}) a->release();
        if (image) munmap((void *)image, image_size);
        if (fd >= 0) close(fd);
    }
};

// room for `need` bytes of joined text, `have` of them written
int gn_reserve(kv_genome *g, uint64_t have, uint64_t need, hipStream_t st)
{
    const uint64_t want = kv_round_up(need + 64, 4096);
    if (want <= g->out.bytes) return KV_OK;
    KvArena grown;
    hipError_t e = grown.need_exact(g->out.bytes == 0 ? want : kv_round_up(gn_grow(g->out.bytes, want), 4096));
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "kv_genome_open: no device memory for the genome text: %s", hipGetErrorString(e));
    if (have) e = hipMemcpyAsync(grown.p, g->out.p, have, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { grown.release(); kv_last_hip_code = (int)e; kv_set_error("kv_genome_open: %s", hipGetErrorString(e)); return KV_ERR_HIP; }
    g->out.release();
    g->out = grown;
    return KV_OK;
}

// one pass: text[0, n) of w.text[w.cur], the held bytes of the segment before in front
int gn_segment(kv_genome *g, GnWork &w, uint64_t n, GnCarry &carry, hipStream_t st)
{
    const uint8_t *text = (const uint8_t *)w.text[w.cur].p;
    const uint32_t n_chunks = (uint32_t)((n + GN_CHUNK - 1) / GN_CHUNK);
    KvCarve<3> chunks({(size_t)n_chunks * 4, ((size_t)n_chunks + 1) * 8, (size_t)GN_NCTR * 8});
    KV_HIP(chunks.from(w.chunks));
    uint32_t *d_counts = chunks.at<uint32_t>(0);
    uint64_t *d_base = chunks.at<uint64_t>(1);
    unsigned long long *d_ctr = chunks.at<unsigned long long>(2);
    KV_HIP(hipMemsetAsync(d_ctr, 0, GN_NCTR * 8, st));
    {
        KvProfScope prof("k_gn_check");
        hipLaunchKernelGGL(k_gn_check, dim3(n_chunks), dim3(GN_THREADS), 0, st, text, n, d_ctr);
    }
    {
        KvProfScope prof("k_count_lines");
        hipLaunchKernelGGL(k_count_lines, dim3(n_chunks), dim3(LN_THREADS), 0, st, text, n, d_counts);
        kv_excl_scan_launch(d_counts, n_chunks, d_base, st);
    }
    KV_HIP(hipGetLastError());
    unsigned long long newlines = 0;
    KV_HIP(hipMemcpyAsync(&newlines, d_base + n_chunks, 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    const uint64_t L = newlines + 1;
    KV_REQUIRE(L < 0xFFFFFFF0ull, KV_ERR_CAPACITY, "kv_genome_open: %llu lines in one segment", (unsigned long long)L);
    KvCarve<10> lines({(size_t)L * 8, (size_t)L * 4, (size_t)L * 4, (size_t)L * 4, (size_t)L * 4, (size_t)L * 4, (size_t)(L + 1) * 8,
                       (size_t)(L + 1) * 8, (size_t)(L + 1) * 8, (size_t)L * 8});
    KV_HIP(lines.from(w.lines));
    uint64_t *d_ls = lines.at<uint64_t>(0);
    uint32_t *d_info = lines.at<uint32_t>(1), *d_pay = lines.at<uint32_t>(2), *d_cdef = lines.at<uint32_t>(3), *d_cid = lines.at<uint32_t>(4),
             *d_cout = lines.at<uint32_t>(5);
    uint64_t *d_defb = lines.at<uint64_t>(6), *d_idb = lines.at<uint64_t>(7), *d_outb = lines.at<uint64_t>(8), *d_dst = lines.at<uint64_t>(9);
    KV_HIP(hipMemsetAsync(d_ls, 0, 8, st));
    const dim3 lgrid(gn_grid(L)), lblock(256);
    {
        KvProfScope prof("k_line_starts");
        hipLaunchKernelGGL(k_line_starts, dim3(n_chunks), dim3(LN_THREADS), 0, st, text, n, (const uint64_t *)d_base, (uint64_t)newlines, d_ls);
    }
    {
        KvProfScope prof("k_gn_classify");
        hipLaunchKernelGGL(k_gn_classify, lgrid, lblock, 0, st, text, n, (const uint64_t *)d_ls, L, carry.mid_line, carry.mid_defline, carry.id_open, d_info,
                           d_pay, d_cdef, d_cid, d_ctr);
        kv_excl_scan_launch(d_cdef, (uint32_t)L, d_defb, st);
        kv_excl_scan_launch(d_cid, (uint32_t)L, d_idb, st);
        hipLaunchKernelGGL(k_gn_out, lgrid, lblock, 0, st, L, (const uint32_t *)d_info, (const uint32_t *)d_pay, (const uint64_t *)d_defb, carry.n_records,
                           d_cout);
        kv_excl_scan_launch(d_cout, (uint32_t)L, d_outb, st);
    }
    KV_HIP(hipGetLastError());
    hipError_t re = hipSuccess;
    KvReadback rb;
    const unsigned long long *ctr = rb.add((const unsigned long long *)d_ctr, GN_NCTR, st, &re);
    const uint64_t *n_defs = rb.add((const uint64_t *)d_defb + L, 1, st, &re);
    const uint64_t *id_bytes = rb.add((const uint64_t *)d_idb + L, 1, st, &re);
    const uint64_t *out_bytes = rb.add((const uint64_t *)d_outb + L, 1, st, &re);
    KV_HIP(re);
    KV_HIP(rb.wait(st));
    GnSegmentResult s;
    s.n = n; s.flags = (uint32_t)ctr[0]; s.last_raw = ctr[1]; s.last_defline = (uint32_t)ctr[2]; s.last_id_open = (uint32_t)ctr[3];
    s.last_held = (uint32_t)ctr[4];
    s.n_defs = *n_defs; s.id_bytes = *id_bytes; s.out_bytes = *out_bytes;
    const GnCarry before = carry;
    KV_STEP(gn_carry_next(carry, s));                  // (a decline ends the file here: nothing of this segment is written)
    KV_REQUIRE(carry.out_off <= carry.text_seen, KV_ERR_ARG, "kv_genome_open: more joined text than text");
    KV_STEP(gn_reserve(g, before.out_off, carry.out_off, st));
    KvCarve<3> recs({(size_t)s.n_defs * 8, (size_t)s.n_defs * 8, (size_t)s.id_bytes + 16});
    KV_HIP(recs.from(w.recs));
    uint64_t *d_rseq = recs.at<uint64_t>(0), *d_rid = recs.at<uint64_t>(1);
    uint8_t *d_ids = recs.at<uint8_t>(2);
    {
        KvProfScope prof("k_gn_place");
        hipLaunchKernelGGL(k_gn_place, lgrid, lblock, 0, st, L, (const uint32_t *)d_info, d_pay, (const uint64_t *)d_defb, (const uint64_t *)d_idb,
                           (const uint64_t *)d_outb, before.n_records, before.out_off, before.id_off, (uint8_t *)g->out.p, d_rseq, d_rid, d_dst);
    }
    {
        KvProfScope prof("k_gn_copy");
        hipLaunchKernelGGL(k_gn_copy, dim3(n_chunks), dim3(GN_THREADS), 0, st, text, n, (const uint64_t *)d_base, (const uint64_t *)d_ls, L,
                           (const uint32_t *)d_info, (const uint32_t *)d_pay, (const uint64_t *)d_dst, (uint8_t *)g->out.p, d_ids);
    }
    KV_HIP(hipGetLastError());
    const size_t r0 = g->seq_start.size(), i0 = g->ids.size();
    g->seq_start.resize(r0 + s.n_defs);
    g->id_off.resize(r0 + s.n_defs);
    g->ids.resize(i0 + s.id_bytes);
    if (s.n_defs) {
        KV_HIP(hipMemcpyAsync(g->seq_start.data() + r0, d_rseq, s.n_defs * 8, hipMemcpyDeviceToHost, st));
        KV_HIP(hipMemcpyAsync(g->id_off.data() + r0, d_rid, s.n_defs * 8, hipMemcpyDeviceToHost, st));
    }
    if (s.id_bytes) KV_HIP(hipMemcpyAsync(&g->ids[i0], d_ids, s.id_bytes, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    ++g->n_segments;
    return KV_OK;
}

// the next segment's text behind the held bytes, in the other text buffer; *n = held + fresh (0: the file has ended)
int gn_next_text(GnWork &w, int container, uint64_t segment, const GnCarry &carry, uint64_t prev_n, uint64_t *pos, uint64_t *n, hipStream_t st)
{
    *n = 0;
    uint64_t fresh = 0, m0 = *pos, m1 = *pos;
    if (container == 0) fresh = gn_plain_take(*pos, w.image_size, segment);
    else if (container == 1) m1 = gn_bgzf_take(w.isize.data(), w.isize.size(), m0, segment, &fresh);
    else {
        bool last = false;
        while (fresh == 0 && !kv_gunzip_done(w.gz)) KV_STEP(kv_gunzip_decode(w.gz, segment, &fresh, &last));
    }
    if (fresh == 0 && !(container == 1 && m1 > m0)) return KV_OK;
    const int nxt = w.cur ^ 1;
    KV_HIP(w.text[nxt].need(kv_round_up(carry.held + fresh + 64, 4096)));
    uint8_t *text = (uint8_t *)w.text[nxt].p;
    if (carry.held) KV_HIP(hipMemcpyAsync(text, (const uint8_t *)w.text[w.cur].p + (prev_n - carry.held), carry.held, hipMemcpyDeviceToDevice, st));
    if (container == 0) {
        KV_HIP(hipMemcpyAsync(text + carry.held, w.image + *pos, fresh, hipMemcpyHostToDevice, st));
        *pos += fresh;
    } else if (container == 1) {
        const uint64_t c0 = w.members[m0].in_off, c1 = w.members[m1 - 1].in_off + w.members[m1 - 1].in_len;
        KV_HIP(w.comp.need(kv_round_up(c1 - c0 + KV_INFLATE_SLACK, 4096)));
        KV_HIP(hipMemcpyAsync(w.comp.p, w.image + c0, c1 - c0, hipMemcpyHostToDevice, st));
        KV_HIP(hipMemsetAsync((uint8_t *)w.comp.p + (c1 - c0), 0, KV_INFLATE_SLACK, st));
        std::vector<uint64_t> text_off(m1 - m0);
        uint64_t at = carry.held;
        for (uint64_t i = m0; i < m1; ++i) { text_off[i - m0] = at; at += w.members[i].isize; }
        KV_STEP(kv_bgzf_inflate((const uint8_t *)w.comp.p, c0, w.members.data() + m0, m1 - m0, text_off.data(), text, w.scratch));
        *pos = m1;
    } else {
        KV_STEP(kv_gunzip_emit(w.gz, text + carry.held));
    }
    w.cur = nxt;
    *n = carry.held + fresh;
    return KV_OK;
}

}  // namespace

extern "C" int kv_genome_open(const char *path, uint64_t segment_text, kv_genome **out)
{
    KV_REQUIRE(path && out, KV_ERR_ARG, "kv_genome_open: null argument");
    *out = nullptr;
    GnWork w;
    w.fd = open(path, O_RDONLY);
    KV_REQUIRE(w.fd >= 0, KV_ERR_IO, "cannot open reference file %s", path);
    struct stat sb;
    KV_REQUIRE(fstat(w.fd, &sb) == 0 && S_ISREG(sb.st_mode), KV_ERR_TYPE, "%s is not a regular file (read on the host)", path);
    if (sb.st_size > 0) {
        void *map = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, w.fd, 0);
        KV_REQUIRE(map != MAP_FAILED, KV_ERR_IO, "cannot map reference file %s", path);
        w.image = (const uint8_t *)map;
        w.image_size = (size_t)sb.st_size;
    }
    hipStream_t st = kv_stream();
    kv_genome *g = new kv_genome;
    struct Guard { kv_genome *g; ~Guard() { delete g; } } guard{g};
    const uint64_t segment = gn_segment_text(segment_text);
    uint64_t known_text = w.image_size;
    if (w.image_size >= 2 && w.image[0] == 0x1f && w.image[1] == 0x8b) {
        int is_bgzf = 0;
        KV_STEP(kv_bgzf_index(w.image, w.image_size, &w.members, &is_bgzf));
        if (is_bgzf) {
            g->container = 1;
            known_text = 0;
            for (const KvBgzfMember &m : w.members) { w.isize.push_back(m.isize); known_text += m.isize; }
        } else {
            g->container = 2;
            w.members.clear();
            w.gz = kv_gunzip_open(w.image, w.image_size, &w.gz_arenas);
            KV_REQUIRE(w.gz, KV_ERR_TYPE, "%s: not a gzip stream the device inflates (read on the host)", path);
            known_text = std::min<uint64_t>(4 * (uint64_t)w.image_size, segment);
        }
    }
    KV_STEP(gn_reserve(g, 0, known_text, st));
    GnCarry carry;
    uint64_t pos = 0, n = 0;
    for (;;) {
        uint64_t got = 0;
        KV_STEP(gn_next_text(w, g->container, segment, carry, n, &pos, &got, st));
        if (got == 0) break;
        n = got;
        if (n == carry.held) continue;                 // members of no text
        KV_STEP(gn_segment(g, w, n, carry, st));
    }
    KV_STEP(gn_carry_finish(carry));
    g->total = carry.out_off;
    g->text_seen = carry.text_seen;
    const uint64_t nrec = carry.n_records;
    KV_REQUIRE(g->seq_start.size() == nrec && g->ids.size() == carry.id_off, KV_ERR_ARG, "kv_genome_open: the record table does not add up");
    g->id_off.push_back(carry.id_off);
    g->seq_len.resize(nrec);
    for (uint64_t r = 0; r < nrec; ++r) g->seq_len[r] = (r + 1 < nrec ? g->seq_start[r + 1] - 1 : g->total) - g->seq_start[r];
    // the bytes behind the text that a 16-byte load of the scan may touch are zero
    KV_HIP(hipMemsetAsync((uint8_t *)g->out.p + g->total, 0, std::min<uint64_t>(g->out.bytes - g->total, 64), st));
    KV_HIP(hipStreamSynchronize(st));
    guard.g = nullptr;
    *out = g;
    return KV_OK;
}

extern "C" int kv_genome_info(kv_genome *g, uint64_t *n_seqs, uint64_t *text_bytes, uint64_t *stats, const char **ids, const uint64_t **id_offs,
                              const uint64_t **starts, const uint64_t **lengths)
{
    KV_REQUIRE(g, KV_ERR_ARG, "kv_genome_info: null handle");
    if (n_seqs) *n_seqs = g->seq_start.size();
    if (text_bytes) *text_bytes = g->total;
    if (stats) { stats[0] = (uint64_t)g->container; stats[1] = g->n_segments; stats[2] = g->text_seen; stats[3] = g->out.bytes; }
    if (ids) *ids = g->ids.data();
    if (id_offs) *id_offs = g->id_off.data();
    if (starts) *starts = g->seq_start.data();
    if (lengths) *lengths = g->seq_len.data();
    return KV_OK;
}

extern "C" int kv_genome_fetch(kv_genome *g, const uint64_t *global_start, const uint64_t *len, uint64_t n, char *out, uint64_t *out_offs)
{
    KV_REQUIRE(g && out_offs && (n == 0 || (global_start && len)), KV_ERR_ARG, "kv_genome_fetch: null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    out_offs[0] = 0;
    if (n == 0) return KV_OK;
    std::vector<uint64_t> ext(2 * n);
    for (uint64_t i = 0; i < n; ++i) {                  // slices clip at the text's end, as Python's do
        const uint64_t a = std::min(global_start[i], g->total), b = a + std::min(len[i], g->total - a);
        ext[2 * i] = a; ext[2 * i + 1] = b;
        out_offs[i + 1] = out_offs[i] + (b - a);
    }
    const uint64_t bytes = out_offs[n];
    if (bytes == 0) return KV_OK;
    KV_REQUIRE(out, KV_ERR_ARG, "kv_genome_fetch: null argument");
    hipStream_t st = kv_stream();
    KvCarve<3> fetch({(size_t)n * 16, (size_t)n * 8, (size_t)bytes + 16});
    KV_HIP(fetch.from(g->fetch));
    uint64_t *d_ext = fetch.at<uint64_t>(0), *d_dst = fetch.at<uint64_t>(1);
    uint8_t *d_out = fetch.at<uint8_t>(2);
    KV_HIP(hipMemcpyAsync(d_ext, ext.data(), n * 16, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_dst, out_offs, n * 8, hipMemcpyHostToDevice, st));
    {
        KvProfScope prof("k_record_copy");
        hipLaunchKernelGGL(k_record_copy, dim3((unsigned)std::min<uint64_t>(n, 16384)), dim3(64), 0, st, (const uint8_t *)g->out.p, (const uint64_t *)d_ext,
                           (const uint64_t *)d_dst, n, d_out);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}

extern "C" int kv_genome_close(kv_genome *g)
{
    if (g) {
        (void)hipStreamSynchronize(kv_stream());
        delete g;
    }
    return KV_OK;
}
