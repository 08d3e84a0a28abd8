// kv_align.hip -- global alignment of contigs against reference cutouts, the first half of `kevlar call` (kevlar/alignment.pyx,
// src/align.c, third-party/ksw2/ksw2_extz.c as the reference calls it: w = -1, zdrop = -1, flag = 0 -- nothing banded, nothing
// dropped, score = H(tlen - 1, qlen - 1), traceback from that corner).  Integer dynamic programming with affine gaps whose
// tie-breaking decides the CIGAR; the rule is written out in DESIGN.md section 10 and restated in tests/align_common.py.
//
// One wavefront per job.  The query is cut into strips of ALN_STRIP = 64 lanes x ALN_COLS columns; a lane keeps H (the diagonal
// value) and E of its columns in registers and runs one target row behind its left neighbour, from which it receives that row's
// (H, F, target code) by a one-lane DPP shift.  Lane 0 takes them from the row's initial values (first strip) or from the
// boundary buffer the last lane of the previous strip wrote.  One step of the wave therefore computes an anti-diagonal of
// 64 x ALN_COLS cells, and every lane has ALN_COLS direction bytes to store: z is kept in that order,
//     z(i, j) at  (strip * (tlen + 63) + i + lane) * ALN_STRIP + j % ALN_STRIP,   strip = j / ALN_STRIP, lane = j % ALN_STRIP / ALN_COLS
// so a step's store is ALN_STRIP contiguous bytes.  The traceback (lane 0 of the same wave, right after the last strip) computes
// the same address.  It writes its runs back to front into a scratch list, claims room in the caller's pool with one atomic
// add and the wave copies the runs there in forward order.
// Host half: what a batch must satisfy is in kv_seq_jobs.h, the order of the jobs, the launches and every job's place in a launch's
// working memory in kv_align_plan.h (both free of HIP and tested without a device); kv_align_batch is the list of the steps.
#include "kv_device.h"
#include "kv_align_plan.h"      // AlignJob, ALN_LANES / ALN_COLS / ALN_STRIP, aln_z_bytes, aln_layout

namespace {

static_assert(ALN_COLS == 4, "a lane's direction bytes of one row are one 32-bit word");

struct AlignParams {
    const AlignJob *jobs;
    const uint8_t *tbases, *qbases;
    uint8_t *z;
    int2 *bnd;
    uint32_t *tmp;
    int a, b, e, oe;            // match, -|mismatch|, gap extension, gap open + extension
    int32_t *scores;            // per job index
    uint64_t *run_off;
    uint32_t *run_cnt;
    uint32_t *pool;
    uint64_t cap;
    unsigned long long *ctr;    // [0] runs claimed so far, [1] ticks of the fill, [2] ticks of the traceback and copy
};

// A/a = 0, C/c = 1, G/g = 2, T/t = 3, every other byte 4
__device__ __forceinline__ int aln_code(uint32_t byte)
{
    const uint32_t u = byte & 0xDFu;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

// the value of the lane below (lane 0 keeps its own): a DPP move, no LDS
__device__ __forceinline__ int aln_from_left(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }

__device__ __forceinline__ uint64_t aln_zaddr(uint32_t tlen, uint32_t i, uint32_t j)
{
    const uint32_t strip = j / ALN_STRIP, within = j % ALN_STRIP;
    return ((uint64_t)strip * (tlen + ALN_LANES - 1) + i + within / ALN_COLS) * ALN_STRIP + within;
}

__global__ __launch_bounds__(ALN_LANES) void k_align(AlignParams p)
{
    const AlignJob jb = p.jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const int tlen = (int)jb.tlen, qlen = (int)jb.qlen;
    const uint8_t *T = p.tbases + jb.toff, *Q = p.qbases + jb.qoff;
    uint8_t *zbytes = p.z + jb.zoff;
    uint32_t *z = reinterpret_cast<uint32_t *>(zbytes);
    int2 *bnd0 = p.bnd + jb.bndoff, *bnd1 = bnd0 + tlen;
    const int a = p.a, b = p.b, e = p.e, oe = p.oe;
    const int nstrips = (qlen + ALN_STRIP - 1) / ALN_STRIP;
    const int nsteps = tlen + ALN_LANES - 1;
    const unsigned long long tick0 = wall_clock64();

    int hd[ALN_COLS], ee[ALN_COLS], qc[ALN_COLS];
    int h_out = 0, f_out = 0, t_out = 4;
    for (int s = 0; s < nstrips; ++s) {
#pragma unroll
        for (int c = 0; c < ALN_COLS; ++c) {
            const int j = s * ALN_STRIP + lane * ALN_COLS + c;
            int code = 4;                                    // columns behind the query compute along and are never read
            if (j < qlen) {
                code = aln_code(jb.rev ? Q[qlen - 1 - j] : Q[j]);
                if (jb.rev && code < 4) code = 3 - code;
            }
            qc[c] = code;
            hd[c] = j == 0 ? 0 : -(oe + e * (j - 1));
            ee[c] = -(2 * oe + e * j);
        }
        const int2 *bin = (s & 1) ? bnd1 : bnd0;
        int2 *bout = (s & 1) ? bnd0 : bnd1;
        const bool carry_in = s > 0, carry_out = s + 1 < nstrips;
        uint32_t *zs = z + (uint64_t)s * nsteps * ALN_LANES;
        int blk_t = 4, blk_h = 0, blk_f = 0;
        h_out = f_out = 0;
        t_out = 4;
        // 64 rows at a time: what lane 0 is fed over the next 64 steps is loaded here, one row per lane, so that the steps
        // themselves wait for no memory (their z stores stay in flight)
        for (int t0 = 0; t0 < nsteps; t0 += ALN_LANES) {
            const int r = t0 + lane;
            blk_t = r < tlen ? aln_code(T[r]) : 4;
            if (carry_in && r < tlen) {
                const int2 v = bin[r];
                blk_h = v.x;
                blk_f = v.y;
            }
            const int t_end = min(t0 + ALN_LANES, nsteps);
            for (int t = t0; t < t_end; ++t) {
                int h1 = aln_from_left(h_out), f = aln_from_left(f_out), tc = aln_from_left(t_out);
                const int src = t & (ALN_LANES - 1);
                const int first_t = __builtin_amdgcn_readlane(blk_t, src);
                const int first_h = __builtin_amdgcn_readlane(blk_h, src);
                const int first_f = __builtin_amdgcn_readlane(blk_f, src);
                if (lane == 0) {
                    tc = first_t;
                    h1 = carry_in ? first_h : -(oe + e * t);
                    f = carry_in ? first_f : -(2 * oe + e * t);
                }
                const int i = t - lane;
                if (i >= 0 && i < tlen) {
                    uint32_t zw = 0;
#pragma unroll
                    for (int c = 0; c < ALN_COLS; ++c) {
                        int h = hd[c];
                        hd[c] = h1;
                        int sc = tc == qc[c] ? a : b;
                        sc = max(tc, qc[c]) > 3 ? 0 : sc;
                        h += sc;
                        int en = ee[c];
                        uint32_t d = h >= en ? 0u : 1u;
                        h = max(h, en);
                        d = h >= f ? d : 2u;
                        h = max(h, f);
                        h1 = h;
                        h -= oe;
                        en -= e;
                        d |= en > h ? 0x08u : 0u;
                        en = max(en, h);
                        ee[c] = en;
                        f -= e;
                        d |= f > h ? 0x10u : 0u;
                        f = max(f, h);
                        zw |= d << (8 * c);
                    }
                    zs[(uint64_t)t * ALN_LANES + lane] = zw;
                    h_out = h1;
                    f_out = f;
                    t_out = tc;
                    if (carry_out && lane == ALN_LANES - 1) bout[i] = make_int2(h1, f);
                }
            }
        }
        __syncthreads();        // one wave: the boundary rows and z are visible to all its lanes
    }
    // H(tlen - 1, qlen - 1): a lane's last row leaves H of column c in hd[c + 1], of its last column in h_out
    const int jl = (qlen - 1) % ALN_STRIP, cl = jl % ALN_COLS;
    int corner = h_out;
#pragma unroll
    for (int c = 0; c + 1 < ALN_COLS; ++c) corner = cl == c ? hd[c + 1] : corner;
    const int score = __shfl(corner, jl / ALN_COLS);
    const unsigned long long tick1 = wall_clock64();

    uint32_t nruns = 0;
    const uint32_t bound = jb.tlen + jb.qlen;
    uint32_t *tmp = p.tmp + jb.tmpoff;
    if (lane == 0) {
        int i = tlen - 1, j = qlen - 1, state = 0;
        uint32_t cur_op = 3, cur_len = 0;                    // ops: 0 M, 1 I, 2 D
        while (i >= 0 && j >= 0) {
            const int t = zbytes[aln_zaddr(jb.tlen, (uint32_t)i, (uint32_t)j)];
            if (state == 0) state = t & 7;
            else if (!((t >> (state + 2)) & 1)) state = 0;
            if (state == 0) state = t & 7;
            const uint32_t op = state == 0 ? 0u : state == 1 ? 2u : 1u;
            if (op != cur_op) {
                if (cur_len) tmp[bound - 1 - nruns++] = cur_len << 4 | cur_op;
                cur_op = op;
                cur_len = 0;
            }
            ++cur_len;
            if (op != 1u) --i;
            if (op != 2u) --j;
        }
        if (i >= 0) {
            if (cur_op != 2u) {
                if (cur_len) tmp[bound - 1 - nruns++] = cur_len << 4 | cur_op;
                cur_op = 2u;
                cur_len = 0;
            }
            cur_len += (uint32_t)(i + 1);
        }
        if (j >= 0) {
            if (cur_op != 1u) {
                if (cur_len) tmp[bound - 1 - nruns++] = cur_len << 4 | cur_op;
                cur_op = 1u;
                cur_len = 0;
            }
            cur_len += (uint32_t)(j + 1);
        }
        if (cur_len) tmp[bound - 1 - nruns++] = cur_len << 4 | cur_op;
    }
    __syncthreads();
    nruns = __shfl(nruns, 0);
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(&p.ctr[0], (unsigned long long)nruns);
    at = __shfl(at, 0);
    if (at + nruns <= p.cap)
        for (uint32_t r = lane; r < nruns; r += ALN_LANES) p.pool[at + r] = tmp[bound - nruns + r];
    if (lane == 0) {
        p.scores[jb.index] = score;
        p.run_off[jb.index] = at;
        p.run_cnt[jb.index] = nruns;
        atomicAdd(&p.ctr[1], tick1 - tick0);
        atomicAdd(&p.ctr[2], wall_clock64() - tick1);
    }
}

unsigned long long g_align_stats[4] = {0, 0, 0, 0};    // of the last kv_align_batch: launches, fill ticks, traceback ticks, cells

}  // namespace

extern "C" int kv_align_z_bytes(uint32_t tlen, uint32_t qlen, uint64_t *bytes)
{
    KV_REQUIRE(bytes, KV_ERR_ARG, "kv_align_z_bytes: null argument");
    KV_REQUIRE(tlen >= 1 && qlen >= 1 && tlen <= KV_SEQ_MAX_LEN && qlen <= KV_SEQ_MAX_LEN, KV_ERR_ARG,
               "alignment of a %u-base target and a %u-base query: lengths must be 1..%u", tlen, qlen, KV_SEQ_MAX_LEN);
    *bytes = aln_z_bytes(tlen, qlen);
    return KV_OK;
}

extern "C" int kv_align_plan(const uint32_t *tlens, const uint32_t *qlens, uint64_t n_jobs, uint64_t z_budget, uint32_t *order,
                             uint64_t *launch_ends, uint64_t *n_launches)
{
    KV_REQUIRE(n_launches && (n_jobs == 0 || (tlens && qlens && order && launch_ends)), KV_ERR_ARG, "kv_align_plan: null argument");
    KV_REQUIRE(n_jobs < 0x7FFFFFFFull, KV_ERR_ARG, "kv_align_plan: %llu jobs", (unsigned long long)n_jobs);
    *n_launches = 0;
    std::vector<KvSeqJob> table(n_jobs);
    for (uint64_t k = 0; k < n_jobs; ++k) {
        KV_STEP(kv_seq_lengths("alignment", k, tlens[k], qlens[k]));
        table[k] = KvSeqJob{0, 0, tlens[k], qlens[k], 0, 0, 0};
    }
    AlignLayout lay;
    KV_STEP(aln_layout(table, z_budget, lay));
    for (uint64_t k = 0; k < n_jobs; ++k) order[k] = lay.descs[k].index;
    std::copy(lay.ends.begin(), lay.ends.end(), launch_ends);
    *n_launches = lay.ends.size();
    return KV_OK;
}

extern "C" int kv_align_batch(const char *tbases, const uint64_t *toffsets, uint64_t n_targets, const char *qbases,
                              const uint64_t *qoffsets, uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs, int match,
                              int mismatch, int gapopen, int gapextend, uint64_t z_budget, int32_t *scores, uint64_t *run_offsets,
                              uint32_t *run_counts, uint32_t *runs, uint64_t capacity, uint64_t *n_runs)
{
    KV_REQUIRE(n_runs && (n_jobs == 0 || (tbases && qbases && scores && run_offsets && run_counts)) && (capacity == 0 || runs), KV_ERR_ARG,
               "kv_align_batch: null argument");
    if (mismatch < 0) mismatch = -mismatch;
    KV_REQUIRE(match >= 0 && match <= 127 && mismatch <= 127 && gapopen >= 0 && gapopen <= 127 && gapextend >= 0 && gapextend <= 127,
               KV_ERR_ARG, "alignment scores must lie in 0..127 (match %d, mismatch %d, gap open %d, gap extension %d)", match, mismatch, gapopen, gapextend);
    *n_runs = 0;
    std::vector<KvSeqJob> table;
    KV_STEP(kv_seq_jobs("kv_align_batch", "alignment", toffsets, n_targets, qoffsets, n_queries, jobs, n_jobs, table));
    AlignLayout lay;
    KV_STEP(aln_layout(table, z_budget, lay));
    g_align_stats[0] = g_align_stats[1] = g_align_stats[2] = g_align_stats[3] = 0;
    if (n_jobs == 0) return KV_OK;

    // carve and upload: one device buffer, its pieces in the order of their sizes
    enum { AB_Z, AB_BND, AB_TMP, AB_T, AB_Q, AB_JOBS, AB_SCORES, AB_OFF, AB_CNT, AB_POOL, AB_CTR, AB_PIECES };
    hipStream_t st = kv_stream();
    const uint64_t tbytes = toffsets[n_targets], qbytes = qoffsets[n_queries];
    const size_t sizes[AB_PIECES] = {lay.z_max, lay.bnd_max * sizeof(int2), lay.tmp_max * 4, tbytes, qbytes, n_jobs * sizeof(AlignJob),
                                     n_jobs * 4, n_jobs * 8, n_jobs * 4, capacity * 4, 64};
    KvDevBuf buf;
    KvCarve<AB_PIECES> d(sizes);
    const hipError_t e = d.from(buf);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "alignment buffers (%llu bytes of direction bytes) allocation failed: %s",
               (unsigned long long)lay.z_max, hipGetErrorString(e));
    AlignParams p;
    p.tbases = d.at<uint8_t>(AB_T); p.qbases = d.at<uint8_t>(AB_Q); p.z = d.at<uint8_t>(AB_Z); p.bnd = d.at<int2>(AB_BND); p.tmp = d.at<uint32_t>(AB_TMP);
    p.a = match; p.b = -mismatch; p.e = gapextend; p.oe = gapopen + gapextend; p.cap = capacity; p.ctr = d.at<unsigned long long>(AB_CTR);
    p.scores = d.at<int32_t>(AB_SCORES); p.run_off = d.at<uint64_t>(AB_OFF); p.run_cnt = d.at<uint32_t>(AB_CNT); p.pool = d.at<uint32_t>(AB_POOL);
    KV_HIP(hipMemcpyAsync(d.at<void>(AB_T), tbases, tbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d.at<void>(AB_Q), qbases, qbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d.at<void>(AB_JOBS), lay.descs.data(), n_jobs * sizeof(AlignJob), hipMemcpyHostToDevice, st));
    KV_HIP(hipMemsetAsync(p.ctr, 0, 64, st));
    {   // launch per plan chunk; launches share z: one after the other on the stream
        KvProfScope prof("k_align");
        uint64_t k = 0;
        for (const uint64_t end : lay.ends) {
            p.jobs = d.at<AlignJob>(AB_JOBS) + k;
            hipLaunchKernelGGL(k_align, dim3((unsigned)(end - k)), dim3(ALN_LANES), 0, st, p);
            k = end;
        }
    }
    KV_HIP(hipGetLastError());
    // fetch; the runs only when the caller's pool held them all
    unsigned long long ctr[3] = {0, 0, 0};
    KV_HIP(hipMemcpyAsync(ctr, p.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(scores, p.scores, n_jobs * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(run_offsets, p.run_off, n_jobs * 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(run_counts, p.run_cnt, n_jobs * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    *n_runs = ctr[0];
    if (ctr[0] && ctr[0] <= capacity) {
        KV_HIP(hipMemcpyAsync(runs, p.pool, ctr[0] * 4, hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
    }
    g_align_stats[0] = lay.ends.size(); g_align_stats[1] = ctr[1]; g_align_stats[2] = ctr[2]; g_align_stats[3] = lay.cells;
    return KV_OK;
}

extern "C" int kv_align_stats(uint64_t *stats_out)
{
    KV_REQUIRE(stats_out, KV_ERR_ARG, "kv_align_stats: null argument");
    for (int k = 0; k < 4; ++k) stats_out[k] = g_align_stats[k];
    return KV_OK;
}
