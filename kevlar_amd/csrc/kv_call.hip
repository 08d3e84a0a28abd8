// kv_call.hip -- the per-base loops of `kevlar call` behind the alignment (kevlar/cigar.py:46-71, kevlar/varmap.py:49-54, 157-161,
// 231-317): for every aligned (cutout, contig, strand) job the end check of the tokenizer, the class of its CIGAR, the
// mismatches of the match blocks it scans and the number of interesting k-mers present in the window of every call it yields.
// The contract is in include/kvsketch.h, the rules in DESIGN.md section 11, the plain-Python restatement in tests/call_common.py.
//
// Host half: the runs of every job become a descriptor -- the candidate of the end check and, for both of its answers, the class
// and the match blocks to scan (kv_call_plan.h) -- and everything that is wrong with the arguments is found (kv_seq_jobs.h,
// kv_call_plan.h; both free of HIP and tested without a device), before anything touches the device; the entry is a list of
// steps.  Device half: one wavefront per job, so a 10 000-base job keeps one wave busy and no other.  A block is a window of the
// two texts with at most one seam (the folded block of the end check is the concatenation of two segments which are apart in one
// of the texts); lanes walk it 64 positions at a time and ballots give the counts and the first four positions in order.  A
// call's window is up to three pieces of the query; the lanes are its start positions and compare an interesting k-mer and its
// reverse complement base by base, so a hit is a hit on the bases.
#include "kv_device.h"
#include "kv_call_plan.h"       // CallBlock, CallShape, CallJob, CALL_OP_*, call_plan_job

namespace {

#define CALL_LANES 64

static_assert(KV_CALL_RECORD_WORDS == 32, "include/kvsketch.h states the record");

struct CallParams {
    const CallJob *jobs;
    const uint8_t *tbases, *qbases;
    const uint32_t *ikmers;     // (offset, ksize) pairs
    const uint8_t *comp;        // the 256-byte complement table
    uint32_t *records;
    uint32_t ksize, mindist;
};

struct CallWindow {             // piece A: block a, positions [a0, a0 + alen); piece B: query bytes [bq, bq + blen); piece C:
    uint32_t a, a0, alen;       // block 1, positions [0, clen)
    uint32_t bq, blen;
    uint32_t clen;
};

struct CallCtx {
    const uint8_t *T, *Q;
    const uint8_t *comp;        // in LDS
    uint32_t qlen, rev;
    CallBlock blk[2];
};

// byte i of the query as the job reads it: the contig, or its reverse complement
__device__ __forceinline__ uint32_t call_q(const CallCtx &c, uint32_t i)
{
    return c.rev ? c.comp[c.Q[c.qlen - 1 - i]] : c.Q[i];
}

// (selects, not an index: the two blocks stay in registers)
__device__ __forceinline__ uint32_t call_blk_q(const CallCtx &c, uint32_t b, uint32_t p)
{
    const uint32_t qpos = b ? c.blk[1].qpos : c.blk[0].qpos, seam = b ? c.blk[1].seam : c.blk[0].seam, gap = b ? c.blk[1].qgap : c.blk[0].qgap;
    return call_q(c, qpos + p + (p >= seam ? gap : 0u));
}

__device__ __forceinline__ uint32_t call_blk_t(const CallCtx &c, uint32_t b, uint32_t p)
{
    const uint32_t tpos = b ? c.blk[1].tpos : c.blk[0].tpos, seam = b ? c.blk[1].seam : c.blk[0].seam, gap = b ? c.blk[1].tgap : c.blk[0].tgap;
    return c.T[tpos + p + (p >= seam ? gap : 0u)];
}

__device__ __forceinline__ uint32_t call_win(const CallCtx &c, const CallWindow &w, uint32_t i)
{
    if (i < w.alen) return call_blk_q(c, w.a, w.a0 + i);
    i -= w.alen;
    if (i < w.blen) return call_q(c, w.bq + i);
    return call_blk_q(c, 1u, i - w.blen);
}

// kevlar/varmap.py:309-317: the interesting k-mers whose sequence, or the reverse complement of it, lies somewhere in the window
__device__ uint32_t call_count_ikmers(const CallCtx &c, const CallWindow &w, const uint32_t *ikmers, uint64_t begin, uint64_t end, int lane)
{
    const uint32_t wlen = w.alen + w.blen + w.clen;
    uint32_t n = 0;
    for (uint64_t a = begin; a < end; ++a) {
        const uint32_t off = ikmers[2 * a], ks = ikmers[2 * a + 1];
        if (ks > wlen) continue;
        const uint32_t nstarts = wlen - ks + 1;
        const uint8_t *K = c.Q + off;                       // of the contig as given, whatever the strand of the job
        bool found = false;
        for (uint32_t s0 = 0; s0 < nstarts && !found; s0 += CALL_LANES) {
            const uint32_t s = s0 + (uint32_t)lane;
            bool hit = false;
            if (s < nstarts) {
                bool fwd = true, rc = true;
                for (uint32_t j = 0; j < ks && (fwd || rc); ++j) {
                    const uint32_t x = call_win(c, w, s + j);
                    fwd = fwd && x == K[j];
                    rc = rc && x == c.comp[K[ks - 1 - j]];
                }
                hit = fwd || rc;
            }
            found = __ballot(hit) != 0ull;
        }
        n += found ? 1u : 0u;
    }
    return n;
}

__global__ __launch_bounds__(CALL_LANES) void k_call_scan(CallParams p)
{
    __shared__ uint32_t comp_words[64];
    const int lane = threadIdx.x;
    const CallJob &jb = p.jobs[blockIdx.x];
    comp_words[lane] = reinterpret_cast<const uint32_t *>(p.comp)[lane];
    __syncthreads();

    CallCtx c;
    c.T = p.tbases + jb.toff;
    c.Q = p.qbases + jb.qoff;
    c.comp = reinterpret_cast<const uint8_t *>(comp_words);
    c.qlen = jb.qlen;
    c.rev = jb.rev;

    // kevlar/cigar.py:46-71: does `prev + last` start with the other sequence's last block?
    uint32_t folded = 0;
    const uint32_t fold_len = jb.fold_len;
    if (fold_len) {
        bool same = true;
        for (uint32_t i0 = 0; i0 < fold_len && same; i0 += CALL_LANES) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool differ = i < fold_len && c.T[jb.fold_t + i] != call_q(c, jb.fold_q + i);
            same = __ballot(differ) == 0ull;
        }
        folded = same ? 1u : 0u;
    }
    const CallShape &sh = jb.shape[folded];
    c.blk[0] = sh.scan[0];
    c.blk[1] = sh.scan[1];
    const uint32_t ksize = p.ksize, mindist = p.mindist;

    // kevlar/varmap.py:241-247: the mismatches of a block of at least ksize bases, those near its ends counted apart
    uint32_t trimmed[2] = {0, 0}, kept[2] = {0, 0};
    uint32_t pos[2][4] = {{~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}};
#pragma unroll
    for (uint32_t b = 0; b < 2; ++b) {
        const uint32_t len = c.blk[b].len;
        if (len == 0 || len < ksize) continue;
        for (uint32_t i0 = 0; i0 < len; i0 += CALL_LANES) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool differ = i < len && call_blk_t(c, b, i) != call_blk_q(c, b, i);
            const bool terminal = mindist != 0 && (i < mindist || len - i < mindist);
            trimmed[b] += (uint32_t)__popcll(__ballot(differ && terminal));
            unsigned long long keep = __ballot(differ && !terminal);
            uint32_t at = kept[b];
            kept[b] += (uint32_t)__popcll(keep);
            for (; at < 4 && keep; ++at, keep &= keep - 1) {
                const uint32_t where = i0 + (uint32_t)__builtin_ctzll(keep);
#pragma unroll
                for (uint32_t s = 0; s < 4; ++s) pos[b][s] = s == at ? where : pos[b][s];
            }
        }
    }

    // the IKMERS number of every call, in the reference's order: the indel, the left flank's SNVs, the right flank's
    uint32_t ik[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (sh.cls == KV_CALL_INDEL) {
        // kevlar/varmap.py:281-296: the last ksize - 1 bases of the left flank (all of it when ksize is 1, as a slice from -0 is),
        // the inserted bases, the first ksize - 1 of the right flank
        CallWindow w;
        const uint32_t l0 = c.blk[0].len, l1 = c.blk[1].len, k1 = ksize - 1;
        w.a = 0;
        w.a0 = (k1 == 0 || k1 >= l0) ? 0u : l0 - k1;
        w.alen = l0 - w.a0;
        w.bq = sh.indel_qpos;
        w.blen = sh.indel_op == CALL_OP_I ? sh.indel_len : 0u;
        w.clen = k1 < l1 ? k1 : l1;
        ik[0] = call_count_ikmers(c, w, p.ikmers, jb.ik_begin, jb.ik_end, lane);
    }
    if (sh.cls != KV_CALL_NONE) {
#pragma unroll
        for (uint32_t b = 0; b < 2; ++b) {
            if (kept[b] < 1 || kept[b] > 4) continue;
            const uint32_t len = c.blk[b].len;
#pragma unroll
            for (uint32_t s = 0; s < 4; ++s) {
                if (s >= kept[b]) continue;
                // kevlar/varmap.py:263-265
                const uint32_t at = pos[b][s];
                const uint32_t lo = at + 1 >= ksize ? at + 1 - ksize : 0u;
                const uint32_t hi = at + ksize < len ? at + ksize : len;
                CallWindow w;
                w.a = b;
                w.a0 = lo;
                w.alen = hi - lo;
                w.bq = 0;
                w.blen = 0;
                w.clen = 0;
                ik[1 + 4 * b + s] = call_count_ikmers(c, w, p.ikmers, jb.ik_begin, jb.ik_end, lane);
            }
        }
    }

    // the record: one lane a word
    uint32_t word = 0;
    if (lane == 0) word = folded;
    if (lane == 1) word = sh.cls;
#pragma unroll
    for (uint32_t b = 0; b < 2; ++b) {
        const int base = 2 + 7 * (int)b;
        if (lane == base) word = c.blk[b].len;
        if (lane == base + 1) word = trimmed[b];
        if (lane == base + 2) word = kept[b];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (lane == base + 3 + s) word = pos[b][s];
    }
#pragma unroll
    for (int s = 0; s < 9; ++s)
        if (lane == 16 + s) word = ik[s];
    if (lane < KV_CALL_RECORD_WORDS) p.records[(uint64_t)jb.index * KV_CALL_RECORD_WORDS + lane] = word;
}

void call_comp_table(uint8_t *table)
{
    // kevlar_amd.sequence.revcom: the IUPAC codes, lower case to upper, every other byte itself
    const char *from = "ATUGCYRSWKMBDHVNatugcyrswkmbdhvn", *to = "TAACGRYSWMKVHDBNTAACGRYSWMKVHDBN";
    for (int b = 0; b < 256; ++b) table[b] = (uint8_t)b;
    for (int k = 0; from[k]; ++k) table[(uint8_t)from[k]] = (uint8_t)to[k];
}

}  // namespace

extern "C" int kv_call_scan(const char *tbases, const uint64_t *toffsets, uint64_t n_targets, const char *qbases,
                            const uint64_t *qoffsets, uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs,
                            const uint64_t *run_offsets, const uint32_t *run_counts, const uint32_t *runs, uint64_t n_runs,
                            const uint64_t *ik_offsets, const uint32_t *ikmers, int ksize, int mindist, uint32_t *records)
{
    KV_REQUIRE(ik_offsets && (n_jobs == 0 || (tbases && qbases && run_offsets && run_counts && records)) && (n_runs == 0 || runs), KV_ERR_ARG,
               "kv_call_scan: null argument");
    KV_REQUIRE(ksize >= 1 && ksize <= (int)KV_SEQ_MAX_LEN && mindist >= 0 && mindist <= (int)KV_SEQ_MAX_LEN, KV_ERR_ARG,
               "kv_call_scan: ksize %d (at least 1) and mindist %d (at least 0)", ksize, mindist);
    std::vector<KvSeqJob> table;
    KV_STEP(kv_seq_jobs("kv_call_scan", "call", toffsets, n_targets, qoffsets, n_queries, jobs, n_jobs, table));
    KV_STEP(kv_seq_ikmers("kv_call_scan", qoffsets, n_queries, ik_offsets, ikmers));
    std::vector<CallJob> descs;
    KV_STEP(call_plan_jobs(table, ik_offsets, run_offsets, run_counts, runs, n_runs, descs));
    if (n_jobs == 0) return KV_OK;

    // carve and upload: one device buffer, its pieces in the order of their sizes (no interesting k-mers: that piece is empty and unread)
    enum { CB_T, CB_Q, CB_JOBS, CB_IK, CB_COMP, CB_REC, CB_PIECES };
    uint8_t comp[256];
    call_comp_table(comp);
    hipStream_t st = kv_stream();
    const uint64_t tbytes = toffsets[n_targets], qbytes = qoffsets[n_queries], n_ik = ik_offsets[n_queries];
    const size_t sizes[CB_PIECES] = {tbytes, qbytes, n_jobs * sizeof(CallJob), n_ik * 8, 256, n_jobs * KV_CALL_RECORD_WORDS * 4};
    KvDevBuf buf;
    KvCarve<CB_PIECES> d(sizes);
    const hipError_t e = d.from(buf);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "call scan buffers allocation failed: %s", hipGetErrorString(e));
    CallParams p;
    p.jobs = d.at<CallJob>(CB_JOBS); p.tbases = d.at<uint8_t>(CB_T); p.qbases = d.at<uint8_t>(CB_Q); p.ikmers = d.at<uint32_t>(CB_IK);
    p.comp = d.at<uint8_t>(CB_COMP); p.records = d.at<uint32_t>(CB_REC); p.ksize = (uint32_t)ksize; p.mindist = (uint32_t)mindist;
    KV_HIP(hipMemcpyAsync(d.at<void>(CB_T), tbases, tbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d.at<void>(CB_Q), qbases, qbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d.at<void>(CB_JOBS), descs.data(), n_jobs * sizeof(CallJob), hipMemcpyHostToDevice, st));
    if (n_ik) KV_HIP(hipMemcpyAsync(d.at<void>(CB_IK), ikmers, n_ik * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d.at<void>(CB_COMP), comp, 256, hipMemcpyHostToDevice, st));
    {
        KvProfScope prof("k_call_scan");
        hipLaunchKernelGGL(k_call_scan, dim3((unsigned)n_jobs), dim3(CALL_LANES), 0, st, p);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(records, p.records, n_jobs * KV_CALL_RECORD_WORDS * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}
