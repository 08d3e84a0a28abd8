// kv_call.hip -- the per-base loops of `kevlar call` behind the alignment (kevlar/cigar.py:46-71, kevlar/varmap.py:49-54, 157-161,
// 231-317): for every aligned (cutout, contig, strand) job the end check of the tokenizer, the class of its CIGAR, the
// mismatches of the match blocks it scans and the number of interesting k-mers present in the window of every call it yields.
// The contract is in include/kvsketch.h, the rules in DESIGN.md section 11, the plain-Python restatement in tests/call_common.py.
//
// Host half: the runs of every job become a descriptor -- the candidate of the end check and, for both of its answers, the class
// and the match blocks to scan -- which is integer work on at most six runs a job; everything that is wrong with the arguments
// is found here, before anything touches the device.  Device half: one wavefront per job, so a 10 000-base job keeps one wave
// busy and no other.  A block is a window of the two texts with at most one seam (the folded block of the end check is the
// concatenation of two segments which are apart in one of the texts); lanes walk it 64 positions at a time and ballots give the
// counts and the first four positions in order.  A call's window is up to three pieces of the query; the lanes are its start
// positions and compare an interesting k-mer and its reverse complement base by base, so a hit is a hit on the bases.
#include <vector>

#include "kv_device.h"

namespace {

#define CALL_LANES 64
#define CALL_MAX_LEN (1u << 22)         // per sequence, as the alignment takes them
#define CALL_OP_M 0u
#define CALL_OP_I 1u
#define CALL_OP_D 2u

static_assert(KV_CALL_RECORD_WORDS == 32, "include/kvsketch.h states the record");

// `len` aligned positions: position p reads target byte tpos + p (+ tgap from the seam on) and query byte qpos + p (+ qgap)
struct CallBlock {
    uint32_t len, tpos, qpos, seam, tgap, qgap;
};

// what a job is once the end check has answered
struct CallShape {
    uint32_t cls;               // KV_CALL_NONE / SNV / INDEL
    uint32_t indel_op;          // CALL_OP_I or CALL_OP_D
    uint32_t indel_len, indel_qpos;
    CallBlock scan[2];          // the match block of an snv, or the left and right flanks of an indel; len 0 = none
};

struct CallJob {
    uint64_t toff, qoff;        // first byte of the target / the query in the concatenated texts
    uint64_t ik_begin, ik_end;  // the query's interesting k-mers
    uint32_t tlen, qlen, rev, index;
    uint32_t fold_len;          // bytes the end check compares; 0 = it cannot fold
    uint32_t fold_t, fold_q;    // where it compares them in the target and in the query
    uint32_t pad;
    CallShape shape[2];         // [0] not folded, [1] folded
};

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

// kevlar/varmap.py:49-54 on block types: an optional leading D/I, then M or M (I|D) M, then an optional trailing D/I
struct CallRun {
    uint32_t op, len, tpos, qpos;
};

void call_shape(const std::vector<CallRun> &blocks, const CallBlock *merged, int merged_at, CallShape &out)
{
    out = CallShape();
    out.cls = KV_CALL_NONE;
    const int n = (int)blocks.size();
    if (n < 1 || n > 5) return;
    const int lead = blocks[0].op != CALL_OP_M ? 1 : 0, trail = blocks[n - 1].op != CALL_OP_M ? 1 : 0;
    const int core = n - lead - trail;
    auto plain = [&](int at) {
        if (merged && at == merged_at) return *merged;         // the concatenation the end check put there
        CallBlock b;
        b.len = blocks[at].len; b.tpos = blocks[at].tpos; b.qpos = blocks[at].qpos; b.seam = b.len; b.tgap = b.qgap = 0;
        return b;
    };
    if (core == 1 && blocks[lead].op == CALL_OP_M) {
        out.cls = KV_CALL_SNV;
        out.scan[0] = plain(lead);
    } else if (core == 3 && blocks[lead].op == CALL_OP_M && blocks[lead + 1].op != CALL_OP_M && blocks[lead + 2].op == CALL_OP_M) {
        out.cls = KV_CALL_INDEL;
        out.scan[0] = plain(lead);
        out.scan[1] = plain(lead + 2);
        out.indel_op = blocks[lead + 1].op;
        out.indel_len = blocks[lead + 1].len;
        out.indel_qpos = blocks[lead + 1].qpos;
    }
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
    KV_REQUIRE(toffsets && qoffsets && ik_offsets && (n_jobs == 0 || (tbases && qbases && jobs && run_offsets && run_counts && records)) &&
                   (n_runs == 0 || runs),
               KV_ERR_ARG, "kv_call_scan: null argument");
    KV_REQUIRE(ksize >= 1 && ksize <= (int)CALL_MAX_LEN && mindist >= 0 && mindist <= (int)CALL_MAX_LEN, KV_ERR_ARG,
               "kv_call_scan: ksize %d (at least 1) and mindist %d (at least 0)", ksize, mindist);
    KV_REQUIRE(n_jobs < 0x7FFFFFFFull, KV_ERR_ARG, "kv_call_scan: %llu jobs", (unsigned long long)n_jobs);
    for (uint64_t c = 0; c < n_targets; ++c)
        KV_REQUIRE(toffsets[c] <= toffsets[c + 1], KV_ERR_ARG, "kv_call_scan: target offsets must not decrease");
    for (uint64_t c = 0; c < n_queries; ++c) {
        KV_REQUIRE(qoffsets[c] <= qoffsets[c + 1], KV_ERR_ARG, "kv_call_scan: query offsets must not decrease");
        KV_REQUIRE(ik_offsets[c] <= ik_offsets[c + 1], KV_ERR_ARG, "kv_call_scan: interesting k-mer offsets must not decrease");
    }
    const uint64_t n_ik = ik_offsets[n_queries];
    KV_REQUIRE(n_ik == 0 || ikmers, KV_ERR_ARG, "kv_call_scan: null argument");
    for (uint64_t q = 0; q < n_queries; ++q) {
        const uint64_t ql = qoffsets[q + 1] - qoffsets[q];
        for (uint64_t a = ik_offsets[q]; a < ik_offsets[q + 1]; ++a)
            KV_REQUIRE(ikmers[2 * a + 1] >= 1 && (uint64_t)ikmers[2 * a] + ikmers[2 * a + 1] <= ql, KV_ERR_ARG,
                       "interesting k-mer %llu of query %llu: %u bases at offset %u of a %llu-base contig", (unsigned long long)(a - ik_offsets[q]),
                       (unsigned long long)q, ikmers[2 * a + 1], ikmers[2 * a], (unsigned long long)ql);
    }

    std::vector<CallJob> descs(n_jobs);
    std::vector<CallRun> blocks;
    for (uint64_t k = 0; k < n_jobs; ++k) {
        const uint32_t t = jobs[3 * k], q = jobs[3 * k + 1];
        KV_REQUIRE(t < n_targets && q < n_queries && jobs[3 * k + 2] <= 1, KV_ERR_ARG,
                   "call job %llu names target %u of %llu, query %u of %llu, strand flag %u", (unsigned long long)k, t,
                   (unsigned long long)n_targets, q, (unsigned long long)n_queries, jobs[3 * k + 2]);
        const uint64_t tl = toffsets[t + 1] - toffsets[t], ql = qoffsets[q + 1] - qoffsets[q];
        KV_REQUIRE(tl >= 1 && ql >= 1, KV_ERR_ARG, "call job %llu has an empty sequence", (unsigned long long)k);
        KV_REQUIRE(tl <= CALL_MAX_LEN && ql <= CALL_MAX_LEN, KV_ERR_ARG, "call job %llu: sequences of %llu and %llu bases (at most %u)",
                   (unsigned long long)k, (unsigned long long)tl, (unsigned long long)ql, CALL_MAX_LEN);
        const uint64_t r0 = run_offsets[k], nr = run_counts[k];
        KV_REQUIRE(r0 <= n_runs && nr <= n_runs - r0, KV_ERR_ARG, "call job %llu: runs %llu .. %llu of %llu", (unsigned long long)k,
                   (unsigned long long)r0, (unsigned long long)(r0 + nr), (unsigned long long)n_runs);
        // the tokenizer (kevlar/cigar.py:28-44); only a short list can match a pattern, of a long one the last three blocks matter
        uint64_t tpos = 0, qpos = 0;
        blocks.clear();
        CallRun tail[3] = {};
        for (uint64_t r = 0; r < nr; ++r) {
            const uint32_t run = runs[r0 + r], op = run & 0xFu, len = run >> 4;
            KV_REQUIRE(op <= CALL_OP_D && len >= 1, KV_ERR_ARG, "call job %llu: run %llu is %u << 4 | %u (a length of at least 1, op 0..2)",
                       (unsigned long long)k, (unsigned long long)r, len, op);
            const CallRun blk = {op, len, (uint32_t)tpos, (uint32_t)qpos};
            if (op != CALL_OP_I) tpos += len;
            if (op != CALL_OP_D) qpos += len;
            KV_REQUIRE(tpos <= tl && qpos <= ql, KV_ERR_ARG, "call job %llu: the runs consume more than the %llu and %llu bases of its sequences",
                       (unsigned long long)k, (unsigned long long)tl, (unsigned long long)ql);
            if (nr <= 6) blocks.push_back(blk);
            tail[0] = tail[1];
            tail[1] = tail[2];
            tail[2] = blk;
        }
        KV_REQUIRE(tpos == tl && qpos == ql, KV_ERR_ARG, "call job %llu: the runs consume %llu and %llu bases, the sequences have %llu and %llu",
                   (unsigned long long)k, (unsigned long long)tpos, (unsigned long long)qpos, (unsigned long long)tl, (unsigned long long)ql);
        CallJob &d = descs[k];
        d = CallJob();
        d.toff = toffsets[t];
        d.qoff = qoffsets[q];
        d.ik_begin = ik_offsets[q];
        d.ik_end = ik_offsets[q + 1];
        d.tlen = (uint32_t)tl;
        d.qlen = (uint32_t)ql;
        d.rev = jobs[3 * k + 2];
        d.index = (uint32_t)k;
        call_shape(blocks, nullptr, -1, d.shape[0]);
        d.shape[1] = d.shape[0];
        if (nr >= 3 && tail[2].op == CALL_OP_M && tail[0].op == CALL_OP_M) {
            // kevlar/cigar.py:52-61: `prev + last` lies in one piece in the sequence the middle block belongs to, from the middle
            // block on; the other sequence's last block is what it has to start with (a middle block that is no D goes the I way)
            d.fold_len = tail[2].len;
            d.fold_t = tail[1].op == CALL_OP_D ? tail[1].tpos : tail[2].tpos;
            d.fold_q = tail[1].op == CALL_OP_D ? tail[2].qpos : tail[1].qpos;
            if (nr <= 6) {
                CallBlock merged;
                merged.len = tail[0].len + tail[2].len;
                merged.tpos = tail[0].tpos;
                merged.qpos = tail[0].qpos;
                merged.seam = tail[0].len;
                merged.tgap = tail[2].tpos - (tail[0].tpos + tail[0].len);
                merged.qgap = tail[2].qpos - (tail[0].qpos + tail[0].len);
                std::vector<CallRun> after(blocks.begin(), blocks.end() - 1);
                after[after.size() - 2].len = merged.len;
                call_shape(after, &merged, (int)after.size() - 2, d.shape[1]);
            } else {
                d.shape[1] = CallShape();
            }
        }
    }
    if (n_jobs == 0) return KV_OK;

    uint8_t comp[256];
    call_comp_table(comp);
    hipStream_t st = kv_stream();
    const uint64_t tbytes = toffsets[n_targets], qbytes = qoffsets[n_queries];
    KvDevBuf d_t, d_q, d_jobs, d_ik, d_comp, d_rec;
    hipError_t e = d_t.alloc(tbytes);
    if (e == hipSuccess) e = d_q.alloc(qbytes);
    if (e == hipSuccess) e = d_jobs.alloc(n_jobs * sizeof(CallJob));
    if (e == hipSuccess) e = d_ik.alloc(n_ik * 8);
    if (e == hipSuccess) e = d_comp.alloc(256);
    if (e == hipSuccess) e = d_rec.alloc(n_jobs * KV_CALL_RECORD_WORDS * 4);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "call scan buffers allocation failed: %s", hipGetErrorString(e));
    KV_HIP(hipMemcpyAsync(d_t.p, tbases, tbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_q.p, qbases, qbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_jobs.p, descs.data(), n_jobs * sizeof(CallJob), hipMemcpyHostToDevice, st));
    if (n_ik) KV_HIP(hipMemcpyAsync(d_ik.p, ikmers, n_ik * 8, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d_comp.p, comp, 256, hipMemcpyHostToDevice, st));
    CallParams p;
    p.jobs = d_jobs.as<CallJob>(); p.tbases = d_t.as<uint8_t>(); p.qbases = d_q.as<uint8_t>(); p.ikmers = d_ik.as<uint32_t>();
    p.comp = d_comp.as<uint8_t>(); p.records = d_rec.as<uint32_t>(); p.ksize = (uint32_t)ksize; p.mindist = (uint32_t)mindist;
    {
        KvProfScope prof("k_call_scan");
        hipLaunchKernelGGL(k_call_scan, dim3((unsigned)n_jobs), dim3(CALL_LANES), 0, st, p);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(records, d_rec.p, n_jobs * KV_CALL_RECORD_WORDS * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}
