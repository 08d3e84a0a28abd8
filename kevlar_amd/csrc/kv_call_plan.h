// kv_call_plan.h -- the host half of kv_call_scan's rules (kv_call.hip), free of HIP: the tokenizer of kevlar/cigar.py:28-44 on
// the runs of one aligned job, the candidate of the end check (kevlar/cigar.py:46-71) and, for both of its answers, the class of
// the CIGAR (kevlar/varmap.py:49-54) and the match blocks the device scans.  Plain C++17: tests/harness/align_call_plan_host.cpp
// compiles it for the host, tests/test_align_call_plan.py holds it to tokenize, endcheck and classify of tests/call_common.py.
#pragma once
#include <cstddef>

#include "kv_seq_jobs.h"

#define CALL_OP_M 0u
#define CALL_OP_I 1u
#define CALL_OP_D 2u
#define CALL_MAX_BLOCKS 6       // only a list this short can match a pattern; of a longer one the last three blocks matter

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
static_assert(sizeof(CallBlock) == 24 && sizeof(CallShape) == 64 && offsetof(CallShape, scan) == 16 && sizeof(CallJob) == 192 &&
                  offsetof(CallJob, ik_begin) == 16 && offsetof(CallJob, qlen) == 36 && offsetof(CallJob, index) == 44 && offsetof(CallJob, fold_len) == 48 &&
                  offsetof(CallJob, fold_q) == 56 && offsetof(CallJob, shape) == 64, "k_call_scan reads the descriptor");

// kevlar/varmap.py:49-54 on block types: an optional leading D/I, then M or M (I|D) M, then an optional trailing D/I
struct CallRun {
    uint32_t op, len, tpos, qpos;
};

static inline void call_shape(const CallRun *blocks, int n, const CallBlock *merged, int merged_at, CallShape &out)
{
    out = CallShape();
    out.cls = KV_CALL_NONE;
    if (n < 1 || n > 5) return;
    const int lead = blocks[0].op != CALL_OP_M ? 1 : 0, trail = blocks[n - 1].op != CALL_OP_M ? 1 : 0, core = n - lead - trail;
    auto plain = [&](int at) {
        if (merged && at == merged_at) return *merged;         // the concatenation the end check put there
        return CallBlock{blocks[at].len, blocks[at].tpos, blocks[at].qpos, blocks[at].len, 0, 0};
    };
    if (core == 1 && blocks[lead].op == CALL_OP_M) {
        out.cls = KV_CALL_SNV;
        out.scan[0] = plain(lead);
    } else if (core == 3 && blocks[lead].op == CALL_OP_M && blocks[lead + 1].op != CALL_OP_M && blocks[lead + 2].op == CALL_OP_M) {
        out.cls = KV_CALL_INDEL;
        out.scan[0] = plain(lead);
        out.scan[1] = plain(lead + 2);
        out.indel_op = blocks[lead + 1].op; out.indel_len = blocks[lead + 1].len; out.indel_qpos = blocks[lead + 1].qpos;
    }
}

// job `index` with its `nr` runs (`length << 4 | op`) -> the descriptor; refuses runs that are no tokenization of its sequences
static inline int call_plan_job(const KvSeqJob &job, uint64_t ik_begin, uint64_t ik_end, const uint32_t *runs, uint64_t nr, uint32_t index, CallJob &out)
{
    const unsigned long long k = index, tl = job.tlen, ql = job.qlen;
    uint64_t tpos = 0, qpos = 0;
    CallRun blocks[CALL_MAX_BLOCKS], tail[3] = {};
    for (uint64_t r = 0; r < nr; ++r) {
        const uint32_t op = runs[r] & 0xFu, len = runs[r] >> 4;
        KV_REQUIRE(op <= CALL_OP_D && len >= 1, KV_ERR_ARG, "call job %llu: run %llu is %u << 4 | %u (a length of at least 1, op 0..2)", k,
                   (unsigned long long)r, len, op);
        const CallRun blk = {op, len, (uint32_t)tpos, (uint32_t)qpos};
        if (op != CALL_OP_I) tpos += len;
        if (op != CALL_OP_D) qpos += len;
        KV_REQUIRE(tpos <= tl && qpos <= ql, KV_ERR_ARG, "call job %llu: the runs consume more than the %llu and %llu bases of its sequences", k, tl, ql);
        if (nr <= CALL_MAX_BLOCKS) blocks[r] = blk;
        tail[0] = tail[1]; tail[1] = tail[2]; tail[2] = blk;
    }
    KV_REQUIRE(tpos == tl && qpos == ql, KV_ERR_ARG, "call job %llu: the runs consume %llu and %llu bases, the sequences have %llu and %llu", k,
               (unsigned long long)tpos, (unsigned long long)qpos, tl, ql);
    out = CallJob();
    out.toff = job.toff; out.qoff = job.qoff; out.ik_begin = ik_begin; out.ik_end = ik_end;
    out.tlen = job.tlen; out.qlen = job.qlen; out.rev = job.rev; out.index = index;
    call_shape(blocks, nr <= CALL_MAX_BLOCKS ? (int)nr : 0, nullptr, -1, out.shape[0]);
    out.shape[1] = out.shape[0];
    if (nr >= 3 && tail[2].op == CALL_OP_M && tail[0].op == CALL_OP_M) {
        // kevlar/cigar.py:52-61: `prev + last` lies in one piece in the sequence the middle block belongs to, from the middle
        // block on; the other sequence's last block is what it has to start with (a middle block that is no D goes the I way)
        out.fold_len = tail[2].len;
        out.fold_t = tail[1].op == CALL_OP_D ? tail[1].tpos : tail[2].tpos;
        out.fold_q = tail[1].op == CALL_OP_D ? tail[2].qpos : tail[1].qpos;
        out.shape[1] = CallShape();                             // (a longer list matches no pattern, folded or not)
        if (nr <= CALL_MAX_BLOCKS) {
            const CallBlock merged = {tail[0].len + tail[2].len, tail[0].tpos, tail[0].qpos, tail[0].len, tail[2].tpos - (tail[0].tpos + tail[0].len),
                                      tail[2].qpos - (tail[0].qpos + tail[0].len)};
            blocks[nr - 3].len = merged.len;                   // the list after the fold: the last block gone, the third-last grown
            call_shape(blocks, (int)nr - 1, &merged, (int)nr - 3, out.shape[1]);
        }
    }
    return KV_OK;
}

// every job of a checked table (kv_seq_jobs.h); job k's runs are runs[run_offsets[k] .. + run_counts[k]) of a pool of n_runs
static inline int call_plan_jobs(const std::vector<KvSeqJob> &table, const uint64_t *ik_offsets, const uint64_t *run_offsets, const uint32_t *run_counts,
                                 const uint32_t *runs, uint64_t n_runs, std::vector<CallJob> &descs)
{
    descs.resize(table.size());
    for (uint64_t k = 0; k < table.size(); ++k) {
        const uint64_t r0 = run_offsets[k], nr = run_counts[k], q = table[k].query;
        KV_REQUIRE(r0 <= n_runs && nr <= n_runs - r0, KV_ERR_ARG, "call job %llu: runs %llu .. %llu of %llu", (unsigned long long)k,
                   (unsigned long long)r0, (unsigned long long)(r0 + nr), (unsigned long long)n_runs);
        KV_STEP(call_plan_job(table[k], ik_offsets[q], ik_offsets[q + 1], runs + r0, nr, (uint32_t)k, descs[k]));
    }
    return KV_OK;
}
