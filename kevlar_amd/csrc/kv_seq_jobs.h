// kv_seq_jobs.h -- what a batch of sequences and jobs must satisfy before kv_align_batch, kv_call_scan or kv_simlike_score touch
// the device, and this is its only statement: concatenated texts with n + 1 offsets that do not decrease, (target, query,
// strand) triples that name sequences that exist, are not empty and hold at most KV_SEQ_MAX_LEN bases, interesting k-mers inside
// their contig.  Plain C++17, no HIP: tests/harness/align_call_plan_host.cpp compiles it, tests/test_align_call_plan.py checks it.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/kvsketch.h"
#include "kv_require.h"

#define KV_SEQ_MAX_LEN (1u << 22)       // per sequence: gap extension * length stays far inside int32

struct KvSeqJob {
    uint64_t toff, qoff;        // first byte of the target / the query in the concatenated texts
    uint32_t tlen, qlen, target, query, rev;
};

static inline int kv_seq_offsets(const char *who, const char *what, const uint64_t *offsets, uint64_t n)
{
    for (uint64_t c = 0; c < n; ++c) KV_REQUIRE(offsets[c] <= offsets[c + 1], KV_ERR_ARG, "%s: %s offsets must not decrease", who, what);
    return KV_OK;
}

static inline int kv_seq_lengths(const char *noun, uint64_t k, uint64_t tl, uint64_t ql)
{
    KV_REQUIRE(tl >= 1 && ql >= 1, KV_ERR_ARG, "%s job %llu has an empty sequence", noun, (unsigned long long)k);
    KV_REQUIRE(tl <= KV_SEQ_MAX_LEN && ql <= KV_SEQ_MAX_LEN, KV_ERR_ARG, "%s job %llu: sequences of %llu and %llu bases (at most %u)", noun,
               (unsigned long long)k, (unsigned long long)tl, (unsigned long long)ql, KV_SEQ_MAX_LEN);
    return KV_OK;
}

// who: the entry, noun: "alignment" or "call" -- for the message.  out[k] is job k.
static inline int kv_seq_jobs(const char *who, const char *noun, const uint64_t *toffsets, uint64_t n_targets, const uint64_t *qoffsets,
                              uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs, std::vector<KvSeqJob> &out)
{
    KV_REQUIRE(toffsets && qoffsets && (n_jobs == 0 || jobs), KV_ERR_ARG, "%s: null argument", who);
    KV_REQUIRE(n_jobs < 0x7FFFFFFFull, KV_ERR_ARG, "%s: %llu jobs", who, (unsigned long long)n_jobs);
    KV_STEP(kv_seq_offsets(who, "target", toffsets, n_targets));
    KV_STEP(kv_seq_offsets(who, "query", qoffsets, n_queries));
    out.resize(n_jobs);
    for (uint64_t k = 0; k < n_jobs; ++k) {
        const uint32_t t = jobs[3 * k], q = jobs[3 * k + 1], rev = jobs[3 * k + 2];
        KV_REQUIRE(t < n_targets && q < n_queries && rev <= 1, KV_ERR_ARG, "%s job %llu names target %u of %llu, query %u of %llu, strand flag %u",
                   noun, (unsigned long long)k, t, (unsigned long long)n_targets, q, (unsigned long long)n_queries, rev);
        const uint64_t tl = toffsets[t + 1] - toffsets[t], ql = qoffsets[q + 1] - qoffsets[q];
        KV_STEP(kv_seq_lengths(noun, k, tl, ql));
        out[k] = KvSeqJob{toffsets[t], qoffsets[q], (uint32_t)tl, (uint32_t)ql, t, q, rev};
    }
    return KV_OK;
}

// the interesting k-mers of every query, (offset, ksize) pairs: at least one base each, inside the contig (qoffsets checked, ik_offsets not null)
static inline int kv_seq_ikmers(const char *who, const uint64_t *qoffsets, uint64_t n_queries, const uint64_t *ik_offsets, const uint32_t *ikmers)
{
    KV_STEP(kv_seq_offsets(who, "interesting k-mer", ik_offsets, n_queries));
    KV_REQUIRE(ik_offsets[n_queries] == 0 || ikmers, KV_ERR_ARG, "%s: null argument", who);
    for (uint64_t q = 0; q < n_queries; ++q)
        for (uint64_t a = ik_offsets[q], ql = qoffsets[q + 1] - qoffsets[q]; a < ik_offsets[q + 1]; ++a)
            KV_REQUIRE(ikmers[2 * a + 1] >= 1 && (uint64_t)ikmers[2 * a] + ikmers[2 * a + 1] <= ql, KV_ERR_ARG,
                       "interesting k-mer %llu of query %llu: %u bases at offset %u of a %llu-base contig", (unsigned long long)(a - ik_offsets[q]),
                       (unsigned long long)q, ikmers[2 * a + 1], ikmers[2 * a], (unsigned long long)ql);
    return KV_OK;
}
