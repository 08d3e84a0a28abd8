// kv_align_plan.h -- the host rules of the batched alignment (kv_align.hip), free of HIP: the direction bytes a job needs, the
// order of the jobs, where the batch is cut into launches and where every job of a launch keeps its direction bytes, boundary
// rows and temporary runs (two jobs of one launch that overlap there give a wrong CIGAR, not an error).  Plain C++17:
// tests/harness/align_call_plan_host.cpp compiles it for the host, tests/test_align_call_plan.py checks order, cuts and disjointness.
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>

#include "kv_seq_jobs.h"

#define ALN_LANES 64
#define ALN_COLS 4
#define ALN_STRIP (ALN_LANES * ALN_COLS)
static_assert(ALN_STRIP == KV_ALIGN_STRIP, "include/kvsketch.h states the strip width");

struct AlignJob {
    uint64_t toff, qoff;        // first byte of the target / the query in the concatenated texts
    uint64_t zoff;              // bytes, into the launch's z region (a multiple of ALN_STRIP)
    uint64_t bndoff;            // int2 entries: two boundary buffers of tlen each
    uint64_t tmpoff;            // uint32 entries: tlen + qlen runs at most
    uint32_t tlen, qlen, rev, index;
};
static_assert(sizeof(AlignJob) == 56 && offsetof(AlignJob, zoff) == 16 && offsetof(AlignJob, bndoff) == 24 && offsetof(AlignJob, tmpoff) == 32 &&
                  offsetof(AlignJob, index) == 52, "k_align reads the descriptor");

static inline uint64_t aln_z_bytes(uint64_t tlen, uint64_t qlen) { return (qlen + ALN_STRIP - 1) / ALN_STRIP * (tlen + ALN_LANES - 1) * ALN_STRIP; }

struct AlignLayout {
    std::vector<AlignJob> descs;        // the jobs by cells, largest first, equal ones in input order: descs[k].index is the job
    std::vector<uint64_t> ends;         // launch l runs descs[ends[l - 1] .. ends[l]), each with its place in the launch's working memory
    uint64_t z_max = 0, bnd_max = 0, tmp_max = 0, cells = 0;        // the most a launch needs: bytes, int2 entries, uint32 entries
};

// a launch takes jobs until the next one's direction bytes would pass the budget; a job that alone passes it is refused
static inline int aln_layout(const std::vector<KvSeqJob> &jobs, uint64_t z_budget, AlignLayout &lay)
{
    const uint64_t n_jobs = jobs.size();
    for (uint64_t k = 0; k < n_jobs; ++k)
        KV_REQUIRE(aln_z_bytes(jobs[k].tlen, jobs[k].qlen) <= z_budget, KV_ERR_CAPACITY,
                   "alignment job %llu (%u x %u) needs %llu bytes of direction bytes, the budget is %llu", (unsigned long long)k, jobs[k].tlen,
                   jobs[k].qlen, (unsigned long long)aln_z_bytes(jobs[k].tlen, jobs[k].qlen), (unsigned long long)z_budget);
    std::vector<uint32_t> order(n_jobs);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return (uint64_t)jobs[x].tlen * jobs[x].qlen > (uint64_t)jobs[y].tlen * jobs[y].qlen;
    });
    lay = AlignLayout();
    lay.descs.resize(n_jobs);
    uint64_t zo = 0, bo = 0, to = 0;
    for (uint64_t k = 0; k < n_jobs; ++k) {
        const KvSeqJob &j = jobs[order[k]];
        const uint64_t need = aln_z_bytes(j.tlen, j.qlen);
        if (k && zo + need > z_budget) { lay.ends.push_back(k); zo = bo = to = 0; }
        lay.descs[k] = AlignJob{j.toff, j.qoff, zo, bo, to, j.tlen, j.qlen, j.rev, order[k]};
        zo += need; bo += 2ull * j.tlen; to += (uint64_t)j.tlen + j.qlen;
        lay.z_max = std::max(lay.z_max, zo); lay.bnd_max = std::max(lay.bnd_max, bo); lay.tmp_max = std::max(lay.tmp_max, to);
        lay.cells += (uint64_t)j.tlen * j.qlen;
    }
    if (n_jobs) lay.ends.push_back(n_jobs);
    return KV_OK;
}
