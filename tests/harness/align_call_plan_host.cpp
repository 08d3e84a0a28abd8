// Host-side harness for kevlar_amd/csrc/kv_seq_jobs.h, kv_align_plan.h and kv_call_plan.h (compiled as plain C++ by
// tests/test_align_call_plan.py): the job table, the alignment's plan and layout and the call descriptors behind a C ABI, so that
// Python can compare them with a restatement of the rules.  Results come back in caller-provided arrays sized by the caller's own
// counts.  With -DKV_HARNESS_MAIN the file is a program: seeded batches through the same functions with the disjointness and
// bounds checks done here, for a run under the host sanitizers.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../kevlar_amd/csrc/kv_align_plan.h"
#include "../../kevlar_amd/csrc/kv_call_plan.h"

static char g_error[512];
void kv_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

namespace {
// (toff, qoff, tlen, qlen, rev) per job
std::vector<KvSeqJob> table_of(const uint64_t *rows, uint64_t n)
{
    std::vector<KvSeqJob> t(n);
    for (uint64_t k = 0; k < n; ++k) t[k] = KvSeqJob{rows[5 * k], rows[5 * k + 1], (uint32_t)rows[5 * k + 2], (uint32_t)rows[5 * k + 3], 0, 0, (uint32_t)rows[5 * k + 4]};
    return t;
}
}  // namespace

extern "C" {
const char *h_last_error() { return g_error; }

void h_constants(uint64_t *out)
{
    const uint64_t c[9] = {KV_SEQ_MAX_LEN, ALN_LANES, ALN_STRIP, CALL_MAX_BLOCKS, sizeof(AlignJob), sizeof(CallJob), KV_CALL_NONE, KV_CALL_SNV, KV_CALL_INDEL};
    memcpy(out, c, sizeof(c));
}

// out: (toff, qoff, tlen, qlen, target, query, rev) per job
int h_seq_jobs(const char *who, const char *noun, const uint64_t *toffsets, uint64_t n_targets, const uint64_t *qoffsets, uint64_t n_queries,
               const uint32_t *jobs, uint64_t n_jobs, uint64_t *out)
{
    std::vector<KvSeqJob> t;
    g_error[0] = 0;
    const int rc = kv_seq_jobs(who, noun, toffsets, n_targets, qoffsets, n_queries, jobs, n_jobs, t);
    if (rc != KV_OK) return rc;
    for (uint64_t k = 0; k < n_jobs; ++k) {
        const uint64_t row[7] = {t[k].toff, t[k].qoff, t[k].tlen, t[k].qlen, t[k].target, t[k].query, t[k].rev};
        memcpy(out + 7 * k, row, sizeof(row));
    }
    return rc;
}

uint64_t h_z_bytes(uint64_t tlen, uint64_t qlen) { return aln_z_bytes(tlen, qlen); }

// rows: (toff, qoff, tlen, qlen, rev) per job.  ends: the launches; descs: (index, toff, qoff, tlen, qlen, rev, zoff, bndoff,
// tmpoff) per descriptor in launch order; scalars: launches, z_max, bnd_max, tmp_max, cells
int h_align_layout(const uint64_t *rows, uint64_t n_jobs, uint64_t z_budget, uint64_t *ends, uint64_t *descs, uint64_t *scalars)
{
    const std::vector<KvSeqJob> t = table_of(rows, n_jobs);
    AlignLayout lay;
    g_error[0] = 0;
    const int rc = aln_layout(t, z_budget, lay);
    if (rc != KV_OK) return rc;
    std::copy(lay.ends.begin(), lay.ends.end(), ends);
    for (uint64_t k = 0; k < lay.descs.size(); ++k) {
        const AlignJob &d = lay.descs[k];
        const uint64_t row[9] = {d.index, d.toff, d.qoff, d.tlen, d.qlen, d.rev, d.zoff, d.bndoff, d.tmpoff};
        memcpy(descs + 9 * k, row, sizeof(row));
    }
    const uint64_t s[5] = {lay.ends.size(), lay.z_max, lay.bnd_max, lay.tmp_max, lay.cells};
    memcpy(scalars, s, sizeof(s));
    return rc;
}

// the host half of kv_call_scan in front of the device: *stage says which rule refused (1 the job table, 2 the interesting
// k-mers, 3 the runs; 0 none).  descs: n_jobs descriptors.
int h_call_plan(const uint64_t *toffsets, uint64_t n_targets, const uint64_t *qoffsets, uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs,
                const uint64_t *run_offsets, const uint32_t *run_counts, const uint32_t *runs, uint64_t n_runs, const uint64_t *ik_offsets,
                const uint32_t *ikmers, CallJob *descs, int *stage)
{
    std::vector<KvSeqJob> t;
    std::vector<CallJob> d;
    g_error[0] = 0;
    *stage = 1;
    KV_STEP(kv_seq_jobs("kv_call_scan", "call", toffsets, n_targets, qoffsets, n_queries, jobs, n_jobs, t));
    *stage = 2;
    KV_STEP(kv_seq_ikmers("kv_call_scan", qoffsets, n_queries, ik_offsets, ikmers));
    *stage = 3;
    KV_STEP(call_plan_jobs(t, ik_offsets, run_offsets, run_counts, runs, n_runs, d));
    *stage = 0;
    std::copy(d.begin(), d.end(), descs);
    return KV_OK;
}
}

#ifdef KV_HARNESS_MAIN
namespace {
uint64_t g_seed = 20261020;
uint32_t rnd(uint32_t lo, uint32_t hi)          // lo .. hi
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (uint32_t)((g_seed >> 33) % (hi - lo + 1));
}
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// intervals (begin, length) of one launch: inside [0, bound) and pairwise disjoint
bool disjoint(std::vector<std::pair<uint64_t, uint64_t>> v, uint64_t bound)
{
    std::sort(v.begin(), v.end());
    uint64_t at = 0;
    for (const auto &x : v) {
        if (x.first < at) return false;
        at = x.first + x.second;
    }
    return at <= bound;
}

int fuzz_layout()
{
    for (int round = 0; round < 300; ++round) {
        const uint64_t n = rnd(1, 200);
        std::vector<uint64_t> rows(5 * n);
        uint64_t biggest = 0, sum = 0;
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t row[5] = {rnd(0, 1u << 30), rnd(0, 1u << 30), rnd(1, 2000), rnd(1, 2000), rnd(0, 1)};
            memcpy(&rows[5 * k], row, sizeof(row));
            biggest = std::max(biggest, aln_z_bytes(row[2], row[3]));
            sum += aln_z_bytes(row[2], row[3]);
        }
        const uint64_t budget = biggest + (uint64_t)((double)(sum - biggest) * rnd(0, 100) / 100.0);
        const std::vector<KvSeqJob> t = table_of(rows.data(), n);
        AlignLayout lay;
        CHECK(aln_layout(t, budget, lay) == KV_OK);
        CHECK(lay.descs.size() == n && !lay.ends.empty() && lay.ends.back() == n);
        uint64_t k = 0;
        for (const uint64_t end : lay.ends) {
            std::vector<std::pair<uint64_t, uint64_t>> z, bnd, tmp;
            for (; k < end; ++k) {
                const AlignJob &d = lay.descs[k];
                CHECK(d.index < n && d.tlen == t[d.index].tlen && d.qlen == t[d.index].qlen);
                z.emplace_back(d.zoff, aln_z_bytes(d.tlen, d.qlen));
                bnd.emplace_back(d.bndoff, 2ull * d.tlen);
                tmp.emplace_back(d.tmpoff, (uint64_t)d.tlen + d.qlen);
            }
            CHECK(disjoint(z, std::min(lay.z_max, budget)) && disjoint(bnd, lay.bnd_max) && disjoint(tmp, lay.tmp_max));
        }
        CHECK(aln_layout(t, biggest - 1, lay) == KV_ERR_CAPACITY);
    }
    return 0;
}

int fuzz_call_plan()
{
    for (int round = 0; round < 2000; ++round) {
        const uint64_t nr = rnd(1, 9);
        uint32_t runs[10];
        uint32_t tl = 0, ql = 0;
        for (uint64_t r = 0; r < nr; ++r) {
            const uint32_t op = rnd(0, 3) % 3, len = rnd(1, 40);       // (M twice as often)
            runs[r] = len << 4 | op;
            if (op != CALL_OP_I) tl += len;
            if (op != CALL_OP_D) ql += len;
        }
        if (tl == 0 || ql == 0) continue;                               // (no job has an empty sequence)
        const KvSeqJob job = {rnd(0, 1000), rnd(0, 1000), tl, ql, 0, 0, rnd(0, 1)};
        CallJob d;
        CHECK(call_plan_job(job, 3, 7, runs, nr, (uint32_t)round, d) == KV_OK);
        CHECK(d.index == (uint32_t)round && d.tlen == tl && d.qlen == ql && d.fold_t + d.fold_len <= tl && d.fold_q + d.fold_len <= ql);
        for (const CallShape &s : d.shape)
            for (const CallBlock &b : s.scan)
                CHECK(b.seam <= b.len && (uint64_t)b.tpos + b.tgap + b.len <= tl && (uint64_t)b.qpos + b.qgap + b.len <= ql);
        CHECK(nr <= CALL_MAX_BLOCKS || d.shape[0].cls == KV_CALL_NONE);
        // one base more or less on either side, a run of no length, another op: refused
        runs[nr] = 1u << 4 | CALL_OP_M;
        CHECK(call_plan_job(job, 3, 7, runs, nr + 1, 0, d) == KV_ERR_ARG && call_plan_job(job, 3, 7, runs, nr - 1, 0, d) == KV_ERR_ARG);
        uint32_t &spoilt = runs[rnd(0, (uint32_t)nr - 1)];
        spoilt = round % 2 ? spoilt & 0xFu : spoilt | 3u;
        CHECK(call_plan_job(job, 3, 7, runs, nr, 0, d) == KV_ERR_ARG);
    }
    return 0;
}
}  // namespace

int main()
{
    if (fuzz_layout() || fuzz_call_plan()) return 1;
    printf("align and call plan fuzz ok\n");
    return 0;
}
#endif
