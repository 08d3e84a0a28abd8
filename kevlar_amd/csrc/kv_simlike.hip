// kv_simlike.hip -- the scorer of `kevlar simlike` (kevlar/simlike.py:22-191, 278-300): for every call of a batch the abundances
// of its alternate-allele window's k-mers in the case, in every control and in the reference genome, the abundance filters and
// the three log likelihoods, in one launch.  The contract is in include/kvsketch.h, the rules in DESIGN.md section 12, the
// plain-Python restatement in tests/simlike_common.py.
//
// One wavefront per call, as in kv_call.hip: a window of 2k - 1 bases is one chunk of 64 k-mers, the refr window of a long
// deletion keeps one wave busy and no other.  The lanes are k-mer positions.  Step 1 hashes a k-mer once per hash family in
// use, looks it up everywhere and appends the counts of the positions the genome does not know to the call's lists, in order
// (ballot and lane prefix, the base carried from chunk to chunk).  Step 2 (dropoutliers) compacts every sample's list in
// place.  Step 3 reads the final lists for the filters and the sums.  The lists are the call's own stretch of the output, so
// steps 2 and 3 load what other lanes of this wave stored: every such hand-over goes through a __syncthreads() of the one-wave
// workgroup, which is the workgroup-scope release and acquire.
#include <cmath>
#include <vector>

#include "kv_device.h"
#include "kv_seq_jobs.h"        // KV_SEQ_MAX_LEN (per window, as kv_call.hip takes its sequences), kv_seq_offsets

namespace {

#define SIM_LANES 64
#define SIM_OUTLIER 20.0                // kevlar/simlike.py:41

static_assert(KV_SIMLIKE_RECORD_WORDS == KV_MAX_SAMPLES + 4, "include/kvsketch.h states the record");

struct SimCall {
    uint64_t aoff, roff;        // first byte of the alt / the refr window
    uint64_t kbase;             // k-mers of the calls in front of this one: where its lists start
    uint32_t alen, rlen;
};

struct SimParams {
    const SketchDev *sk[KV_MAX_SAMPLES];        // case, controls
    const SketchDev *refr;
    const SimCall *calls;
    const uint8_t *alt, *ref;
    uint32_t *records;
    double *ll;
    uint8_t *counts, *refr_out;
    double mu, sigma, epsilon;
    int32_t nsamples, ksize, fam_mask, refr_fam;        // fam_mask: bit HF_* set when a sketch of that family is among them
    int32_t casemin, ctrlmax, caseabundlow, ctrlabundhigh, dropoutliers;
};

__device__ __forceinline__ uint32_t sim_lane_rank(unsigned long long mask, int lane)
{
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ double sim_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return __shfl(v, 0);
}

__device__ __forceinline__ uint64_t sim_hash(const uint8_t *w, int k, int fam)
{
    return kmer_hash_chars([&](int j) { return (uint32_t)w[j]; }, [&](int j) { return complement_char(w[k - 1 - j]); }, k, fam);
}

// kevlar/simlike.py:99-132
struct SimModel {
    double mu, eps;
    double m1, s1, c1, m2, s2, c2;      // the two normal densities: mean, sd, -log(sd) - log(sqrt(2 pi))
    double le, l1e, le_indel, l1e_indel;        // log(error), log(1 - error); the same for the indel mode's error / 100
};

__device__ __forceinline__ SimModel sim_model(double mu, double sigma, double eps)
{
    SimModel m;
    const double half_log_2pi = 0.5 * log(2.0 * 3.14159265358979323846);
    m.mu = mu; m.eps = eps;
    m.m1 = mu / 2; m.s1 = sigma / 2; m.c1 = -log(m.s1) - half_log_2pi;
    m.m2 = mu; m.s2 = sigma; m.c2 = -log(m.s2) - half_log_2pi;
    m.le = log(eps); m.l1e = log(1.0 - eps);
    m.le_indel = log(eps * 0.01); m.l1e_indel = log(1.0 - eps * 0.01);
    return m;
}

// genotype 0; refrabund 0 = none (an indel, or a refr allele k-mer the genome's sketch does not hold)
__device__ __forceinline__ double sim_lp0(const SimModel &m, uint32_t abund, uint32_t refrabund)
{
    const bool indel = refrabund == 0;
    const double n = m.mu * (double)(indel ? 1u : refrabund);
    double a = (double)abund;
    if (a > n) a = n;
    const double fn = floor(n), fa = floor(a);
    const double lognck = lgamma(fn + 1.0) - lgamma(fa + 1.0) - lgamma(fn - fa + 1.0);
    return lognck + a * (indel ? m.le_indel : m.le) + (n - a) * (indel ? m.l1e_indel : m.l1e);
}

__device__ __forceinline__ double sim_lp1(const SimModel &m, uint32_t abund)
{
    const double z = ((double)abund - m.m1) / m.s1;
    return -(z * z) / 2.0 + m.c1;
}

__device__ __forceinline__ double sim_lp2(const SimModel &m, uint32_t abund)
{
    const double z = ((double)abund - m.m2) / m.s2;
    return -(z * z) / 2.0 + m.c2;
}

__global__ __launch_bounds__(SIM_LANES) void k_simlike(SimParams p)
{
    __shared__ uint32_t final_len[KV_MAX_SAMPLES];
    const int lane = threadIdx.x;
    const SimCall cl = p.calls[blockIdx.x];
    const int k = p.ksize, S = p.nsamples;
    const uint32_t nk = cl.alen - (uint32_t)k + 1u;
    const bool snv = cl.alen == cl.rlen;
    const uint8_t *A = p.alt + cl.aoff, *R = p.ref + cl.roff;
    uint8_t *lists = p.counts + cl.kbase * (uint64_t)S;         // sample s: lists[s * nk ..], nk entries of room
    uint8_t *rlist = p.refr_out + cl.kbase;

    // ---- 1: counts, and the positions whose k-mer the genome does not hold ------------------------------------------------
    uint32_t kept = 0;
    for (uint32_t i0 = 0; i0 < nk; i0 += SIM_LANES) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool live = i < nk;
        uint64_t h[2] = {0, 0};
        if (live) {
            if (p.fam_mask & (1 << HF_MURMUR)) h[HF_MURMUR] = sim_hash(A + i, k, HF_MURMUR);
            if (p.fam_mask & (1 << HF_TWOBIT)) h[HF_TWOBIT] = sim_hash(A + i, k, HF_TWOBIT);
        }
        const bool keep = live && sketch_get(p.refr, p.refr_fam ? h[1] : h[0]) == 0;
        const unsigned long long mask = __ballot(keep);
        const uint32_t at = kept + sim_lane_rank(mask, lane);
        for (int s = 0; s < S; ++s) {
            const SketchDev *sk = p.sk[s];
            if (keep) lists[(uint64_t)s * nk + at] = (uint8_t)sketch_get(sk, sk->hashfam ? h[1] : h[0]);
        }
        if (snv && keep) rlist[at] = (uint8_t)sketch_get(p.refr, sim_hash(R + i, k, p.refr_fam));
        kept += (uint32_t)__popcll(mask);
    }
    __syncthreads();

    // ---- 2: per sample, drop the counts 20 or more away from the sample's mean (kevlar/simlike.py:38-48) ------------------
    if (lane < KV_MAX_SAMPLES) final_len[lane] = kept;
    if (p.dropoutliers && kept) {
        for (int s = 0; s < S; ++s) {
            uint8_t *list = lists + (uint64_t)s * nk;
            uint32_t part = 0;
            for (uint32_t j = (uint32_t)lane; j < kept; j += SIM_LANES) part += list[j];
            const uint64_t sum = __shfl(wave_sum_u64((uint64_t)part), 0);
            const double mean = (double)sum / (double)kept;
            uint32_t left = 0;
            for (uint32_t j0 = 0; j0 < kept; j0 += SIM_LANES) {
                const uint32_t j = j0 + (uint32_t)lane;
                const uint32_t a = j < kept ? list[j] : 0u;
                const bool stay = j < kept && fabs((double)a - mean) < SIM_OUTLIER;
                const unsigned long long mask = __ballot(stay);
                __syncthreads();        // every lane has its count before a slot at or in front of it is written
                if (stay) list[left + sim_lane_rank(mask, lane)] = (uint8_t)a;
                left += (uint32_t)__popcll(mask);
            }
            for (uint32_t j = left + (uint32_t)lane; j < kept; j += SIM_LANES) list[j] = 0;     // (behind a list its room reads as zero)
            if (lane == 0) final_len[s] = left;
        }
    }
    __syncthreads();

    const uint32_t n_case = final_len[0];
    const uint32_t n_refr = snv ? kept : n_case;        // kevlar/simlike.py:89-95
    const uint8_t *lcase = lists;

    // ---- 3a: the filters (kevlar/simlike.py:278-300) --------------------------------------------------------------------
    uint32_t flags = snv ? 0u : KV_SIMLIKE_NO_REFR;
    {
        bool above = false, lowrun = false;
        uint32_t run = 0;               // low counts on end in front of this chunk
        const uint32_t want = p.caseabundlow > 0 ? (uint32_t)p.caseabundlow : 0u;
        for (uint32_t j0 = 0; j0 < n_case; j0 += SIM_LANES) {
            const uint32_t j = j0 + (uint32_t)lane;
            const int a = j < n_case ? (int)lcase[j] : 0;
            above = above || __ballot(j < n_case && a >= p.casemin) != 0ull;
            const unsigned long long low = __ballot(j < n_case && a < p.casemin);
            // the run of low counts that ends at this lane: up to the nearest lane below that is not low, or into the carry
            const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
            const unsigned long long high = ~low & upto;
            const uint32_t here = high ? (uint32_t)lane - (63u - (uint32_t)__builtin_clzll(high)) : (uint32_t)lane + 1u + run;
            lowrun = lowrun || (want && __ballot(here >= want) != 0ull);
            run = __shfl(here, 63);
        }
        if (!above) flags |= KV_SIMLIKE_PASSENGER;
        if (lowrun) flags |= KV_SIMLIKE_CASE_ABUND;
    }
    if (p.ctrlabundhigh > 0) {
        for (int s = 1; s < S; ++s) {
            const uint8_t *list = lists + (uint64_t)s * nk;
            const uint32_t n = final_len[s];
            uint32_t high = 0;
            for (uint32_t j0 = 0; j0 < n; j0 += SIM_LANES) {
                const uint32_t j = j0 + (uint32_t)lane;
                high += (uint32_t)__popcll(__ballot(j < n && (int)list[j] > p.ctrlmax));
            }
            if (high > (uint32_t)p.ctrlabundhigh) flags |= KV_SIMLIKE_CTRL_ABUND;
        }
    }
    if (final_len[1] != n_refr || final_len[2] != n_refr) flags |= KV_SIMLIKE_MISMATCH;    // kevlar/simlike.py:136-137

    // ---- 3b: the likelihoods (kevlar/simlike.py:135-191), lists paired by position up to the shorter one -------------------
    double lldn = 0.0, llfp = 0.0, llih = 0.0;
    if (!(flags & KV_SIMLIKE_MISMATCH)) {
        const SimModel m = sim_model(p.mu, p.sigma, p.epsilon);
        for (uint32_t j = (uint32_t)lane; j < n_case; j += SIM_LANES) lldn += sim_lp1(m, lcase[j]);
        for (int s = 0; s < S; ++s) {
            const uint8_t *list = lists + (uint64_t)s * nk;
            const uint32_t n = final_len[s] < n_refr ? final_len[s] : n_refr;
            for (uint32_t j = (uint32_t)lane; j < n; j += SIM_LANES) {
                const double v = sim_lp0(m, list[j], snv ? (uint32_t)rlist[j] : 0u);
                llfp += v;
                if (s) lldn += v;
            }
        }
        const uint8_t *lmom = lists + nk, *ldad = lists + 2ull * nk;
        uint32_t n = n_case < final_len[1] ? n_case : final_len[1];
        n = n < final_len[2] ? n : final_len[2];
        const double third = log(1.0 / 15.0);
        for (uint32_t j = (uint32_t)lane; j < n; j += SIM_LANES) {
            const uint32_t ac = lcase[j], am = lmom[j], af = ldad[j];
            const double pc[3] = {0.0, sim_lp1(m, ac), sim_lp2(m, ac)};
            const double pm[3] = {sim_lp0(m, am, 0u), sim_lp1(m, am), sim_lp2(m, am)};
            const double pf[3] = {sim_lp0(m, af, 0u), sim_lp1(m, af), sim_lp2(m, af)};
            // the 11 of the 15 inheritance scenarios in which the proband carries the allele: (child, mother, father), packed
            // two bits a genotype
            const uint32_t scenarios[11] = {0x11, 0x21, 0x05, 0x15, 0x25, 0x09, 0x19, 0x16, 0x26, 0x1A, 0x2A};
            double best = 0.0;
#pragma unroll
            for (int c = 0; c < 11; ++c) {
                const uint32_t sc = scenarios[c];
                const double v = pc[sc & 3u] + pm[(sc >> 2) & 3u] + pf[(sc >> 4) & 3u] + third;
                best = (c == 0 || v > best) ? v : best;
            }
            llih += best;
        }
        lldn = sim_wave_sum(lldn);
        llfp = sim_wave_sum(llfp);
        llih = log(15.0 / 11.0) + sim_wave_sum(llih);
    }

    // the record: one lane a word
    uint32_t word = 0;
    if (lane < KV_MAX_SAMPLES) word = lane < S ? final_len[lane] : 0u;
    if (lane == KV_MAX_SAMPLES) word = n_refr;
    if (lane == KV_MAX_SAMPLES + 1) word = nk - n_case;
    if (lane == KV_MAX_SAMPLES + 2) word = flags;
    if (lane == KV_MAX_SAMPLES + 3) word = nk;
    if (lane < KV_SIMLIKE_RECORD_WORDS) p.records[(uint64_t)blockIdx.x * KV_SIMLIKE_RECORD_WORDS + lane] = word;
    if (lane < 3) p.ll[3ull * blockIdx.x + lane] = lane == 0 ? lldn : (lane == 1 ? llfp : llih);
}

}  // namespace

extern "C" int kv_simlike_score(kv_sketch *const *samples, int nsamples, kv_sketch *refr, const char *alt, const uint64_t *alt_offsets,
                                const char *ref, const uint64_t *ref_offsets, uint64_t n_calls, int ksize, double mu, double sigma,
                                double epsilon, int casemin, int ctrlmax, int caseabundlow, int ctrlabundhigh, int dropoutliers,
                                uint32_t *records, double *likelihoods, uint8_t *counts, uint8_t *refr_abunds)
{
    KV_REQUIRE(samples && refr && alt_offsets && ref_offsets && (n_calls == 0 || (alt && ref && records && likelihoods && counts && refr_abunds)),
               KV_ERR_ARG, "kv_simlike_score: null argument");
    KV_REQUIRE(nsamples >= 3 && nsamples <= KV_MAX_SAMPLES, KV_ERR_ARG, "kv_simlike_score: %d samples (a case and 2 to %d controls)", nsamples,
               KV_MAX_SAMPLES - 1);
    KV_REQUIRE(n_calls < 0x7FFFFFFFull, KV_ERR_ARG, "kv_simlike_score: %llu calls", (unsigned long long)n_calls);
    KV_REQUIRE(std::isfinite(mu) && std::isfinite(sigma) && std::isfinite(epsilon) && epsilon > 0.0 && epsilon < 1.0 && sigma > 0.0 && mu >= 0.0,
               KV_ERR_ARG, "kv_simlike_score: mu %g (at least 0), sigma %g (above 0), epsilon %g (between 0 and 1)", mu, sigma, epsilon);
    KV_REQUIRE(ksize >= 1 && ksize <= KV_MAX_K, KV_ERR_ARG, "k=%d out of range", ksize);
    SimParams p;
    memset(&p, 0, sizeof(p));
    for (int s = 0; s <= nsamples; ++s) {
        const kv_sketch *sk = s < nsamples ? samples[s] : refr;
        KV_REQUIRE(sk, KV_ERR_ARG, "kv_simlike_score: null sketch");
        KV_REQUIRE(sk->h.ksize == ksize, KV_ERR_ARG, "kv_simlike_score: a sketch of k = %d in a run of k = %d", sk->h.ksize, ksize);
        KV_REQUIRE(sk->h.hashfam != HF_TWOBIT || ksize <= 32, KV_ERR_ARG, "graph sketches need k <= 32 (got %d)", ksize);
        p.fam_mask |= 1 << sk->h.hashfam;
    }
    KV_STEP(kv_seq_offsets("kv_simlike_score", "window", alt_offsets, n_calls));
    KV_STEP(kv_seq_offsets("kv_simlike_score", "window", ref_offsets, n_calls));
    std::vector<SimCall> descs(n_calls);
    uint64_t total = 0;
    for (uint64_t c = 0; c < n_calls; ++c) {
        const uint64_t al = alt_offsets[c + 1] - alt_offsets[c], rl = ref_offsets[c + 1] - ref_offsets[c];
        KV_REQUIRE(al >= (uint64_t)ksize && rl >= (uint64_t)ksize, KV_ERR_ARG, "call %llu: windows of %llu and %llu bases, shorter than k = %d",
                   (unsigned long long)c, (unsigned long long)al, (unsigned long long)rl, ksize);
        KV_REQUIRE(al <= KV_SEQ_MAX_LEN && rl <= KV_SEQ_MAX_LEN, KV_ERR_ARG, "call %llu: windows of %llu and %llu bases (at most %u)",
                   (unsigned long long)c, (unsigned long long)al, (unsigned long long)rl, KV_SEQ_MAX_LEN);
        descs[c] = SimCall{alt_offsets[c], ref_offsets[c], total, (uint32_t)al, (uint32_t)rl};
        total += al - (uint64_t)ksize + 1;
    }
    if (n_calls == 0) return KV_OK;
    for (int s = 0; s <= nsamples; ++s) KV_STEP(kv_sketch_ready(s < nsamples ? samples[s] : refr));
    for (int s = 0; s < nsamples; ++s) p.sk[s] = samples[s]->d_desc;
    p.refr = refr->d_desc;
    p.refr_fam = refr->h.hashfam;

    // allocate and upload: a device buffer per piece, in the order of their sizes.  (One buffer carved into the seven, as kv_align_batch
    // and kv_call_scan have it, made the whole call of 10 000 windows 6 % slower: seven allocations below a megabyte beat one of four.)
    enum { SB_ALT, SB_REF, SB_CALLS, SB_REC, SB_LL, SB_COUNTS, SB_REFR, SB_PIECES };
    hipStream_t st = kv_stream();
    const uint64_t abytes = alt_offsets[n_calls], rbytes = ref_offsets[n_calls], cbytes = total * (uint64_t)nsamples;
    const size_t sizes[SB_PIECES] = {abytes, rbytes, n_calls * sizeof(SimCall), n_calls * KV_SIMLIKE_RECORD_WORDS * 4, n_calls * 3 * sizeof(double),
                                     cbytes, total};
    KvDevBuf d[SB_PIECES];
    hipError_t e = hipSuccess;
    for (int i = 0; i < SB_PIECES && e == hipSuccess; ++i) e = d[i].alloc(sizes[i]);
    KV_REQUIRE(e == hipSuccess, KV_ERR_HIP, "simlike buffers allocation failed: %s", hipGetErrorString(e));
    p.calls = d[SB_CALLS].as<SimCall>(); p.alt = d[SB_ALT].as<uint8_t>(); p.ref = d[SB_REF].as<uint8_t>();
    p.records = d[SB_REC].as<uint32_t>(); p.ll = d[SB_LL].as<double>(); p.counts = d[SB_COUNTS].as<uint8_t>(); p.refr_out = d[SB_REFR].as<uint8_t>();
    KV_HIP(hipMemcpyAsync(d[SB_ALT].p, alt, abytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d[SB_REF].p, ref, rbytes, hipMemcpyHostToDevice, st));
    KV_HIP(hipMemcpyAsync(d[SB_CALLS].p, descs.data(), n_calls * sizeof(SimCall), hipMemcpyHostToDevice, st));
    // (the lists' room behind their final lengths reads as zero)
    KV_HIP(hipMemsetAsync(p.counts, 0, cbytes, st));
    KV_HIP(hipMemsetAsync(p.refr_out, 0, total, st));
    p.mu = mu; p.sigma = sigma; p.epsilon = epsilon;
    p.nsamples = nsamples; p.ksize = ksize;
    p.casemin = casemin; p.ctrlmax = ctrlmax; p.caseabundlow = caseabundlow; p.ctrlabundhigh = ctrlabundhigh;
    p.dropoutliers = dropoutliers ? 1 : 0;
    {
        KvProfScope prof("k_simlike");
        hipLaunchKernelGGL(k_simlike, dim3((unsigned)n_calls), dim3(SIM_LANES), 0, st, p);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(records, p.records, n_calls * KV_SIMLIKE_RECORD_WORDS * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(likelihoods, p.ll, n_calls * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(counts, p.counts, cbytes, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(refr_abunds, p.refr_out, total, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}
