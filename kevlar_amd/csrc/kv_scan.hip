// kv_scan.hip -- the one counts-to-bases kernel: exclusive scan of n 32-bit counts into n + 1 64-bit bases, the total behind
// the last.  The novel scan lists its hits per tile with it and the FASTQ reader its lines per chunk.
#include "kv_device.h"

namespace {

// exclusive scan of n 32-bit counts into 64-bit bases (single 1024-thread workgroup)
__global__ __launch_bounds__(1024) void k_excl_scan_u32(const uint32_t *counts, uint32_t n, uint64_t *base)
{
    // One workgroup; a wave takes 64 * PER consecutive counts per round, 64 at a time: consecutive lanes on consecutive counts, so a
    // load is one 256-byte piece of memory and a store one of 512, and the wave's running total rides along from one 64 to the next.
    // (A thread on PER consecutive counts -- eight 4-byte loads 32 bytes apart from its neighbour's, eight 8-byte stores 64 bytes apart --
    // made every round ~7 us of single-CU memory pipe: 0.108 ms for the 117 k tiles of config 2.)  The next round's counts are
    // requested before this round's barriers.
    constexpr uint32_t PER = 8;
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t nxt[PER];
    auto request = [&](uint32_t start) {
        const uint32_t i0 = start + wave * 64u * PER + lane;
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) nxt[u] = i0 + u * 64u < n ? counts[i0 + u * 64u] : 0u;
    };
    request(0);
    for (uint32_t start = 0; start < n; start += 1024 * PER) {
        const uint32_t i0 = start + wave * 64u * PER + lane;
        uint32_t c[PER];
        uint64_t excl[PER];                             // exclusive prefix inside the wave's stretch
        uint64_t run = 0;                               // total of the pieces in front (wave-uniform)
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {
            c[u] = nxt[u];
            uint64_t incl = c[u];                       // (wave_incl_scan written out: the helper costs this kernel three VGPRs)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t up = __shfl_up(incl, d);
                if (lane >= (uint32_t)d) incl += up;
            }
            excl[u] = run + incl - c[u];
            run += __shfl(incl, 63);
        }
        if (start + 1024 * PER < n) request(start + 1024 * PER);
        if (lane == 0) wsum[wave] = run;
        __syncthreads();
        const uint64_t before = waves_before(wsum, wave, (uint64_t)carry);
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u)
            if (i0 + u * 64u < n) base[i0 + u * 64u] = before + excl[u];
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + run;
        __syncthreads();
    }
    if (threadIdx.x == 0) base[n] = carry;
}

}  // namespace

void kv_excl_scan_launch(const uint32_t *d_counts, uint32_t n, uint64_t *d_base, hipStream_t st)
{
    hipLaunchKernelGGL(k_excl_scan_u32, dim3(1), dim3(1024), 0, st, d_counts, n, d_base);
}

extern "C" int kv_excl_scan_u32(const uint32_t *d_counts, uint32_t n, uint64_t *d_base)
{
    KV_REQUIRE(d_base && (d_counts || n == 0), KV_ERR_ARG, "kv_excl_scan_u32: null buffer");
    hipStream_t st = kv_stream();
    kv_excl_scan_launch(d_counts, n, d_base, st);
    KV_HIP(hipGetLastError());
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}
