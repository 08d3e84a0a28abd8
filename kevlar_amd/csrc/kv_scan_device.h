// kv_scan_device.h -- the one prefix sum of the kernels: inclusive over the 64 lanes of a wave, and the wave totals in front of a
// wave for the workgroup-wide form.  A caller derives exclusive = inclusive - own and total = __shfl(incl, 63), writes its wave's
// total to an LDS array of its own and places the barrier itself (several kernels put other LDS writes under the same one).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

// T: uint32_t or uint64_t
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// `before` plus the totals of the waves in front of `wave` (wsum[w]: total of wave w, written before the caller's barrier)
template <typename T, typename W>
__device__ __forceinline__ T waves_before(const T *wsum, W wave, T before = 0)
{
    for (W w = 0; w < wave; ++w) before += wsum[w];
    return before;
}

}  // namespace
