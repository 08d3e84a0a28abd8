// kv_roll2bit_device.h -- the 2-bit key of a window of bases as the exact-match kernels keep it (kv_localize.hip, kv_assemble.hip):
// the code of a byte, and the forward and reverse-complement key of a window rolled one base at a time.  Include inside a .hip file.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

// A=0 C=1 G=2 T=3 (the order of the letters, so the smaller key is the smaller string: kevlar.revcommin); lower case counts as upper
__device__ __forceinline__ uint32_t loc_code(uint32_t byte, uint32_t &valid)
{
    const uint32_t u = byte & 0xDFu;
    valid = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
    return ((u >> 1) & 3u) ^ ((u >> 2) & 1u);
}

// forward and reverse-complement key of a window as 2Z-bit numbers in W 64-bit words, most significant word first
template <int W>
struct LocRoll {
    uint64_t f[W], r[W];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int w = 0; w < W; ++w) f[w] = r[w] = 0;
    }
    // topbits = 2Z - 64 (W - 1): the bits of the key that sit in word 0
    __device__ __forceinline__ void push(uint32_t c, int topbits)
    {
#pragma unroll
        for (int w = 0; w < W - 1; ++w) f[w] = (f[w] << 2) | (f[w + 1] >> 62);
        f[W - 1] = (f[W - 1] << 2) | c;
        if (topbits < 64) f[0] &= (1ull << topbits) - 1ull;
#pragma unroll
        for (int w = W - 1; w > 0; --w) r[w] = (r[w] >> 2) | (r[w - 1] << 62);
        r[0] = (r[0] >> 2) | ((uint64_t)(3u - c) << (topbits - 2));
    }
    __device__ __forceinline__ void canonical(uint64_t *key) const
    {
        bool f_less = false, decided = false;
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (!decided && f[w] != r[w]) { f_less = f[w] < r[w]; decided = true; }
        const bool use_f = f_less || !decided;
#pragma unroll
        for (int w = 0; w < W; ++w) key[w] = use_f ? f[w] : r[w];
    }
};

}  // namespace
