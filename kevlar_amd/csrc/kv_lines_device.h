// kv_lines_device.h -- the line kernels of text that sits in HBM, shared by the FASTQ reader (kv_fastq.hip) and the FASTA
// splitter (kv_genome.hip): newlines per 16-KB chunk, the byte offset of every line start, and the gather of byte ranges.
// Include inside a .hip file, behind kv_device.h.
#pragma once
#include "kv_device.h"

namespace {

#define LN_CHUNK 16384u           // bytes per line-counting workgroup
#define LN_THREADS 256

// bit b of the result: byte b of the 16 is a newline
__device__ __forceinline__ uint32_t newline_mask16(const uint4 v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = w[q] ^ 0x0a0a0a0au;                                    // newline bytes become zero
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 exactly in the zero bytes
        mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    return mask;
}

__device__ __forceinline__ uint32_t newline_mask_at(const uint8_t *__restrict__ text, uint64_t at, uint64_t n)
{
    if (at + 16 <= n) return newline_mask16(*(const uint4 *)(text + at));       // `at` is a multiple of 16 in an aligned buffer
    uint32_t mask = 0;
    for (uint32_t b = 0; b < 16 && at + b < n; ++b) mask |= (text[at + b] == '\n' ? 1u : 0u) << b;
    return mask;
}

// newlines in text[0, n) per chunk
__global__ __launch_bounds__(LN_THREADS) void k_count_lines(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wsum[LN_THREADS / 64];
    const uint64_t c0 = (uint64_t)blockIdx.x * LN_CHUNK;
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x * 16u; i < LN_CHUNK; i += LN_THREADS * 16u) mine += (uint32_t)__popc(newline_mask_at(text, c0 + i, n));
    mine = (uint32_t)wave_sum_u64(mine);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// line_start[l + 1] = offset behind the l-th newline (line_start[0] = 0 is set by the host); only the first
// `max_lines` lines are recorded
__global__ __launch_bounds__(LN_THREADS) void k_line_starts(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ base,
                                                            uint64_t max_lines, uint64_t *__restrict__ line_start)
{
    __shared__ uint32_t wsum[LN_THREADS / 64];
    const uint64_t c0 = (uint64_t)blockIdx.x * LN_CHUNK;
    uint64_t line = base[blockIdx.x];
    if (line >= max_lines) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i0 = 0; i0 < LN_CHUNK; i0 += LN_THREADS * 16u) {
        const uint64_t at = c0 + i0 + threadIdx.x * 16u;
        uint32_t mask = newline_mask_at(text, at, n);
        const uint32_t c = (uint32_t)__popc(mask);
        const uint32_t incl = wave_incl_scan(c);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < LN_THREADS / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        uint64_t l = line + before + incl - c;
        while (mask) {
            const uint32_t b = (uint32_t)__ffs((int)mask) - 1u;
            mask &= mask - 1u;
            if (l + 1 <= max_lines) line_start[l + 1] = at + b + 1;
            ++l;
        }
        line += all;
        __syncthreads();
    }
}

// one workgroup per requested range ext[2 i] .. ext[2 i + 1] of the text: its bytes to out[dst[i] ..]
__global__ __launch_bounds__(64) void k_record_copy(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext, const uint64_t *__restrict__ dst,
                                                    uint64_t n, uint8_t *__restrict__ out)
{
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint64_t a = ext[2 * i], len = ext[2 * i + 1] - a, to = dst[i];
        for (uint64_t j = threadIdx.x; j < len; j += 64) out[to + j] = text[a + j];
    }
}

}  // namespace
