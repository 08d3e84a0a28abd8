// kv_inflate_device.h -- the DEFLATE pieces both inflaters share (kv_inflate.hip: one wavefront per BGZF member;
// kv_gunzip.hip: one wavefront per stretch of an ordinary gzip stream): the bit reader, canonical Huffman tables in LDS, the
// reader of a block's header and the wave-uniform symbol decode.  Device code only.
//
// What is NOT here, on purpose: the two symbol loops, their flush lambdas, their match copies and their stored-block paths.
// They store different things (bytes; 16-bit symbols with markers for sources in front of the stretch), stop on different
// conditions (isize; cap, target starts, member trailers) and report differently (failed; five status codes): one loop
// would branch on its caller at every one of those points, inside kernels held to exactly 64 VGPRs with spills.  The ten
// lines that turn a length symbol into (length, distance) are in both loops as well: as one function here they made
// k_gz_decode<10, true> and k_inflate measurably slower (profiles/README.md has the figures).
// Nor k_gz_sync's LaneBits / lane_symbol: those are divergent reads, a position per lane, not this scalar walk.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace {

#define INF_FAST_LL 10          // bits of the literal/length lookup table
#define INF_FAST_D 8            // ... of the distance table
#define INF_MAX_OUT 65536u

struct BitReader {
    const uint32_t *words;      // aligned words of the payload
    uint32_t next;              // index of the next word to take
    uint64_t buf;               // bits not yet consumed, LSB first
    uint32_t cnt;               // how many
    uint32_t ahead;             // words[next], already loaded (hides the load behind the decode)
};

__device__ __forceinline__ void br_init(BitReader &br, const uint8_t *payload)
{
    const uint64_t addr = (uint64_t)payload;
    const uint32_t mis = (uint32_t)(addr & 3u);
    br.words = (const uint32_t *)(addr - mis);
    br.buf = (uint64_t)(br.words[0] >> (8u * mis));
    br.cnt = 32u - 8u * mis;
    br.next = 1;
    br.ahead = br.words[1];
}

__device__ __forceinline__ void br_need(BitReader &br, uint32_t n)   // n <= 32
{
    if (br.cnt < n) {
        br.buf |= (uint64_t)br.ahead << br.cnt;
        br.cnt += 32u;
        br.next += 1;
        br.ahead = br.words[br.next];
    }
}

__device__ __forceinline__ uint32_t br_bits(BitReader &br, uint32_t n)   // n <= 16
{
    br_need(br, n);
    const uint32_t v = (uint32_t)br.buf & ((1u << n) - 1u);
    br.buf >>= n;
    br.cnt -= n;
    return v;
}

// The code tables of the block being decoded, in LDS.  With a window of 1 K bytes (kv_inflate.hip, FAST_LL 10) or 1 K symbols
// (kv_gunzip.hip, FAST_LL 9) in front of it this makes 4.6 KB a workgroup: 32 workgroups per CU, 8 waves per SIMD, the most
// the hardware takes -- a table bit more on either side and a CU holds fewer decoders.
template <int FAST_LL>
struct InfCodes {
    uint16_t ll_table[1 << FAST_LL];
    uint16_t d_table[1 << INF_FAST_D];
    uint16_t ll_count[16], d_count[16];
    uint16_t ll_symbol[288], d_symbol[32];
    uint8_t lengths[352];          // 19 code-length codes, then up to 286 + 30 code lengths
};

// canonical Huffman code of `n` symbols with the given lengths: count[len], symbols sorted by (len, symbol), and the
// lookup table of the codes of at most `fast` bits (entry = symbol | len << 9; 0 = longer code).  Returns false if the
// lengths oversubscribe the code space, or leave some of it unused where zlib's inflate (inftrees.c) does not take that:
// the code-length code must be complete; a literal/length or distance code may be incomplete only if no code is longer
// than one bit (a single code of length 1, or none at all); the fixed distance code (30 of 32 codes) is as it is.
enum { INF_CODE_PRECODE = 0, INF_CODE_BLOCK = 1, INF_CODE_FIXED = 2 };
__device__ bool build_code(const uint8_t *lengths, int n, uint16_t *count, uint16_t *symbol, uint16_t *table, int fast, int kind)
{
    for (int l = 0; l <= 15; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lengths[s]]++;
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return false;
    }
    if (left > 0 && kind != INF_CODE_FIXED) {
        if (kind == INF_CODE_PRECODE) return false;
        for (int l = 2; l <= 15; ++l)
            if (count[l]) return false;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
    for (int s = 0; s < n; ++s)
        if (lengths[s]) symbol[offs[lengths[s]]++] = (uint16_t)s;
    for (int i = 0; i < (1 << fast); ++i) table[i] = 0;
    // codes in canonical order: first code of each length, then consecutive
    uint32_t code = 0, index = 0;
    for (int l = 1; l <= fast; ++l) {
        for (uint32_t j = 0; j < count[l]; ++j, ++code, ++index) {
            const uint32_t rev = __brev(code) >> (32 - l);            // the stream carries a code's bits MSB first
            const uint16_t entry = (uint16_t)(symbol[index] | (l << 9));
            for (uint32_t fill = rev; fill < (1u << fast); fill += 1u << l) table[fill] = entry;
        }
        code <<= 1;
    }
    return true;
}

// One symbol.  Every lane runs this with the same (wave-uniform) reader state, so the arithmetic lives on the scalar unit;
// only the table word comes through a vector register and is made uniform again at once.
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
__device__ __forceinline__ int decode_sym(BitReader &br, const uint16_t *count, const uint16_t *symbol, const uint16_t *table, int fast)
{
    br_need(br, 15);
    const uint32_t e = INF_UNI(table[(uint32_t)br.buf & ((1u << fast) - 1u)]);
    if (e) {
        const uint32_t l = e >> 9;
        br.buf >>= l;
        br.cnt -= l;
        return (int)(e & 0x1ffu);
    }
    // a code longer than the table: bit by bit through the canonical counts
    int code = 0, first = 0, index = 0;
    uint64_t bits = br.buf;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = (int)INF_UNI(count[l]);
        if (code - c < first) {
            br.buf >>= l;
            br.cnt -= l;
            return (int)INF_UNI(symbol[index + (code - first)]);
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// The length / distance code tables of RFC 1951 section 3.2.5 as arithmetic: a table in constant memory is a vector load
// here, and the s_waitcnt vmcnt(0) behind it also waits for every text store the wave still has in flight -- a
// microsecond per match.  (tests/test_gpu_deflate.py compares the text with zlib over every length and distance symbol, each
// at its smallest and largest extra bits: group 'tables' of tests/deflate_common.py.)
__device__ __forceinline__ uint32_t inf_len_extra(uint32_t ls) { return ls < 8u || ls == 28u ? 0u : (ls - 4u) >> 2; }
__device__ __forceinline__ uint32_t inf_len_base(uint32_t ls)
{
    return ls < 8u ? 3u + ls : ls == 28u ? 258u : 3u + ((4u + (ls & 3u)) << ((ls - 4u) >> 2));
}
__device__ __forceinline__ uint32_t inf_dist_extra(uint32_t ds) { return ds < 4u ? 0u : (ds >> 1) - 1u; }
__device__ __forceinline__ uint32_t inf_dist_base(uint32_t ds) { return ds < 4u ? 1u + ds : 1u + ((2u + (ds & 1u)) << ((ds >> 1) - 1u)); }
// the order the code-length code's own lengths arrive in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
__device__ __forceinline__ uint32_t inf_clen_order(uint32_t s)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((s < 12u ? lo >> (5u * s) : hi >> (5u * (s - 12u))) & 31u);
}

// The Huffman codes of a block whose 3 header bits have been read (btype 1: the fixed ones, 2: the ones the block spells
// out) -> lookup tables in LDS.  All lanes take part; returns 0 for an invalid description.
template <int FAST_LL>
__device__ uint32_t inf_block_codes(BitReader &br, InfCodes<FAST_LL> &c, uint32_t lane, uint32_t btype)
{
    uint32_t ok = 1;
    if (btype == 1) {
        if (lane == 0) {
            for (int s = 0; s < 144; ++s) c.lengths[s] = 8;
            for (int s = 144; s < 256; ++s) c.lengths[s] = 9;
            for (int s = 256; s < 280; ++s) c.lengths[s] = 7;
            for (int s = 280; s < 288; ++s) c.lengths[s] = 8;
            ok = build_code(c.lengths, 288, c.ll_count, c.ll_symbol, c.ll_table, FAST_LL, INF_CODE_FIXED);
            for (int s = 0; s < 30; ++s) c.lengths[s] = 5;
            ok = ok && build_code(c.lengths, 30, c.d_count, c.d_symbol, c.d_table, INF_FAST_D, INF_CODE_FIXED);
        }
    } else {
        const uint32_t nlen = br_bits(br, 5) + 257, ndist = br_bits(br, 5) + 1, ncode = br_bits(br, 4) + 4;
        if (nlen > 286 || ndist > 30) return 0;
        if (lane < 19) c.lengths[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t s = 0; s < ncode; ++s) {
            const uint32_t v = br_bits(br, 3);
            if (lane == 0) c.lengths[inf_clen_order(s)] = (uint8_t)v;
        }
        // the code-length code lives in the distance arrays for a moment
        if (lane == 0) ok = build_code(c.lengths, 19, c.d_count, c.d_symbol, c.d_table, 7, INF_CODE_PRECODE);
        ok = INF_UNI(ok);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t idx = 0, prev = 0;
        while (ok && idx < nlen + ndist) {
            const int sym = decode_sym(br, c.d_count, c.d_symbol, c.d_table, 7);
            if (sym < 0) { ok = 0; break; }
            uint32_t rep = 1, val = (uint32_t)sym;
            if (sym == 16) {
                if (idx == 0) { ok = 0; break; }
                val = prev;
                rep = 3 + br_bits(br, 2);
            } else if (sym == 17) { val = 0; rep = 3 + br_bits(br, 3); }
            else if (sym == 18) { val = 0; rep = 11 + br_bits(br, 7); }
            if (idx + rep > nlen + ndist) { ok = 0; break; }
            if (lane < rep) c.lengths[19 + idx + lane] = (uint8_t)val;       // rep <= 138: at most three rows
            if (lane + 64 < rep) c.lengths[19 + idx + lane + 64] = (uint8_t)val;
            if (lane + 128 < rep) c.lengths[19 + idx + lane + 128] = (uint8_t)val;
            idx += rep;
            prev = val;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0 && ok) {
            ok = c.lengths[19 + 256] != 0;      // a block without an end code cannot end
            ok = ok && build_code(c.lengths + 19, (int)nlen, c.ll_count, c.ll_symbol, c.ll_table, FAST_LL, INF_CODE_BLOCK);
            ok = ok && build_code(c.lengths + 19 + nlen, (int)ndist, c.d_count, c.d_symbol, c.d_table, INF_FAST_D, INF_CODE_BLOCK);
        }
    }
    ok = INF_UNI(ok);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return ok;
}

}  // namespace
