// kv_varfilter_plan.h -- the host rules of `kevlar varfilter` (kv_varfilter.hip), free of HIP: the bytes that separate tokens, the
// number grammar, the hash and the open-addressing table of the chromosome names, what the arguments of a call index must satisfy,
// the workgroup tile a chunk of BED text is scanned in, and where a buffer of text is cut into a chunk that ends at a line end.
// The byte rules are marked VF_HD: the device code of kv_varfilter.hip uses the same functions.  Plain C++17:
// tests/harness/varfilter_plan_host.cpp compiles it for the host, tests/test_varfilter_reference.py checks the edges.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/kvsketch.h"
#include "kv_require.h"

#if defined(__HIPCC__)
#define VF_HD __host__ __device__ __forceinline__
#define VF_HDM __host__ __device__ __forceinline__
#else
#define VF_HD static inline
#define VF_HDM inline
#endif

#define VF_THREADS 256
#define VF_TILE_SMALL 4096u                 // bytes of text per workgroup: more workgroups from a small chunk
#define VF_TILE_LARGE 16384u                // the tile's lines are dealt to its 256 lanes: 2.5 each at 25 bytes a line, fewer idle lanes
#ifndef VF_LARGE_FROM
#define VF_LARGE_FROM (4ull << 20)          // chunk size from which the large tile still gives every CU a workgroup (256 tiles)
#endif
#define VF_LDS_BEFORE 16u                   // bytes staged in front of a tile (the byte that ends the previous line is among them)
#define VF_LDS_AFTER 240u                   // ... and behind it: a line that starts in the tile is usually parsed out of LDS alone
#define VF_MAX_CHUNK (1ull << 40)
#define VF_MAX_CALLS 0xFFFFFFF0ull          // call numbers are 32-bit
#define VF_NO_CHROM 0xFFFFFFFFu             // "not among the calls' chromosomes"; also an empty slot of the name table
#define VF_NO_OFFSET 0xFFFFFFFFFFFFFFFFull  // no bad line
#define VF_TABLE_LEAST 64

// 0x09-0x0d, 0x1c-0x1f and the space: what Python's str.strip() and \s take among the ASCII bytes ('\n' included: it ends a token
// like the others, and a line as well)
VF_HD bool vf_is_sep(uint32_t c) { return (c - 9u) <= 4u || (c - 0x1cu) <= 4u; }

// FNV-1a over the bytes of a name, then a finisher; a slot of the table is picked by it, a hit never decided by it
VF_HD uint64_t vf_hash_init() { return 0xcbf29ce484222325ull; }
VF_HD uint64_t vf_hash_step(uint64_t h, uint32_t byte) { return (h ^ (uint64_t)byte) * 0x100000001b3ull; }
VF_HD uint64_t vf_hash_finish(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

// [+-]?[0-9]+ with a value within int64, a byte at a time: feed() every byte of the token, then ok() and value()
struct VfNumber {
    uint64_t mag = 0;           // magnitude so far, at most 2^63
    uint32_t digits = 0, neg = 0, bad = 0;
    VF_HDM void feed(uint32_t c, bool first)
    {
        if (first && (c == '+' || c == '-')) { neg = c == '-'; return; }
        const uint32_t d = c - '0';
        if (d > 9u) { bad = 1; return; }
        ++digits;                                                                   // (2^32 leading zeros wrap: a chunk is shorter)
        // 2^63 = 9223372036854775808: the last step that stays at or below it
        if (mag > 922337203685477580ull || (mag == 922337203685477580ull && d > 8u)) { bad = 1; return; }
        mag = mag * 10u + d;
    }
    VF_HDM bool ok() const { return !bad && digits > 0 && (neg || mag < (1ull << 63)); }
    VF_HDM int64_t value() const { return (int64_t)(neg ? 0ull - mag : mag); }
};

// a region (s, e) hits a call (a, b): intervaltree >= 3.0.2, where an empty or inverted query finds nothing
VF_HD bool vf_overlap(int64_t s, int64_t e, int64_t a, int64_t b) { return s < e && a < e && b > s; }

static inline uint64_t vf_table_cap(uint64_t n_names)
{
    uint64_t c = VF_TABLE_LEAST;
    while (c < 2 * n_names + 16) c <<= 1;       // at most half full: a probe ends at an empty slot
    return c;
}

static inline uint64_t vf_name_hash(const uint8_t *name, uint64_t len)
{
    uint64_t h = vf_hash_init();
    for (uint64_t i = 0; i < len; ++i) h = vf_hash_step(h, name[i]);
    return vf_hash_finish(h);
}

// the id of the name in the table, or VF_NO_CHROM: the walk the device repeats on the bytes of a token
static inline uint32_t vf_table_find(const std::vector<uint32_t> &table, const uint8_t *names, const uint64_t *name_off, const uint8_t *name,
                                     uint64_t len)
{
    const uint64_t mask = table.size() - 1;
    for (uint64_t s = vf_name_hash(name, len) & mask;; s = (s + 1) & mask) {
        const uint32_t id = table[s];
        if (id == VF_NO_CHROM) return VF_NO_CHROM;
        if (name_off[id + 1] - name_off[id] == len && memcmp(names + name_off[id], name, len) == 0) return id;
    }
}

// slot -> chromosome id; the names must be distinct (two ids of one name would split its calls)
static inline int vf_table_build(const uint8_t *names, const uint64_t *name_off, uint64_t n_names, std::vector<uint32_t> &table)
{
    KV_REQUIRE(n_names < VF_NO_CHROM, KV_ERR_ARG, "kv_varfilter_create: %llu chromosome names", (unsigned long long)n_names);
    KV_REQUIRE(n_names == 0 || name_off, KV_ERR_ARG, "kv_varfilter_create: null argument");
    for (uint64_t c = 0; c < n_names; ++c)
        KV_REQUIRE(name_off[c] <= name_off[c + 1], KV_ERR_ARG, "kv_varfilter_create: name offsets must not decrease");
    KV_REQUIRE(n_names == 0 || name_off[n_names] == 0 || names, KV_ERR_ARG, "kv_varfilter_create: null argument");
    table.assign(vf_table_cap(n_names), VF_NO_CHROM);
    const uint64_t mask = table.size() - 1;
    for (uint64_t c = 0; c < n_names; ++c) {
        const uint8_t *name = names + name_off[c];
        const uint64_t len = name_off[c + 1] - name_off[c];
        KV_REQUIRE(vf_table_find(table, names, name_off, name, len) == VF_NO_CHROM, KV_ERR_ARG,
                   "kv_varfilter_create: chromosome name %llu repeats an earlier one", (unsigned long long)c);
        uint64_t s = vf_name_hash(name, len) & mask;
        while (table[s] != VF_NO_CHROM) s = (s + 1) & mask;
        table[s] = (uint32_t)c;
    }
    return KV_OK;
}

static inline int vf_check_calls(const uint32_t *call_chrom, const int64_t *call_start, const int64_t *call_end, uint64_t n_calls,
                                 uint64_t n_names)
{
    KV_REQUIRE(n_calls <= VF_MAX_CALLS, KV_ERR_CAPACITY, "kv_varfilter_create: %llu calls in one index", (unsigned long long)n_calls);
    KV_REQUIRE(n_calls == 0 || (call_chrom && call_start && call_end), KV_ERR_ARG, "kv_varfilter_create: null argument");
    for (uint64_t i = 0; i < n_calls; ++i)
        KV_REQUIRE(call_chrom[i] < n_names, KV_ERR_ARG, "kv_varfilter_create: call %llu is on chromosome %u of %llu",
                   (unsigned long long)i, call_chrom[i], (unsigned long long)n_names);
    return KV_OK;
}

static inline int vf_check_regions(const uint32_t *chrom_id, uint64_t n, uint64_t n_names, uint64_t *n_known)
{
    *n_known = 0;
    for (uint64_t i = 0; i < n; ++i) {
        KV_REQUIRE(chrom_id[i] < n_names || chrom_id[i] == VF_NO_CHROM, KV_ERR_ARG, "kv_varfilter_regions: region %llu is on chromosome %u of %llu",
                   (unsigned long long)i, chrom_id[i], (unsigned long long)n_names);
        *n_known += chrom_id[i] != VF_NO_CHROM;
    }
    return KV_OK;
}

// the tile of a chunk of n_bytes, and how many workgroups scan it
static inline uint32_t vf_tile_bytes(uint64_t n_bytes) { return n_bytes >= VF_LARGE_FROM ? VF_TILE_LARGE : VF_TILE_SMALL; }
static inline uint64_t vf_n_tiles(uint64_t n_bytes, uint32_t tile) { return (n_bytes + tile - 1) / tile; }
// non-empty lines of a tile: each has a byte and the '\n' behind it, the last line of a text may lack that
static inline uint32_t vf_tile_lines(uint32_t tile) { return tile / 2 + 1; }

// Where a buffer of text is cut: the chunk is buf[0 .. cut), it ends behind the last '\n' of the buffer, or with the buffer when
// the file ends there.  0: no line ends in the buffer yet (the caller reads on: a line longer than a chunk grows the chunk).
static inline uint64_t vf_chunk_cut(const uint8_t *buf, uint64_t n, int at_eof)
{
    if (at_eof) return n;
    while (n > 0 && buf[n - 1] != '\n') --n;
    return n;
}
