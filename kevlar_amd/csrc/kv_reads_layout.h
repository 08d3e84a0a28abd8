// kv_reads_layout.h -- how a batch of reads is laid out for the hashing kernels: word offsets and the tile table.
// The rule decides which k-mers every kernel sees, and this is its only statement.  Plain C++17 with no HIP in it:
// tests/harness/reads_layout_host.cpp compiles it for the host and tests/test_reads_layout.py checks it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/kvsketch.h"   // KV_MAX_K

// tile geometry of the hashing kernels
#define KV_TILE_MAX_READS 64
#define KV_TILE_LDS_BYTES 16384  // ASCII staging (forward + reverse complement) per tile: 64 reads of 100 bp
#define KV_READ_PAD 24           // over-read slack after each staged strand
#define KV_SEG_BASES 7680        // k-mer starts per segment tile: 2 x (7680 + KV_MAX_K - 1 + pad) bytes of ASCII fit the tile budget

// One unit of work of the hashing kernels: `count` whole reads starting at read `first`, or (seg != 0) the
// segment of read `first` whose k-mers START in [seg_start, seg_start + KV_SEG_BASES): the kernel stages
// KV_SEG_BASES + k - 1 bases, so every k-mer of a chromosome-length sequence belongs to exactly one tile
// whatever k is (the tile table itself does not depend on k).
struct TileDesc {
    uint32_t first, count, seg_start, seg;
};

struct KvReadsPlan {
    uint64_t n_words = 0, n_bases = 0;
    uint32_t max_len = 0;
    uint32_t tile_max_bases = 0;              // most bases any tile stages (a segment tile: at most KV_SEG_BASES + KV_MAX_K)
    uint32_t n_tiles = 0;                     // 0 only for a batch without reads (`tiles` then still holds one zero descriptor);
                                              // a read without bases still opens a run
    uint32_t uni_len = 0, uni_per_tile = 0;   // uniform batch: read i sits at word i * ((uni_len + 15) / 16) and tile t holds
                                              // reads [t * uni_per_tile, ...); 0 when the batch is not uniform
    bool closed_form = false;                 // uniform, and the caller asked for no tables: woff and tiles are left empty, the
                                              // caller writes them by the arithmetic above
    std::vector<uint64_t> woff;               // n_reads + 1 word offsets   } filled unless closed_form
    std::vector<TileDesc> tiles;              // never empty                }
};

// reads of `len` bases that fit one tile (at most KV_TILE_MAX_READS); 0: a read this long needs segment tiles
static inline uint32_t kv_reads_per_tile(uint32_t len)
{
    const uint64_t budget = KV_TILE_LDS_BYTES - 64, need = 2 * (((uint64_t)len + KV_READ_PAD + 3) & ~3ull);
    return (uint32_t)std::min<uint64_t>(KV_TILE_MAX_READS, budget / need);
}

// Tiles: consecutive reads whose staged ASCII (both strands, padded) fits the LDS budget; a sequence too long for one tile
// (contigs, the chromosomes of a reference genome counted into a mask) becomes a series of segment tiles of KV_SEG_BASES
// k-mer starts each.  Reads of one non-zero length that fit a tile make a uniform batch, whose layout is arithmetic:
// with uniform_tables == false the plan says closed_form, its woff / tiles stay empty and the caller writes them by that arithmetic
// (tile t = {t * uni_per_tile, min(uni_per_tile, n_reads - t * uni_per_tile), 0, 0}), which is what the loop below gives.
static inline KvReadsPlan kv_reads_plan(const uint32_t *lens, uint64_t n_reads, bool uniform_tables)
{
    KvReadsPlan p;
    bool same = n_reads > 0 && lens[0] > 0 && kv_reads_per_tile(lens[0]) > 0;
    for (uint64_t i = 1; same && i < n_reads; ++i) same = lens[i] == lens[0];
    if (same) {
        p.uni_len = lens[0];
        p.uni_per_tile = kv_reads_per_tile(lens[0]);
        if (!uniform_tables) {
            p.closed_form = true;
            p.n_words = n_reads * (((uint64_t)p.uni_len + 15) / 16);
            p.n_bases = n_reads * (uint64_t)p.uni_len;
            p.max_len = p.uni_len;
            p.tile_max_bases = (uint32_t)std::min<uint64_t>(p.uni_per_tile, n_reads) * p.uni_len;
            p.n_tiles = (uint32_t)((n_reads + p.uni_per_tile - 1) / p.uni_per_tile);
            return p;
        }
    }
    p.woff.resize(n_reads + 1);
    const uint32_t budget = KV_TILE_LDS_BYTES - 64;
    uint32_t used = 0, count = 0, first = 0, run_bases = 0;
    auto close_run = [&](uint32_t next_first) {
        if (count) p.tiles.push_back(TileDesc{first, count, 0u, 0u});
        p.tile_max_bases = std::max(p.tile_max_bases, run_bases);
        used = 0; count = 0; first = next_first; run_bases = 0;
    };
    for (uint64_t i = 0; i < n_reads; ++i) {
        const uint32_t len = lens[i];
        p.woff[i] = p.n_words;
        p.n_words += ((uint64_t)len + 15) / 16;
        p.n_bases += len;
        p.max_len = std::max(p.max_len, len);
        if (kv_reads_per_tile(len) == 0) {
            close_run((uint32_t)i + 1);
            for (uint32_t start = 0; start < len; start += KV_SEG_BASES) p.tiles.push_back(TileDesc{(uint32_t)i, 1u, start, 1u});
            p.tile_max_bases = std::max<uint32_t>(p.tile_max_bases, std::min<uint32_t>(len, KV_SEG_BASES + KV_MAX_K));
            continue;
        }
        const uint32_t need = 2 * ((len + KV_READ_PAD + 3) & ~3u);
        if (count > 0 && (count == KV_TILE_MAX_READS || used + need > budget)) close_run((uint32_t)i);
        if (count == 0) first = (uint32_t)i;
        used += need; count += 1; run_bases += len;
    }
    close_run((uint32_t)n_reads);
    p.woff[n_reads] = p.n_words;
    p.n_tiles = (uint32_t)p.tiles.size();
    if (p.tiles.empty()) p.tiles.push_back(TileDesc{0u, 0u, 0u, 0u});
    return p;
}
