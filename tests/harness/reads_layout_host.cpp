// Host-side harness for kevlar_amd/csrc/kv_reads_layout.h (compiled as plain C++ by tests/test_reads_layout.py):
// the layout planner of a read batch behind a C ABI, so that Python can compare it with a restatement of the rule.
#include <stdint.h>
#include <string.h>
#include "../../kevlar_amd/csrc/kv_reads_layout.h"

extern "C" {
// out[0 .. 6]: KV_TILE_LDS_BYTES, KV_TILE_MAX_READS, KV_READ_PAD, KV_SEG_BASES, KV_MAX_K, sizeof(TileDesc), sizeof(uint64_t)
void h_layout_constants(uint64_t *out)
{
    const uint64_t c[7] = {KV_TILE_LDS_BYTES, KV_TILE_MAX_READS, KV_READ_PAD, KV_SEG_BASES, KV_MAX_K, sizeof(TileDesc), sizeof(uint64_t)};
    memcpy(out, c, sizeof(c));
}

uint32_t h_reads_per_tile(uint32_t len) { return kv_reads_per_tile(len); }

// scalars[0 .. 7]: n_words, n_bases, max_len, tile_max_bases, n_tiles, uni_len, uni_per_tile, closed_form; the return value is the number of
// tile descriptors the plan holds and *n_woff the number of word offsets (both 0 when the plan left its tables out).  At most
// woff_cap offsets go to woff and tile_cap descriptors, four words each, to tiles.
uint64_t h_reads_plan(const uint32_t *lens, uint64_t n_reads, int uniform_tables, uint64_t *scalars, uint64_t *woff, uint64_t woff_cap,
                      uint64_t *n_woff, uint32_t *tiles, uint64_t tile_cap)
{
    const KvReadsPlan p = kv_reads_plan(lens, n_reads, uniform_tables != 0);
    const uint64_t s[8] = {p.n_words, p.n_bases, p.max_len, p.tile_max_bases, p.n_tiles, p.uni_len, p.uni_per_tile, p.closed_form};
    memcpy(scalars, s, sizeof(s));
    *n_woff = p.woff.size();
    for (uint64_t i = 0; i < p.woff.size() && i < woff_cap; ++i) woff[i] = p.woff[i];
    for (uint64_t t = 0; t < p.tiles.size() && t < tile_cap; ++t) {
        const uint32_t d[4] = {p.tiles[t].first, p.tiles[t].count, p.tiles[t].seg_start, p.tiles[t].seg};
        memcpy(tiles + 4 * t, d, sizeof(d));
    }
    return p.tiles.size();
}
}
