// Host-side harness for kevlar_amd/csrc/kv_varfilter_plan.h (compiled as plain C++ by tests/test_varfilter_reference.py): the byte
// rules, the name table, the argument checks, the tile choice and the chunk cut behind a C ABI, so that Python can compare them with
// a restatement.  With -DKV_HARNESS_MAIN the file is a program: seeded inputs through the same functions, for a run under the host
// sanitizers.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../kevlar_amd/csrc/kv_varfilter_plan.h"

static char g_error[512];
void kv_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

extern "C" {
const char *h_last_error() { return g_error; }

void h_constants(uint64_t *out)
{
    const uint64_t c[10] = {VF_THREADS, VF_TILE_SMALL, VF_TILE_LARGE, VF_LARGE_FROM, VF_LDS_BEFORE, VF_LDS_AFTER, VF_MAX_CHUNK, VF_MAX_CALLS,
                            VF_NO_CHROM, VF_TABLE_LEAST};
    memcpy(out, c, sizeof(c));
}

int h_is_sep(uint32_t c) { return vf_is_sep(c); }
int h_overlap(int64_t s, int64_t e, int64_t a, int64_t b) { return vf_overlap(s, e, a, b); }

// 1 and *value when the token is a number of the grammar
int h_number(const uint8_t *token, uint64_t len, int64_t *value)
{
    VfNumber v;
    for (uint64_t i = 0; i < len; ++i) v.feed(token[i], i == 0);
    if (!v.ok()) return 0;
    *value = v.value();
    return 1;
}

uint64_t h_table_cap(uint64_t n_names) { return vf_table_cap(n_names); }
uint64_t h_name_hash(const uint8_t *name, uint64_t len) { return vf_name_hash(name, len); }

// ids_out[q] = the id of query q in the table built of the names
int h_table(const uint8_t *names, const uint64_t *name_off, uint64_t n_names, const uint8_t *queries, const uint64_t *query_off, uint64_t n_queries,
            uint32_t *ids_out, uint64_t *slots_used)
{
    std::vector<uint32_t> table;
    g_error[0] = 0;
    KV_STEP(vf_table_build(names, name_off, n_names, table));
    uint64_t used = 0;
    for (uint32_t id : table) used += id != VF_NO_CHROM;
    *slots_used = used;
    for (uint64_t q = 0; q < n_queries; ++q)
        ids_out[q] = vf_table_find(table, names, name_off, queries + query_off[q], query_off[q + 1] - query_off[q]);
    return KV_OK;
}

int h_check_calls(const uint32_t *call_chrom, const int64_t *call_start, const int64_t *call_end, uint64_t n_calls, uint64_t n_names)
{
    g_error[0] = 0;
    return vf_check_calls(call_chrom, call_start, call_end, n_calls, n_names);
}

int h_check_regions(const uint32_t *chrom_id, uint64_t n, uint64_t n_names, uint64_t *n_known)
{
    g_error[0] = 0;
    return vf_check_regions(chrom_id, n, n_names, n_known);
}

uint64_t h_tile_bytes(uint64_t n_bytes) { return vf_tile_bytes(n_bytes); }
uint64_t h_n_tiles(uint64_t n_bytes, uint32_t tile) { return vf_n_tiles(n_bytes, tile); }
uint64_t h_tile_lines(uint32_t tile) { return vf_tile_lines(tile); }
uint64_t h_chunk_cut(const uint8_t *buf, uint64_t n, int at_eof) { return vf_chunk_cut(buf, n, at_eof); }
}

#ifdef KV_HARNESS_MAIN
namespace {
uint64_t g_seed = 20261021;
uint32_t rnd(uint32_t lo, uint32_t hi)          // lo .. hi
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (uint32_t)((g_seed >> 33) % (hi - lo + 1));
}
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int fuzz_numbers()
{
    for (int round = 0; round < 20000; ++round) {
        const int64_t want = (int64_t)((((uint64_t)rnd(0, 0x7FFFFFFFu) << 33) ^ ((uint64_t)rnd(0, 0x7FFFFFFFu) << 2) ^ rnd(0, 3)) >> rnd(1, 63)) * (rnd(0, 1) ? 1 : -1);
        char text[64];
        snprintf(text, sizeof(text), "%s%lld", want >= 0 && rnd(0, 1) ? "+" : "", (long long)want);
        int64_t got = 0;
        CHECK(h_number((const uint8_t *)text, strlen(text), &got) == 1 && got == want);
    }
    int64_t v = 0;
    CHECK(h_number((const uint8_t *)"9223372036854775807", 19, &v) == 1 && v == INT64_MAX);
    CHECK(h_number((const uint8_t *)"-9223372036854775808", 20, &v) == 1 && v == INT64_MIN);
    CHECK(h_number((const uint8_t *)"9223372036854775808", 19, &v) == 0);
    CHECK(h_number((const uint8_t *)"-9223372036854775809", 20, &v) == 0);
    CHECK(h_number((const uint8_t *)"", 0, &v) == 0 && h_number((const uint8_t *)"+", 1, &v) == 0 && h_number((const uint8_t *)"1_000", 5, &v) == 0);
    return 0;
}

int fuzz_tables()
{
    for (int round = 0; round < 200; ++round) {
        const uint32_t n = rnd(0, 3000);
        std::string blob;
        std::vector<uint64_t> off(1, 0);
        for (uint32_t c = 0; c < n; ++c) {
            blob += "chr" + std::to_string(c * 7919u % 100003u) + (rnd(0, 9) ? "" : std::string(rnd(1, 200), 'x'));
            off.push_back(blob.size());
        }
        std::vector<uint32_t> table;
        CHECK(vf_table_build((const uint8_t *)blob.data(), off.data(), n, table) == KV_OK);
        CHECK(table.size() >= 2 * (uint64_t)n + 16 && (table.size() & (table.size() - 1)) == 0);
        for (uint32_t c = 0; c < n; ++c)
            CHECK(vf_table_find(table, (const uint8_t *)blob.data(), off.data(), (const uint8_t *)blob.data() + off[c], off[c + 1] - off[c]) == c);
        CHECK(vf_table_find(table, (const uint8_t *)blob.data(), off.data(), (const uint8_t *)"nowhere", 7) == VF_NO_CHROM);
        if (n) {                                 // the first name once more
            blob += blob.substr(0, off[1]);
            off.push_back(blob.size());
            CHECK(vf_table_build((const uint8_t *)blob.data(), off.data(), n + 1, table) == KV_ERR_ARG);
        }
    }
    return 0;
}

int fuzz_cuts()
{
    for (int round = 0; round < 2000; ++round) {
        std::string buf(rnd(0, 300), 'a');
        for (char &c : buf) c = rnd(0, 20) ? 'a' : '\n';
        const uint64_t cut = vf_chunk_cut((const uint8_t *)buf.data(), buf.size(), 0);
        CHECK(cut <= buf.size() && (cut == 0 || buf[cut - 1] == '\n') && buf.find('\n', cut) == std::string::npos);
        CHECK(vf_chunk_cut((const uint8_t *)buf.data(), buf.size(), 1) == buf.size());
    }
    return 0;
}
}  // namespace

int main()
{
    if (fuzz_numbers() || fuzz_tables() || fuzz_cuts()) return 1;
    printf("varfilter plan fuzz ok\n");
    return 0;
}
#endif
