// Host-side harness for kevlar_amd/csrc/kv_asm_plan.h (compiled as plain C++ by tests/test_assemble_reference.py): the argument
// rules, the sizes and the launch plan of the batched assembly behind a C ABI, so that Python can compare them with a restatement.
// Results come back in caller-provided arrays sized by the caller's own counts.  With -DKV_HARNESS_MAIN the file is a program:
// seeded batches through the same functions with the cover and budget checks done here, for a run under the host sanitizers.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../kevlar_amd/csrc/kv_asm_plan.h"

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
    const uint64_t c[8] = {ASM_MIN_K, ASM_MAX_K, ASM_THREADS, ASM_RUN, ASM_MAX_GRID, ASM_TABLE_LEAST, ASM_MAX_WINDOWS, sizeof(AsmLaunch)};
    memcpy(out, c, sizeof(c));
}

uint64_t h_table_cap(uint64_t n_windows) { return asm_table_cap(n_windows); }
uint64_t h_grid(uint64_t n) { return asm_grid(n); }
uint64_t h_launch_bytes(uint64_t n_windows, uint64_t n_bases, uint64_t n_reads, int ksize) { return asm_launch_bytes(n_windows, n_bases, n_reads, ksize); }
uint64_t h_read_windows(uint64_t len, int ksize) { return asm_read_windows(len, ksize); }
uint64_t h_read_runs(uint64_t len, int ksize) { return asm_read_runs(len, ksize); }

int h_check_args(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize, uint32_t min_count)
{
    g_error[0] = 0;
    return asm_check_args(read_off, n_reads, part_first, n_parts, ksize, min_count);
}

// rows: (part0, part1, read0, read1, n_bases, n_windows, n_runs, table_cap, bytes) per launch, n_parts rows at most
int h_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize, uint64_t mem_budget,
           uint64_t *rows, uint64_t *n_launches)
{
    std::vector<AsmLaunch> launches;
    g_error[0] = 0;
    KV_STEP(asm_check_args(read_off, n_reads, part_first, n_parts, ksize, 1));
    KV_STEP(asm_plan(read_off, n_reads, part_first, n_parts, ksize, mem_budget, launches));
    for (size_t l = 0; l < launches.size(); ++l) {
        const AsmLaunch &a = launches[l];
        const uint64_t row[9] = {a.part0, a.part1, a.read0, a.read1, a.n_bases, a.n_windows, a.n_runs, a.table_cap, a.bytes};
        memcpy(rows + 9 * l, row, sizeof(row));
    }
    *n_launches = launches.size();
    return KV_OK;
}
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

int fuzz_plan()
{
    for (int round = 0; round < 400; ++round) {
        const int ksize = 13 + 2 * (int)rnd(0, 25);
        const uint64_t n_parts = rnd(0, 60);
        std::vector<uint64_t> part_first(1, 0), read_off(1, 0);
        for (uint64_t p = 0; p < n_parts; ++p) {
            const uint32_t reads = rnd(0, 40);
            for (uint32_t r = 0; r < reads; ++r) read_off.push_back(read_off.back() + rnd(0, 300));
            part_first.push_back(read_off.size() - 1);
        }
        const uint64_t n_reads = read_off.size() - 1;
        CHECK(asm_check_args(read_off.data(), n_reads, part_first.data(), n_parts, ksize, 1) == KV_OK);
        uint64_t biggest = 0, all_windows = 0;
        for (uint64_t p = 0; p < n_parts; ++p) {
            uint64_t win = 0;
            for (uint64_t r = part_first[p]; r < part_first[p + 1]; ++r) win += asm_read_windows(read_off[r + 1] - read_off[r], ksize);
            all_windows += win;
            biggest = std::max(biggest, asm_launch_bytes(win, read_off[part_first[p + 1]] - read_off[part_first[p]], part_first[p + 1] - part_first[p], ksize));
        }
        const uint64_t everything = asm_launch_bytes(all_windows, read_off[n_reads], n_reads, ksize);
        const uint64_t budget = biggest + (uint64_t)((double)(everything - std::min(everything, biggest)) * rnd(0, 100) / 100.0);
        std::vector<AsmLaunch> launches;
        CHECK(asm_plan(read_off.data(), n_reads, part_first.data(), n_parts, ksize, budget, launches) == KV_OK);
        uint64_t at = 0, windows = 0;
        for (const AsmLaunch &l : launches) {       // the launches cover the partitions in order, each inside the budget
            CHECK(l.part0 == at && l.part1 > l.part0 && l.read0 == part_first[l.part0] && l.read1 == part_first[l.part1]);
            CHECK(l.bytes <= budget && l.bytes == asm_launch_bytes(l.n_windows, l.n_bases, l.read1 - l.read0, ksize));
            CHECK(l.table_cap >= 2 * l.n_windows + 16 && (l.table_cap & (l.table_cap - 1)) == 0);
            CHECK(l.n_bases == read_off[l.read1] - read_off[l.read0] && l.n_runs * ASM_RUN >= l.n_windows);
            at = l.part1;
            windows += l.n_windows;
        }
        CHECK(at == n_parts && windows == all_windows);
        if (n_parts && biggest) CHECK(asm_plan(read_off.data(), n_reads, part_first.data(), n_parts, ksize, biggest - 1, launches) == KV_ERR_CAPACITY);
    }
    return 0;
}
}  // namespace

int main()
{
    if (fuzz_plan()) return 1;
    printf("assembly plan fuzz ok\n");
    return 0;
}
#endif
