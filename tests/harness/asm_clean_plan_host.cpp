// Host-side harness for the cleaning-aware half of kevlar_amd/csrc/kv_asm_plan.h (compiled as plain C++ by
// tests/test_asmclean_reference.py, beside asm_plan_host.cpp): the bytes of a launch that cleans, the argument rule of the
// cleaning settings and the launch plan under those bytes, behind a C ABI, so that Python can compare them with the restatement in
// tests/asmclean_common.py.  Results come back in caller-provided arrays sized by the caller's own counts.
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
const char *hc_last_error() { return g_error; }

void hc_constants(uint64_t *out)
{
    const uint64_t c[2] = {ASM_CLEAN_BYTES_PER_WINDOW, ASM_DEFAULT_CLEAN_ROUNDS};
    memcpy(out, c, sizeof(c));
}

uint64_t hc_launch_bytes(uint64_t n_windows, uint64_t n_bases, uint64_t n_reads, int ksize, uint32_t tip_nodes, uint32_t bubble_nodes)
{
    return asm_launch_bytes(n_windows, n_bases, n_reads, ksize, asm_cleaning(tip_nodes, bubble_nodes));
}

int hc_check_clean(uint32_t tip_nodes, uint32_t bubble_nodes, uint32_t clean_rounds)
{
    g_error[0] = 0;
    return asm_check_clean(tip_nodes, bubble_nodes, clean_rounds);
}

// rows: (part0, part1, read0, read1, n_bases, n_windows, n_runs, table_cap, bytes) per launch, n_parts rows at most
int hc_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize, uint64_t mem_budget,
            uint32_t tip_nodes, uint32_t bubble_nodes, uint32_t clean_rounds, uint64_t *rows, uint64_t *n_launches)
{
    std::vector<AsmLaunch> launches;
    g_error[0] = 0;
    KV_STEP(asm_check_args(read_off, n_reads, part_first, n_parts, ksize, 1));
    KV_STEP(asm_check_clean(tip_nodes, bubble_nodes, clean_rounds));
    KV_STEP(asm_plan(read_off, n_reads, part_first, n_parts, ksize, mem_budget, launches, asm_cleaning(tip_nodes, bubble_nodes)));
    for (size_t l = 0; l < launches.size(); ++l) {
        const AsmLaunch &a = launches[l];
        const uint64_t row[9] = {a.part0, a.part1, a.read0, a.read1, a.n_bases, a.n_windows, a.n_runs, a.table_cap, a.bytes};
        memcpy(rows + 9 * l, row, sizeof(row));
    }
    *n_launches = launches.size();
    return KV_OK;
}
}
