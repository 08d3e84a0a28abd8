// kv_asm_plan.h -- the host rules of the batched assembly (kv_assemble.hip), free of HIP: what a batch of partitions must satisfy,
// how many windows, runs and table slots it has, the launch grids, and where a call is cut into launches under a memory budget
// (with the bytes of the cleaning rounds when a call cleans: tests/harness/asm_clean_plan_host.cpp).
// A launch holds whole partitions: a K-mer of one partition says nothing about the same K-mer of another, so nothing crosses a
// cut.  Plain C++17: tests/harness/asm_plan_host.cpp compiles it for the host, tests/test_assemble_reference.py checks the edges.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/kvsketch.h"
#include "kv_require.h"

#define ASM_MIN_K 13
#define ASM_MAX_K 63
#define ASM_THREADS 256
#define ASM_RUN 32                          // consecutive windows of one read a lane rolls its keys over
#define ASM_MAX_GRID 4096
#define ASM_TABLE_LEAST 1024
#define ASM_MAX_WINDOWS 0x3FFFFFF0ull       // per launch: window ids and 2 * id + strand are 32-bit
#define ASM_BYTES_PER_WINDOW(W) (8ull * (W) + 16ull)   // key; owner, partition, count, degree mask + flags
#define ASM_BYTES_PER_CHUNK 12ull                      // per ASM_THREADS windows: heads, heads in front
#define ASM_CLEAN_BYTES_PER_WINDOW 12ull               // cleaning (rules 3a-3c): head index of either strand, liveness
#define ASM_DEFAULT_CLEAN_ROUNDS 8

struct AsmLaunch {
    uint64_t part0, part1;                  // partitions [part0, part1)
    uint64_t read0, read1;                  // their reads
    uint64_t n_bases, n_windows, n_runs;    // bases from read_off[read0]; windows of K valid-or-not bases; runs of <= ASM_RUN windows
    uint64_t table_cap;                     // slots of the key table, a power of two
    uint64_t bytes;                         // device memory of the launch in front of the walk (heads and output follow the counts)
};

static inline uint64_t asm_words(int ksize) { return ksize <= 31 ? 1 : 2; }
static inline uint64_t asm_read_windows(uint64_t len, int ksize) { return len >= (uint64_t)ksize ? len - (uint64_t)ksize + 1 : 0; }
static inline uint64_t asm_chunks(uint64_t n_windows) { return (n_windows + ASM_THREADS - 1) / ASM_THREADS; }
static inline uint64_t asm_read_runs(uint64_t len, int ksize) { return (asm_read_windows(len, ksize) + ASM_RUN - 1) / ASM_RUN; }
// at most half full: a probe ends at an empty slot
static inline uint64_t asm_table_cap(uint64_t n_windows)
{
    uint64_t c = ASM_TABLE_LEAST;
    while (c < 2 * n_windows + 16) c <<= 1;
    return c;
}
static inline unsigned asm_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + ASM_THREADS - 1) / ASM_THREADS, ASM_MAX_GRID)); }
static inline uint64_t asm_launch_bytes(uint64_t n_windows, uint64_t n_bases, uint64_t n_reads, int ksize, bool cleaning = false)
{
    return n_windows * (ASM_BYTES_PER_WINDOW(asm_words(ksize)) + (cleaning ? ASM_CLEAN_BYTES_PER_WINDOW : 0)) +
           (asm_chunks(n_windows) + 1) * ASM_BYTES_PER_CHUNK + 8 * asm_table_cap(n_windows) + n_bases + 32 * (n_reads + 1);
}
// limits 0, 0 mean no cleaning, and then the number of rounds says nothing
static inline bool asm_cleaning(uint32_t tip_nodes, uint32_t bubble_nodes) { return tip_nodes != 0 || bubble_nodes != 0; }
static inline int asm_check_clean(uint32_t tip_nodes, uint32_t bubble_nodes, uint32_t clean_rounds)
{
    KV_REQUIRE(!asm_cleaning(tip_nodes, bubble_nodes) || clean_rounds >= 1, KV_ERR_ARG,
               "kv_assemble_clean_batch: clean_rounds must be at least 1 (tip_nodes %u, bubble_nodes %u)", tip_nodes, bubble_nodes);
    return KV_OK;
}

static inline int asm_check_args(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                                 uint32_t min_count)
{
    KV_REQUIRE(read_off && part_first, KV_ERR_ARG, "kv_assemble_batch: null argument");
    KV_REQUIRE(ksize >= ASM_MIN_K && ksize <= ASM_MAX_K && (ksize & 1), KV_ERR_ARG, "kv_assemble_batch: K must be odd and %d..%d (got %d)",
               ASM_MIN_K, ASM_MAX_K, ksize);
    KV_REQUIRE(min_count >= 1, KV_ERR_ARG, "kv_assemble_batch: min_count must be at least 1");
    KV_REQUIRE(n_parts < 0xFFFFFFF0ull, KV_ERR_ARG, "kv_assemble_batch: %llu partitions in one call", (unsigned long long)n_parts);
    for (uint64_t r = 0; r < n_reads; ++r)
        KV_REQUIRE(read_off[r] <= read_off[r + 1], KV_ERR_ARG, "kv_assemble_batch: read offsets must not decrease");
    KV_REQUIRE(part_first[0] == 0 && part_first[n_parts] == n_reads, KV_ERR_ARG,
               "kv_assemble_batch: the partitions must cover reads 0..%llu", (unsigned long long)n_reads);
    for (uint64_t p = 0; p < n_parts; ++p)
        KV_REQUIRE(part_first[p] <= part_first[p + 1], KV_ERR_ARG, "kv_assemble_batch: partition bounds must not decrease");
    return KV_OK;
}

// a launch takes partitions until the next one would pass the budget; a partition that alone passes it is refused
static inline int asm_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                           uint64_t mem_budget, std::vector<AsmLaunch> &launches, bool cleaning = false)
{
    launches.clear();
    AsmLaunch cur = AsmLaunch();
    for (uint64_t p = 0; p < n_parts; ++p) {
        uint64_t win = 0, runs = 0;
        for (uint64_t r = part_first[p]; r < part_first[p + 1]; ++r) {
            win += asm_read_windows(read_off[r + 1] - read_off[r], ksize);
            runs += asm_read_runs(read_off[r + 1] - read_off[r], ksize);
        }
        const uint64_t bases = read_off[part_first[p + 1]] - read_off[part_first[p]], reads = part_first[p + 1] - part_first[p];
        const uint64_t alone = asm_launch_bytes(win, bases, reads, ksize, cleaning);
        KV_REQUIRE(alone <= mem_budget && win <= ASM_MAX_WINDOWS, KV_ERR_CAPACITY,
                   "partition %llu (%llu reads, %llu windows) needs %llu bytes, the budget is %llu", (unsigned long long)p,
                   (unsigned long long)reads, (unsigned long long)win, (unsigned long long)alone, (unsigned long long)mem_budget);
        const bool open = cur.part1 > cur.part0;
        if (open && (asm_launch_bytes(cur.n_windows + win, cur.n_bases + bases, cur.read1 - cur.read0 + reads, ksize, cleaning) > mem_budget ||
                     cur.n_windows + win > ASM_MAX_WINDOWS)) {
            launches.push_back(cur);
            cur = AsmLaunch();
        }
        if (cur.part1 == cur.part0) { cur.part0 = p; cur.read0 = part_first[p]; }
        cur.part1 = p + 1;
        cur.read1 = part_first[p + 1];
        cur.n_bases += bases; cur.n_windows += win; cur.n_runs += runs;
    }
    if (cur.part1 > cur.part0) launches.push_back(cur);
    for (AsmLaunch &l : launches) {
        l.table_cap = asm_table_cap(l.n_windows);
        l.bytes = asm_launch_bytes(l.n_windows, l.n_bases, l.read1 - l.read0, ksize, cleaning);
    }
    return KV_OK;
}
