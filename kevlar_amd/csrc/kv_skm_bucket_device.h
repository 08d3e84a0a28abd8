// kv_skm_bucket_device.h -- device half of kv_skm.hip, the kernels that work on fine buckets: the LDS combining table, the balanced
// walk over a bucket's k-mer occurrences, S3 (k_skm_count), S3' (k_skm_route), S6 (k_skm_novel, k_skm_novel_list), the owner's scan
// (k_skm_set_hits), the loose-list kernel of each, and the small kernels around the scan.  Included by kv_skm.hip only, after
// kv_skm_emit_device.h (SkmGeom, the record stores).
#pragma once
#include "kv_skm_emit_device.h"

// the controls' abundance lists a scan may use (same bucket geometry as the case sample's buckets)
#define SKM_MAX_ABL 8
struct SkmAblSet {
    int n, ctrl_max;
    const uint64_t *keys[SKM_MAX_ABL];
    const uint8_t *cnts[SKM_MAX_ABL];
    const uint32_t *bstart[SKM_MAX_ABL], *bcount[SKM_MAX_ABL];
    uint32_t maxv[SKM_MAX_ABL];      // what a counter of that control can hold: an entry rejects if min(count, maxv) > ctrl_max
};

namespace {

#define SKM_THREADS3 512
// buckets per ticket of the bucket kernels' work counter (SKM_TILES_PER_TICKET in kv_skm_emit_device.h says why a ticket covers several)
#define SKM_BUCKETS_PER_TICKET 8u
#define SKM_MAXPROBE 48
// workgroups of the loose-list kernels (grid-stride over a list that is all but empty when the batch fits: 4096 workgroups cost
// 0.14 ms each launch just to start, find nothing and leave)
#define SKM_LOOSE_WGS 1024

// ---- LDS combining table -------------------------------------------------------------------------------
// the step from a slot to the next one tried: an odd number taken from the key's hash (double hashing: two keys that meet in one slot
// part ways at once, no clusters -- the wave waits for the lane with the longest chain)
// (k_skm_count 3.23 -> 3.04 ms per sample of config 2 against linear probing, a step of 1)
#define SKM_STEP_MASK 62u
#define SKM_PROBE_STEP(h) ((((h) >> 20) & SKM_STEP_MASK) | 1u)
// slot a hash starts at / the slot `step` further on, for tables of 2^n slots and of any other size (3072: the count's instances that
// share their LDS with a table of records) -- there the top bits of the hash pick the slot, so the step comes from the low ones
template <int TS>
__device__ __forceinline__ uint32_t skm_slot0(uint32_t sh) { return (TS & (TS - 1)) == 0 ? sh & (uint32_t)(TS - 1) : __umulhi(sh, (uint32_t)TS); }
template <int TS>
__device__ __forceinline__ uint32_t skm_step_of(uint32_t sh) { return (TS & (TS - 1)) == 0 ? SKM_PROBE_STEP(sh) : (((sh >> 2) & 62u) | 1u); }
template <int TS>
__device__ __forceinline__ uint32_t skm_slot_next(uint32_t slot, uint32_t step)
{
    if ((TS & (TS - 1)) == 0) return (slot + step) & (uint32_t)(TS - 1);
    slot += step;
    return slot >= (uint32_t)TS ? slot - (uint32_t)TS : slot;
}
template <int KW, int TS>
struct SkmTable {
    unsigned long long key[KW][TS];
};

template <int KW, int TS>
__device__ __forceinline__ void skm_table_clear(SkmTable<KW, TS> &tb)
{
    for (uint32_t i = threadIdx.x; i < TS; i += blockDim.x) {
        tb.key[0][i] = SKM_EMPTY;
        if (KW == 2) tb.key[KW - 1][i] = SKM_EMPTY;
    }
}

// slot of the key, claiming a free slot if it is new; -1 when SKM_MAXPROBE slots are all taken by other keys.  With
// two key words a slot is identified word by word: whoever sets word 0 (or finds it equal) goes on to set or
// compare word 1, and moves to the next slot if another k-mer with the same first 32 bases got there first.
template <int KW, int TS>
__device__ __forceinline__ int skm_table_insert(SkmTable<KW, TS> &tb, const SkmKey<KW> &c)
{
    const uint32_t sh = skm_slot_hash<KW>(c);
    uint32_t slot = skm_slot0<TS>(sh);
    const uint32_t step = skm_step_of<TS>(sh);
    for (int probe = 0; probe < SKM_MAXPROBE; ++probe) {
        // (reading the slot first and swapping only into an empty one was measured 5 % slower: the read does not save
        // the swap's round trip, it adds one for every new key)
        const unsigned long long old0 = atomicCAS(&tb.key[0][slot], SKM_EMPTY, (unsigned long long)c.w[0]);
        if (old0 == SKM_EMPTY || old0 == c.w[0]) {
            if (KW == 1) return (int)slot;
            const unsigned long long old1 = atomicCAS(&tb.key[KW - 1][slot], SKM_EMPTY, (unsigned long long)c.w[KW - 1]);
            if (old1 == SKM_EMPTY || old1 == c.w[KW - 1]) return (int)slot;
        }
        slot = skm_slot_next<TS>(slot, step);
    }
    return -1;
}

template <int KW, int TS>
__device__ __forceinline__ int skm_table_find(const SkmTable<KW, TS> &tb, const SkmKey<KW> &c)
{
    const uint32_t sh = skm_slot_hash<KW>(c);
    uint32_t slot = skm_slot0<TS>(sh);
    const uint32_t step = skm_step_of<TS>(sh);
    for (int probe = 0; probe < SKM_MAXPROBE; ++probe) {
        const unsigned long long k0 = tb.key[0][slot];
        if (k0 == SKM_EMPTY) return -1;
        if (k0 == c.w[0] && (KW == 1 || tb.key[KW - 1][slot] == c.w[KW - 1])) return (int)slot;
        slot = skm_slot_next<TS>(slot, step);
    }
    return -1;
}

// the key in table slot `slot` / the same, and the slot emptied (a drain that reads the table empties it as it goes)
template <int KW, int TS>
__device__ __forceinline__ SkmKey<KW> skm_table_key(const SkmTable<KW, TS> &tb, uint32_t slot)
{
    SkmKey<KW> c;
    c.w[0] = tb.key[0][slot];
    if (KW == 2) c.w[KW - 1] = tb.key[KW - 1][slot];
    return c;
}
template <int KW, int TS>
__device__ __forceinline__ SkmKey<KW> skm_table_take(SkmTable<KW, TS> &tb, uint32_t slot)
{
    const SkmKey<KW> c = skm_table_key(tb, slot);
    tb.key[0][slot] = SKM_EMPTY;
    if (KW == 2) tb.key[KW - 1][slot] = SKM_EMPTY;
    return c;
}

// entry e of an array of keys (KW words each: the distinct list, an abundance list); !live: the empty key, nothing is read
template <int KW>
__device__ __forceinline__ SkmKey<KW> skm_key_load(const uint64_t *keys, uint64_t e, bool live = true)
{
    SkmKey<KW> c;
    c.w[0] = live ? keys[e * KW] : SKM_EMPTY;
    if (KW == 2) c.w[KW - 1] = live ? keys[e * KW + (KW - 1)] : SKM_EMPTY;
    return c;
}
template <int KW>
__device__ __forceinline__ void skm_key_store(uint64_t *keys, uint64_t e, const SkmKey<KW> &c)
{
    keys[e * KW] = c.w[0];
    if (KW == 2) keys[e * KW + (KW - 1)] = c.w[KW - 1];
}

// A place behind an LDS cursor for every lane of the wave that wants one (the lanes that are in here vote): one atomic per wave.
// The place of a lane that wants none means nothing.
__device__ __forceinline__ uint32_t skm_wave_reserve(uint32_t *cursor, bool want)
{
    const unsigned long long here = __ballot(true), vote = __ballot(want);
    if (!vote) return 0u;
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)here) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(vote));
    base = (uint32_t)__shfl((int)base, (int)leader);
    return base + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
}

// distinct list: key and hash of a drained k-mer behind the workgroup's cursor, if it lies within the `lim` entries from `org` on
// (by reference: k_skm_route keeps the two in LDS and reads them behind the atomic, each where it is used, as its hand-written site
// did -- fetched ahead of the call they stay live across it: 16 bytes of scratch per lane more in k_skm_route<1, 4096>)
template <int KW, typename Org>
__device__ __forceinline__ void skm_dl_push(const SkmGeom &sg, uint32_t *dl_cur, const Org &org, const uint32_t &lim, const SkmKey<KW> &c, uint64_t h)
{
    const uint32_t at = skm_wave_reserve(dl_cur, true);
    if (at < lim) {
        const uint64_t e = (uint64_t)org + at;
        skm_key_store<KW>(sg.dl_keys, e, c);
        sg.dl_hash[e] = h;
    }
}

// count side of one distinct k-mer seen `count` times: filter, then T weighted items through `emit(table, bin, weight)`
template <typename Emit>
__device__ __forceinline__ uint32_t skm_count_kmer(uint64_t h, uint32_t count, const SketchDev *__restrict__ sk,
                                                   const SketchDev *__restrict__ mask, const ConsumeFilter &f, int T, Emit emit)
{
    if (!consume_filter_pass(f, mask, h)) return 0;
    uint32_t left = min(count, 255u);                  // no counter holds more than 255
    // (tried: lane l starting with table l mod 4, so that one emit instruction spreads over the cursors of all tables instead
    // of 64 lanes sharing the ~20 cursors of one -- 3.6 -> 4.2 ms: what costs is the number of distinct segments, i.e. cache
    // lines, one store instruction touches, not the same-address LDS atomics; more coarse buckets cost the same way)
    while (left) {
        const uint32_t wgt = min(left, BIN_W_MAX);
#pragma unroll
        for (int t = 0; t < BIN_MAX_T; ++t)
            if (t < T) emit(t, fastmod(h, sk->size[t], sk->magic[t]), wgt);
        left -= wgt;
    }
    return count;
}

// every wave walks its share of the table and hands the occupied slots to `body` 64 at a time (all lanes busy):
// occupied slots are queued in LDS and drained whenever a full wave of them is ready
template <int TS, typename Body>
__device__ __forceinline__ void skm_for_occupied(const unsigned long long *key0, uint16_t *queue_all, uint32_t queue_stride, Body body, const uint32_t *skip = nullptr)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    uint16_t *queue = queue_all + wave * queue_stride;               // >= 128 entries; wave-private, ordered by the fences below
    const uint32_t per_wave = TS / nwaves;
    const uint32_t s_end = (wave + 1) * per_wave;
    uint32_t qn = 0;                                    // < 64 between iterations
    for (uint32_t s0 = wave * per_wave;; s0 += 64) {
        const bool last = s0 >= s_end;
        if (!last) {
            const uint32_t slot = s0 + lane;
            const bool occ = key0[slot] != SKM_EMPTY && !(skip && ((skip[slot >> 5] >> (slot & 31u)) & 1u));      // skip: a bit per slot
            const unsigned long long ballot = __ballot(occ);
            if (occ) __hip_atomic_store(&queue[qn + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))], (uint16_t)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            qn += (uint32_t)__popcll(ballot);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (qn >= 64 || (last && qn > 0)) {
            const uint32_t take = min(qn, 64u);
            qn -= take;
            if (lane < take) body((uint32_t)__hip_atomic_load(&queue[qn + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (last) break;
    }
}

// ---- balanced walk over the k-mer occurrences of a fine bucket ------------------------------------------------
// Records hold 1..ncap k-mers, so a thread per record would leave most lanes waiting for the longest one, and a
// thread per occurrence cuts every k-mer out of its record from scratch (round 2: 115 VALU instructions per
// occurrence, the largest item of the count kernel).  The walk therefore deals UNITS: SKM_UNIT consecutive k-mers
// of one record.  Each wave takes 64 records (one per lane, in registers), numbers their units with a prefix sum and
// walks them 64 at a time: lane p of block t0 handles unit t0 + p, finds the record that owns it from a bit mask of
// record starts (one LDS word pair per block, popcounts), fetches that record's words from the owning lane with
// ds_bpermute, cuts the unit's first k-mer out, takes its reverse complement once and ROLLS both strands through
// the unit's other k-mers (two shifts each).  Records average ~9 k-mers: units of 4 are 85 % full.
#define SKM_UNIT 4

__device__ __forceinline__ uint64_t skm_shfl64(uint64_t v, uint32_t src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// occurrences that found no room in the LDS table leave as one-k-mer records (either strand of the k-mer): one atomic per wave
template <int KW, bool WANT_POS>
__device__ __forceinline__ void skm_walk_loose(const SkmGeom &sg, bool alone, const SkmKey<KW> &kmer, uint64_t hdr, uint32_t owner,
                                               uint64_t pos0, uint32_t j0, uint32_t u, uint32_t lane, int recw)
{
    const unsigned long long need = __ballot(alone);
    if (!need) return;
    // (the count pass does not fetch the records' headers for the walk; here -- a wave in a few hundred -- it does,
    // so that the loose record carries the occurrence's real position: a scan that goes by the count pass's
    // distinct list evaluates these records as they are)
    // (WANT_POS: pos0 is this occurrence's position already; else it is derived here from the owner's header, orientation included)
    const uint64_t posu = WANT_POS ? pos0 : skm_hdr_pos_of(skm_shfl64(hdr, owner), j0 + u);
    unsigned long long first = 0;
    if (lane == 0) first = atomicAdd(&sg.ctr[SKM_CTR_LOOSE], (unsigned long long)__popcll(need));
    first = skm_shfl64(first, 0);
    if (alone) {
        const unsigned long long idx = first + (unsigned long long)__popcll(need & ((1ull << lane) - 1ull));
        uint64_t one[3] = {kmer.w[0], KW == 2 ? kmer.w[KW - 1] : 0ull, 0ull};
        if (idx < sg.loose_cap) skm_store_record(sg.loose + idx * (uint64_t)recw, skm_header(posu, 1u, 0u), one, sg.nbw);
        else sg.ctr[SKM_CTR_FAIL] = 1;
    }
}

// body(k-mer, position of the occurrence) -> true if the occurrence could not be combined and must travel alone through the
// loose list; WANT_POS = false skips fetching the header (count pass).  The records are oriented: a k-mer's key is the k-mer as
// the record holds it.
template <int KW, bool WANT_POS, int FK = 0, bool COMPACT = false, typename Body>
__device__ __forceinline__ void skm_walk_bucket(const SkmGeom &sg, uint32_t b, uint32_t *sbits_all, Body body)
{
    static_assert(!COMPACT || (KW == 1 && !WANT_POS), "compact records: one-word keys, no positions");
    constexpr uint32_t G = SKM_UNIT;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint32_t *sbits = sbits_all + wave * sg.sbw;       // sbw words: 64 records x ncap k-mers (units need fewer), + the word a 64-bit read may straddle into
    const int k = FK ? FK : sg.k, recw = COMPACT ? 2 : (FK ? 1 + KW + 1 : sg.recw);        // FK: k (and with it the record width) known when compiled
    // a compact record (16 bytes, one load) is taken apart into what the code below knows: a header without a position, two base words
    auto load = [&](const uint64_t *rec, uint64_t &hdr, uint64_t &b0, uint64_t &b1, uint64_t &b2) {
        if (COMPACT) {
            typedef uint64_t u64x2a __attribute__((ext_vector_type(2), aligned(16)));
            const u64x2a both = *(const u64x2a *)rec;
            b0 = both.x; b1 = skm_c_b1(both.y); hdr = skm_header(0ull, skm_c_n(both.y), 0u, skm_c_rev(both.y));
        } else {
            hdr = rec[0]; b0 = rec[1]; b1 = rec[2];
            if (KW == 2) b2 = rec[3];
        }
    };
    // Which records a wave takes does not depend on how full the bucket's segments are: pair p = wave, wave + nwaves, ...
    // is records [64 g, 64 g + 64) of segment s = p mod nwg2, g = p / nwg2.  The records are therefore requested together
    // with the segment counts (which only mask them afterwards) instead of behind them, and the same addresses of the
    const uint32_t *cnt2 = sg.cnt2 + (uint64_t)b * sg.nwg2;
    uint32_t p = wave;
    uint32_t g = p / sg.nwg2, sgm = p - g * sg.nwg2;
    uint64_t hdr = 0, b0 = 0, b1 = 0, b2 = 0;
    {
        const uint32_t at = min(g * 64u + lane, sg.cap2 - 1u);
        const uint64_t *rec = sg.seg2 + (((uint64_t)b * sg.nwg2 + sgm) * sg.cap2 + at) * (uint64_t)recw;
        load(rec, hdr, b0, b1, b2);
    }
    uint32_t maxc = 0;
    for (uint32_t s2 = 0; s2 < sg.nwg2; ++s2) maxc = max(maxc, cnt2[s2]);
    for (;;) {
        if (g * 64u >= maxc) break;
        const uint32_t NR = cnt2[sgm], i = g * 64u + lane;      // (the name the code below knows the bound by)
        const uint32_t nk = i < NR ? skm_hdr_n(hdr) : 0u;
        const uint32_t nu = (nk + G - 1u) / G;          // units of this record
        uint32_t incl = nu;                             // (wave_incl_scan of kv_scan_device.h written out: through the helper this kernel did not compile to the same code)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63), excl = incl - nu;
        const uint32_t exnk = excl | (nk << 16);        // < 64 * ncap units: 16 bits are plenty
        const uint32_t nwords = (total >> 5) + 2u;
        for (uint32_t wd = lane; wd < nwords; wd += 64) sbits[wd] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (nu) atomicOr(&sbits[excl >> 5], 1u << (excl & 31));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t before = 0;                            // records that start in front of this block
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {
            // (relaxed wave-scope loads: a volatile access through the generic pointer became a system-scope FLAT load
            // with its own s_waitcnt vmcnt(0), two in a row per block)
            const uint64_t starts = (uint64_t)__hip_atomic_load(&sbits[t0 >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) |
                                    ((uint64_t)__hip_atomic_load(&sbits[(t0 >> 5) + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) << 32);
            const uint32_t t = t0 + lane;
            const uint32_t owner = (before + (uint32_t)__popcll(starts & ((2ull << lane) - 1ull)) - 1u) & 63u;
            before += (uint32_t)__popcll(starts);
            const uint32_t oe = (uint32_t)__shfl((int)exnk, (int)owner);
            const uint64_t o0 = skm_shfl64(b0, owner), o1 = skm_shfl64(b1, owner);
            const uint64_t o2 = KW == 2 ? skm_shfl64(b2, owner) : 0ull;
            const uint64_t oh = WANT_POS ? skm_shfl64(hdr, owner) : 0ull;
            const uint32_t j0 = t < total ? (t - (oe & 0xffffu)) * G : 0u;
            const uint32_t cnt = t < total ? min(G, (oe >> 16) - j0) : 0u;     // k-mers of this unit: 1..G (0: no unit)
            SkmKey<KW> fw = skm_kmer_of<KW>(o0, o1, o2, j0, k);
            const uint32_t tail = (uint32_t)skm_window64(o0, o1, o2, j0 + (uint32_t)k);   // the bases that enter k-mers 1 .. G - 1
            // read position of the unit's first k-mer and the step to the next: a reversed record's k-mer j stands at pos + n - 1 - j
            uint64_t pos0 = 0;
            int step = 1;
            if (WANT_POS) {
                const bool rv = skm_hdr_rev(oh) != 0u;
                pos0 = skm_hdr_pos(oh) + (rv ? skm_hdr_n(oh) - 1u - j0 : j0);
                step = rv ? -1 : 1;
            }
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) {
                if (u) { SkmKey<KW> other = fw; skm_roll<KW>(fw, other, (tail >> (2u * (u - 1u))) & 3u, k); }      // (the other strand is dead code here)
                const uint64_t posu = pos0 + (uint64_t)(int64_t)(step * (int)u);
                bool alone = false;
                if (u < cnt) alone = body(fw, posu);
                skm_walk_loose<KW, WANT_POS>(sg, alone, fw, hdr, owner, posu, j0, u, lane, sg.lrecw);
            }
        }
        __builtin_amdgcn_wave_barrier();                // the next group clears the mask
        p += nwaves;
        g = p / sg.nwg2; sgm = p - g * sg.nwg2;
        if (g * 64u >= maxc) break;
        if (g * 64u + lane < cnt2[sgm]) {
            const uint64_t *rec = sg.seg2 + (((uint64_t)b * sg.nwg2 + sgm) * sg.cap2 + g * 64u + lane) * (uint64_t)recw;
            load(rec, hdr, b0, b1, b2);
        }
    }
}

// ---- what the bucket kernels share besides the walk: work tickets, the loose list ---------------------------------------
// Persistent workgroups draw buckets from one device-wide counter, sg.bpt consecutive buckets per ticket (SKM_BUCKETS_PER_TICKET):
// the first one before the loop, the next one while the current bucket is processed.
template <int CTR>
__device__ __forceinline__ uint32_t skm_first_bucket(const SkmGeom &sg) { return (uint32_t)atomicAdd(&sg.ctr[CTR], 1ull) * sg.bpt; }

// Thread 0, once everybody has read bucket b out of `next`: the bucket after b, 0xffffffff when the workgroup has taken its quota3.
// CTR: SKM_CTR_TICKET_COUNT or SKM_CTR_TICKET_SCAN.  FAIL_ENDS: a raised SKM_CTR_FAIL ends the pass at the next ticket (the caller
// redoes the batch).  ESTIMATE: the early exit -- a batch that does not fit the LDS tables (low coverage per batch: nearly every
// k-mer distinct) is given up early: once 2 % of the buckets are done, more than 4 % of their k-mers outside the tables raise the
// flag.  The count pass runs it, and the scan that cut the batch itself (k_skm_novel): its caller then scans tile by tile, and
// remembers, instead of pushing the whole batch through the loose list.
template <int CTR, bool FAIL_ENDS, bool ESTIMATE>
__device__ __forceinline__ void skm_next_bucket(const SkmGeom &sg, uint32_t b, uint32_t taken, uint32_t &next)
{
    if ((b + 1u) & (sg.bpt - 1u)) next = b + 1u;       // same ticket
    else if (taken + 1 >= sg.quota3 || (FAIL_ENDS && __hip_atomic_load(&sg.ctr[SKM_CTR_FAIL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) next = 0xffffffffu;
    else {
        const unsigned long long ticket = atomicAdd(&sg.ctr[CTR], 1ull);
        next = (uint32_t)ticket * sg.bpt;
        if (ESTIMATE) {
            const unsigned long long done = ticket * sg.bpt;
            if (done * 50ull >= sg.n_buckets) {
                const unsigned long long now = __hip_atomic_load(&sg.ctr[SKM_CTR_LOOSE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), start = sg.ctr[SKM_CTR_LOOSE_S12];
                if (now > start && (now - start) * 25ull > done * sg.bucket_kmers) sg.ctr[SKM_CTR_FAIL] = 1;
            }
        }
    }
}

// records on the loose list (those beyond its room were lost: skm_loose_push has raised SKM_CTR_FAIL)
__device__ __forceinline__ uint64_t skm_loose_len(const SkmGeom &sg)
{
    const unsigned long long n = sg.ctr[SKM_CTR_LOOSE];
    return n > sg.loose_cap ? sg.loose_cap : n;
}

// The loose list dealt to waves: body(k-mer as the record holds it, live, header of its record, index of the k-mer in the record),
// called by all lanes of a wave together (a body may vote: spill_items_wave) -- `live` says whether the lane has a k-mer.
// A wave takes up to 64 records at a time: the one-k-mer records (occurrences that missed a full LDS table: nearly all of them) are
// handled one per lane; a record with several k-mers (it missed its segment in S1 / S2) is spread over the lanes, one k-mer each,
// instead of holding 63 lanes up while one lane rolls through it (a thread per record rolled through up to ncap k-mers, each a chain
// of table probes: 0.167 ms for the handful of records a config-2 scan finds here).
// (k_skm_loose_route and k_skm_loose_set_hits go through the list with a thread per record instead, and their two loops stay written
// out: see k_skm_loose_route.)
template <int KW, typename Body>
__device__ __forceinline__ void skm_loose_walk_wave(const SkmGeom &sg, Body body)
{
    const unsigned long long n = skm_loose_len(sg);      // (here, not handed in by the kernel: that cost the four instances two VGPRs each)
    const int k = sg.k;
    const uint32_t lane = threadIdx.x & 63u;
    // records a wave takes at a time: the records with several k-mers are handled one after the other (in the count each a round trip
    // to the spill counter), so a short list -- 40 k records at config 2 -- is dealt a few records to every wave, not 64 to one wave in
    // seven (k_skm_loose_count 0.135 -> 0.0x ms per launch; a long list -- k = 51: millions of one-k-mer records -- keeps 64)
    const uint64_t total_waves = (uint64_t)gridDim.x * (blockDim.x >> 6), wave_id = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t per = (uint32_t)min((unsigned long long)64, max((unsigned long long)1, (n + total_waves - 1) / total_waves));
    for (uint64_t i0 = wave_id * per; i0 < n; i0 += total_waves * per) {
        const uint64_t i = i0 + lane;
        const bool have = lane < per && i < n;
        const uint64_t *rec = sg.loose + (have ? i : 0) * (uint64_t)sg.lrecw;
        uint64_t bw[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bw[t] = (have && t < sg.nbw) ? rec[1 + t] : 0ull;
        const uint64_t hdr = have ? rec[0] : 0ull;
        const uint32_t nk = skm_hdr_n(hdr);
        body(skm_first_kmer<KW>(bw, k), nk == 1, hdr, 0u);
        unsigned long long longer = __ballot(nk > 1);
        while (longer) {
            const uint32_t src = (uint32_t)__ffsll((long long)longer) - 1u;
            longer &= longer - 1ull;
            const uint64_t b0 = skm_shfl64(bw[0], src), b1 = skm_shfl64(bw[1], src), b2 = skm_shfl64(bw[2], src), h_src = skm_shfl64(hdr, src);
            const uint32_t nk_src = (uint32_t)__shfl((int)nk, (int)src);
            for (uint32_t j0 = 0; j0 < nk_src; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool live = j < nk_src;
                body(skm_kmer_of<KW>(b0, b1, b2, live ? j : 0u, k), live, h_src, live ? j : 0u);
            }
        }
    }
}

// ---- S3: count ------------------------------------------------------------------------------------------
// dynamic LDS of the bucket kernels: [256] byte -> ASCII table, [T * C] bin cursors (count only), then the per-wave
// scratch: record-start bits of the walk, reused as the queue of occupied slots
__host__ __device__ inline uint32_t skm_wave_scratch_words(uint32_t sbw) { return sbw > 64u ? sbw : 64u; }

// FK: the instance for the k everybody runs (kevlar's default, 31; the host checks k and the record width): shifts, masks and the
// murmur tail become constants -- 3 % of the kernel.  FK = 0 reads k from the geometry.
// waves per SIMD the two-word-key instances are compiled for (6: three workgroups per CU at 80 VGPRs, 13-19 of them spilled; 4: two
// workgroups at up to 128 VGPRs, nothing spilled)
#define SKM_K2_WAVES 6
// The instances for a fixed k (FK != 0) take the two murmurs from the product tables (skm_key_hash_pl: P1 / P2, 4 KB of
// dynamic LDS in place of the 1 KB ASCII table) and keep their occurrence counters as 16-bit halves of a word -- that is where the
// 3 KB come from with three workgroups on a CU; the host launches them only for buckets that cannot hold 65536 occurrences
// (skm_count_pl_fits), the instances with k at run time count in 32 bits.
// slots of the k = 51 instances' table: their buckets are sized for 2048 slots (the scan kernels' tables), the count's own table may be
// roomier -- fewer occurrences on the loose list, shorter probe chains -- as long as three workgroups fit a CU (2560: 52.7 KB each)
#define SKM_TS51 2560
// (k = 31: 4608 slots measured 1 % faster than 4096 -- and let a bucket's distinct list outgrow what the list scan takes, SKM_LIST_MAX:
// scratch/fuzz_list.py seed 702, trial 149 lost 8 % of its hits; the table stays at 4096, the assertion below holds every instance to it)
#define SKM_TS31 4096
// entries of one bucket the scan from the distinct list takes (k_skm_novel_list): a bucket's list has at most as many entries as the
// count kernel's LDS table has slots
#define SKM_LIST_MAX 4096u
// FORCE_LOOSE: the instances KV_SKM_FORCE_LOOSE runs (sg.force_loose); the others leave its test out of the occurrence loop (0.07 ms per sample)
template <int KW, int TS, bool FORCE_LOOSE, int FK, bool COMPACT = false>
__global__ __launch_bounds__(SKM_THREADS3, KW == 2 ? SKM_K2_WAVES : 6) void k_skm_count(SkmGeom sg, const SketchDev *__restrict__ sk,
                                                           const SketchDev *__restrict__ mask, ConsumeFilter f, BinGeom g)
{
    static_assert((uint32_t)TS <= SKM_LIST_MAX, "a bucket's distinct list (one entry per occupied slot) must fit what k_skm_novel_list takes");
    constexpr bool PL = FK != 0;
    __shared__ SkmTable<KW, TS> tb;
    __shared__ uint32_t cnt[PL ? TS / 2 : TS];   // occurrences of the key in the same slot (PL: slot s in half s & 1 of word s >> 1)
    __shared__ uint32_t next_bucket;
    __shared__ uint32_t abl_cur, abl_b0, abl_prev;      // abundance list: entries appended so far, ... when the bucket began, the bucket
    __shared__ uint32_t dl_cur, dl_b0;                  // distinct list: the same two
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    const uint32_t ns = (uint32_t)(g.T * g.C);
    uint32_t *lut = dyn, *cur = dyn + (PL ? 1024 : 256), *scratch = cur + ((ns + 3u) & ~3u);
    uint64_t *P1 = (uint64_t *)dyn, *P2 = P1 + 256;
    for (uint32_t s = threadIdx.x; s < ns; s += SKM_THREADS3) cur[s] = 0;
    if (threadIdx.x < 256) {
        if (PL) { P1[threadIdx.x] = skm_ascii4_times(threadIdx.x, MM_C1); P2[threadIdx.x] = skm_ascii4_times(threadIdx.x, MM_C2); }
        else lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    }
    const HashParams hp = FK ? make_hash_params(FK, f.hp.hashfam) : f.hp;
    uint64_t n_added = 0, n_distinct = 0;
    const uint32_t cap1 = (uint32_t)g.cap1;
    uint32_t *my_seg = g.gbuf1 + (uint64_t)blockIdx.x * g.cap1;          // + stream * seg_stride: this workgroup's segment of a stream
    const uint64_t seg_stride = (uint64_t)g.nwgA * g.cap1;
    auto emit = [&](int t, uint64_t bin, uint32_t wgt) {
        const uint32_t slice = (uint32_t)(bin >> g.sbits);
        const uint32_t c = g.F == 1 ? slice : __umulhi(slice, g.recipF);
        const uint32_t sidx = (uint32_t)t * (uint32_t)g.C + c;
        const uint32_t item = ((slice - c * (uint32_t)g.F) << g.sbits) | ((uint32_t)bin & ((1u << g.sbits) - 1u)) | ((wgt - 1u) << BIN_W_SHIFT);
        const uint32_t pos = atomicAdd(&cur[sidx], 1u);
        if (pos < cap1) my_seg[sidx * seg_stride + pos] = item;
        else spill_item(g, t, bin, wgt);
    };
    // the table is emptied as it is read (below), so it is cleared only once; the next bucket's ticket is fetched
    // while the current bucket is processed
    skm_table_clear(tb);
    for (uint32_t i = threadIdx.x; i < (PL ? TS / 2 : TS); i += SKM_THREADS3) cnt[i] = 0;
    if (threadIdx.x == 0) { next_bucket = skm_first_bucket<SKM_CTR_TICKET_COUNT>(sg); abl_cur = 0; abl_b0 = 0; abl_prev = 0xffffffffu; dl_cur = 0; dl_b0 = 0; }
    // where the finished bucket's entries of the abundance list lie (nothing if the workgroup's stretch ran out)
    auto abl_close = [&]() {
        if (sg.abl_keys && abl_prev != 0xffffffffu) {
            const bool fits = abl_cur <= sg.abl_cap_wg;
            sg.abl_bstart[abl_prev] = blockIdx.x * sg.abl_cap_wg + abl_b0;
            sg.abl_bcount[abl_prev] = fits ? abl_cur - abl_b0 : 0u;
        }
        if (sg.dl_keys && abl_prev != 0xffffffffu) {
            sg.dl_bstart[abl_prev] = blockIdx.x * sg.dl_cap_wg + dl_b0;
            sg.dl_bcount[abl_prev] = dl_cur - dl_b0;                // (a stretch that ran out is reported through SKM_CTR_DL_RAN_OUT: the whole list is then dropped)
        }
    };
    for (uint32_t taken = 0; taken < sg.quota3; ++taken) {
        __syncthreads();
        const uint32_t b = next_bucket;
        if (b >= sg.n_buckets) break;
        __syncthreads();
        if (threadIdx.x == 0) {
            abl_close();
            abl_prev = b; abl_b0 = abl_cur; dl_b0 = dl_cur;
            skm_next_bucket<SKM_CTR_TICKET_COUNT, true, true>(sg, b, taken, next_bucket);
        }
        // combine the occurrences of the bucket
        skm_walk_bucket<KW, false, FK, COMPACT>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t) {
            // (KV_SKM_FORCE_LOOSE: one key in 64 is treated like a key that found its table full -- every occurrence travels alone;
            // results stay exact, tests use it to put single k-mers on the loose list of a batch that otherwise fits)
            const bool forced = FORCE_LOOSE && sg.force_loose && ((c.w[0] * 0x9e3779b97f4a7c15ull) >> 58) == 0;
            const int slot = skm_cacheable<KW>(c) && !forced ? skm_table_insert(tb, c) : -1;
            if (slot >= 0) {
                if (PL) atomicAdd(&cnt[(uint32_t)slot >> 1], 1u << (((uint32_t)slot & 1u) * 16u));
                else atomicAdd(&cnt[slot], 1u);
            }
            return slot < 0;         // table region full (or unstorable key): this occurrence travels alone
        });
        __syncthreads();
        // every distinct k-mer once
        skm_for_occupied<TS>(tb.key[0], (uint16_t *)scratch, skm_wave_scratch_words(sg.sbw) * 2u, [&](uint32_t slot) {
            const SkmKey<KW> c = skm_table_take(tb, slot);
            uint32_t seen;
            if (PL) {               // (the other half of the word is another lane's, maybe at this very moment)
                const uint32_t sh = (slot & 1u) * 16u;
                seen = (cnt[slot >> 1] >> sh) & 0xffffu;
                atomicSub(&cnt[slot >> 1], seen << sh);
            } else {
                seen = cnt[slot];
                cnt[slot] = 0;
            }
            n_distinct += 1;
            uint64_t h;
            if constexpr (PL) h = skm_key_hash_pl<KW, FK>(c, P1, P2);
            else h = skm_key_hash<KW>(c, lut, hp);
            // distinct list: key and hash of every k-mer in here (the scan of this batch then neither combines nor hashes again)
            if (sg.dl_keys) skm_dl_push<KW>(sg, &dl_cur, (uint64_t)blockIdx.x * sg.dl_cap_wg, sg.dl_cap_wg, c, h);
            uint32_t added;
            if (g.fast4 && !f.use_mask) {
                // four tables below 2^31 bins: the quotient of h / size from the FP64 pipe (kv_fastmod.h), the remainder in 32 bits --
                // h - q size lies in [-size, size), so its low word is the remainder or the remainder + 2^32 - size, told apart by bit 31 --
                // and the items appended with 32-bit index arithmetic: ~95 lane-instructions per k-mer for the 222 of the general form
                // (64-bit remainders, the sizes fetched from the sketch's descriptor, scalar registers spilled around them)
                const bool pass = !f.use_band || (h >= f.band_lo && h < f.band_hi);
                added = pass ? seen : 0u;
                if (pass) {
                    const double hd = kv_fastmod_hd(h);
                    uint32_t bin[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) bin[t] = kv_fastmod32(h, hd, (uint32_t)g.tsize[t], g.tmagic[t]);
                    uint32_t left = min(seen, 255u);
                    const uint32_t omask = (1u << g.sbits) - 1u, stride32 = (uint32_t)seg_stride;
                    while (left) {
                        const uint32_t wgt = min(left, BIN_W_MAX), wbits = (wgt - 1u) << BIN_W_SHIFT;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const uint32_t slice = bin[t] >> g.sbits;
                            const uint32_t c = g.F == 1 ? slice : __umulhi(slice, g.recipF);
                            const uint32_t sidx = (uint32_t)t * (uint32_t)g.C + c;
                            const uint32_t item = ((slice - c * (uint32_t)g.F) << g.sbits) | (bin[t] & omask) | wbits;
                            const uint32_t pos = atomicAdd(&cur[sidx], 1u);
                            if (pos < cap1) my_seg[sidx * stride32 + pos] = item;
                            else spill_item(g, t, (uint64_t)bin[t], wgt);
                        }
                        left -= wgt;
                    }
                }
            } else {
                added = skm_count_kmer(h, seen, sk, mask, f, g.T, emit);
            }
            n_added += added;
            // abundance list: a k-mer this batch adds at least twice (the lanes of the wave that are in here vote)
            if (sg.abl_keys) {
                const bool want = added >= 2u;
                const uint32_t at = skm_wave_reserve(&abl_cur, want);
                if (want && at < sg.abl_cap_wg) {
                    const uint64_t e = (uint64_t)blockIdx.x * sg.abl_cap_wg + at;
                    skm_key_store<KW>(sg.abl_keys, e, c);
                    sg.abl_cnts[e] = (uint8_t)min(added, 255u);
                }
            }
        });
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        abl_close();
        if (sg.dl_keys && dl_cur > sg.dl_cap_wg) atomicAdd(&sg.ctr[SKM_CTR_DL_RAN_OUT], 1ull);
    }
    for (uint32_t s = threadIdx.x; s < ns; s += SKM_THREADS3)
        g.gcnt1[(uint64_t)s * g.nwgA + blockIdx.x] = (uint32_t)min((uint64_t)cur[s], g.cap1);
    n_added = wave_sum_u64(n_added);
    n_distinct = wave_sum_u64(n_distinct);
    if ((threadIdx.x & 63) == 0 && n_added) atomicAdd(&g.ctr[BIN_CTR_ADDED], (unsigned long long)n_added);
    if ((threadIdx.x & 63) == 0 && n_distinct) atomicAdd(&sg.ctr[SKM_CTR_DISTINCT], (unsigned long long)n_distinct);
}

// loose records: every k-mer occurrence on its own, increments through the spill list (global atomics)
template <int KW>
__global__ __launch_bounds__(256) void k_skm_loose_count(SkmGeom sg, const SketchDev *__restrict__ sk,
                                                         const SketchDev *__restrict__ mask, ConsumeFilter f, BinGeom g)
{
    __shared__ uint32_t lut[256];
    if (sg.ctr[SKM_CTR_FAIL] != 0) return;                  // the pass was given up: the caller redoes the batch another way
    lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    __syncthreads();
    const int k = sg.k;
    uint64_t n_added = 0;
    // (every lane votes in spill_items_wave: the walk calls this wave-uniformly)
    skm_loose_walk_wave<KW>(sg, [&](const SkmKey<KW> &fw, bool live, uint64_t, uint32_t) {
        uint64_t h = 0;
        bool pass = false;
        if (live) {
            h = skm_key_hash<KW>(skm_canonical<KW>(fw, skm_revcomp<KW>(fw, k)), lut, f.hp);
            pass = consume_filter_pass(f, mask, h);
        }
        n_added += pass ? 1 : 0;
        uint64_t bins[BIN_MAX_T];
#pragma unroll
        for (int t = 0; t < BIN_MAX_T; ++t) bins[t] = (pass && t < g.T) ? fastmod(h, sk->size[t], sk->magic[t]) : 0ull;
        spill_items_wave(g, bins, 1u, pass);
    });
    n_added = wave_sum_u64(n_added);
    if ((threadIdx.x & 63) == 0 && n_added) atomicAdd(&g.ctr[BIN_CTR_ADDED], (unsigned long long)n_added);
}

// ---- S3': route (read-sharded multi-GPU count) ---------------------------------------------------------------
// Same walk as k_skm_count, but a distinct k-mer leaves as one (hash, count) item for the rank that owns the hash's
// band instead of T bin items: what crosses xGMI shrinks by the shard's own coverage, and the owner adds each item
// with one weighted saturating add per table (kv_consume_hashes_weighted).
#define SKM_ROUTE_MAX_DEST 16
// (out of line: a pair that misses its segment is rare in the kernels that call this from their drain, whose registers it must not cost)
struct SkmOverflowSink { unsigned long long *ctr; uint64_t *ovf; uint8_t *ovf_dest; uint64_t ovf_cap; int ndest; };
__device__ __attribute__((noinline)) void skm_route_overflow(SkmOverflowSink rs, uint32_t d, uint64_t h, uint64_t count)
{
    // the overflow list: one returning atomic for the lanes of the wave that are here together, not one each (the loose kernel sends
    // every item this way: 4.5 M of them took 25 ms one by one at ~180 per microsecond), and one add per destination among them
    const unsigned long long here = __ballot(true);
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)here) - 1u;
    unsigned long long o = 0;
    if (lane == leader) o = atomicAdd(&rs.ctr[ROUTE_CTR_OVERFLOW], (unsigned long long)__popcll(here));
    o = skm_shfl64(o, leader) + (unsigned long long)__popcll(here & ((1ull << lane) - 1ull));
    const bool fits = o < rs.ovf_cap;
    for (int dd = 0; dd < rs.ndest; ++dd) {
        const unsigned long long same = __ballot(fits && d == (uint32_t)dd);
        if (same && lane == (uint32_t)__ffsll((long long)same) - 1u) atomicAdd(&rs.ctr[ROUTE_CTR_DEST0 + dd], (unsigned long long)__popcll(same));
    }
    if (fits) {
        *(ulonglong2 *)(rs.ovf + 2 * o) = make_ulonglong2(h, count);
        rs.ovf_dest[o] = (uint8_t)d;
    }
}

__device__ __forceinline__ void skm_route_item(const KvRouteSink &rs, const uint64_t *lo, uint32_t *cur, uint64_t h, uint64_t count)
{
    if (h == UINT64_MAX) return;                 // the top hash value belongs to no band (kv_shard.hip)
    uint32_t d = 0;
    for (int b = 1; b < rs.ndest; ++b) d += h >= lo[b] ? 1u : 0u;
    const uint32_t pos = cur ? atomicAdd(&cur[d], 1u) : 0xffffffffu;
    if (pos < rs.seg_cap) *(ulonglong2 *)(rs.seg + (((uint64_t)d * rs.nwg + blockIdx.x) * rs.seg_cap + pos) * 2) = make_ulonglong2(h, count);
    else skm_route_overflow(SkmOverflowSink{rs.ctr, rs.ovf, rs.ovf_dest, rs.ovf_cap, rs.ndest}, d, h, count);
}

template <int KW, int TS, bool COMPACT = false>
__global__ __launch_bounds__(SKM_THREADS3, 6) void k_skm_route(SkmGeom sg, HashParams hp, KvRouteSink rs)
{
    __shared__ SkmTable<KW, TS> tb;
    __shared__ uint32_t cnt[TS];
    __shared__ uint32_t next_bucket;
    __shared__ uint32_t cur[SKM_ROUTE_MAX_DEST];
    __shared__ uint64_t lo[SKM_ROUTE_MAX_DEST];
    __shared__ uint32_t dl_cur, dl_b0, dl_prev;         // distinct list (sg.dl_keys != NULL: the owner will answer the scan from it, kv_skm_mex_scan_set)
    __shared__ uint32_t dl_org, dl_lim;                 // where the workgroup's entries start and how many fit: its own stretch, or (sg.dl_chunk) the chunk it drew last
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    uint32_t *lut = dyn, *scratch = dyn + 256;
    if (threadIdx.x < 256) lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    if (threadIdx.x < (uint32_t)rs.ndest) { cur[threadIdx.x] = 0; lo[threadIdx.x] = rs.bs * (uint64_t)threadIdx.x; }
    uint64_t n_distinct = 0;
    skm_table_clear(tb);
    for (uint32_t i = threadIdx.x; i < TS; i += SKM_THREADS3) cnt[i] = 0;
    if (threadIdx.x == 0) {
        next_bucket = skm_first_bucket<SKM_CTR_TICKET_COUNT>(sg); dl_cur = 0; dl_b0 = 0; dl_prev = 0xffffffffu;
        dl_org = sg.dl_chunk ? 0u : blockIdx.x * sg.dl_cap_wg; dl_lim = sg.dl_chunk ? 0u : sg.dl_cap_wg;
    }
    auto dl_close = [&]() {
        if (sg.dl_keys && dl_prev != 0xffffffffu) {
            sg.dl_bstart[dl_prev] = dl_org + dl_b0;
            sg.dl_bcount[dl_prev] = dl_cur - dl_b0;              // (a stretch that ran out is reported through SKM_CTR_DL_RAN_OUT: the whole list is then dropped)
            if (sg.dl_chunk && dl_cur > dl_lim) atomicAdd(&sg.ctr[SKM_CTR_DL_RAN_OUT], 1ull);
        }
    };
    // passes a bucket is combined in (see below), from its record count
    auto passes_of = [&](uint32_t b) {
        const uint32_t least = sg.passes > 1u ? sg.passes : 1u;
        const uint32_t *cnt2 = sg.cnt2 + (uint64_t)b * sg.nwg2;
        uint32_t nrec = 0;
        for (uint32_t s2 = 0; s2 < sg.nwg2; ++s2) nrec += cnt2[s2];
        // ~9.5 k-mers a record, a fifth of them distinct at sequencing coverage: 1.9 distinct k-mers per record, a pass's share under
        // 0.65 of the table.  Any number of passes (the class of a k-mer is a range of its hash, not a bit field): powers of two made the
        // average bucket of config 4 take 8 where 5 do.
        const uint32_t per_pass = (uint32_t)TS * 13u / 20u;
        const uint32_t want = (19u * nrec / 10u + per_pass - 1u) / per_pass;
        return min(64u, max(least, want));
    };
    for (uint32_t taken = 0; taken < sg.quota3; ++taken) {
        __syncthreads();
        const uint32_t b = next_bucket;
        if (b >= sg.n_buckets) break;
        __syncthreads();
        if (threadIdx.x == 0) {
            dl_close();
            if (sg.dl_keys && sg.dl_chunk) {
                // The pool (an owner whose share is too big for a stretch per workgroup with slack for the unevenness of their shares:
                // config 4's 7.9 G occurrences, 1.5 G of them distinct).  A bucket's list is one stretch, and a pass leaves at most a table's
                // worth of entries: a chunk that may not hold this bucket's is left as it is and the next one drawn.
                const uint32_t need = passes_of(b) * (uint32_t)TS;
                if (dl_cur + need > dl_lim) {
                    const unsigned long long c = atomicAdd(&sg.ctr[SKM_CTR_POOL_CHUNKS], 1ull);
                    if (c < sg.dl_nchunks && need <= sg.dl_chunk) { dl_org = (uint32_t)c * sg.dl_chunk; dl_lim = sg.dl_chunk; }
                    else { dl_org = 0; dl_lim = 0; atomicAdd(&sg.ctr[SKM_CTR_DL_RAN_OUT], 1ull); }          // the pool is empty (or the bucket beyond any chunk): no list
                    dl_cur = 0;
                }
            }
            dl_prev = b; dl_b0 = dl_cur;
            skm_next_bucket<SKM_CTR_TICKET_COUNT, true, false>(sg, b, taken, next_bucket);
        }
        // A sample too big for the bucket geometry (255 x 4096 buckets: beyond 8.5 G k-mers a bucket holds more distinct k-mers than the
        // table has slots) is combined in passes: pass p walks the whole bucket and takes the k-mers whose hash says p -- the walk is paid
        // once per pass, the inserts, the hashes and the pairs once in all (kv_skm_mex_route sets sg.passes)
        // (how many: by the bucket's own size -- with 12-base minimizers a million buckets are far from even, a popular minimizer makes
        // its bucket several times the average -- from its record count: ~9.5 k-mers a record, a fifth of them distinct at sequencing
        // coverage, a pass's share under 0.7 of the table; sg.passes, the estimate from the average, is the least)
        const uint32_t passes = passes_of(b);
        for (uint32_t pass = 0; pass < passes; ++pass) {
        if (pass) __syncthreads();                       // (the drain of the pass before empties the table)
        skm_walk_bucket<KW, false, 0, COMPACT>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t) {
            if (!skm_cacheable<KW>(c)) return pass == 0u;                                           // (travels alone, once)
            if (passes > 1u && __umulhi(skm_slot_hash<KW>(c) * 0x9E3779B1u, passes) != pass) return false;       // (bits the slot and the probe step do not come from)
            const int slot = skm_table_insert(tb, c);
            if (slot >= 0) atomicAdd(&cnt[slot], 1u);
            return slot < 0;
        });
        __syncthreads();
        skm_for_occupied<TS>(tb.key[0], (uint16_t *)scratch, skm_wave_scratch_words(sg.sbw) * 2u, [&](uint32_t slot) {
            const SkmKey<KW> c = skm_table_take(tb, slot);
            const uint32_t seen = cnt[slot];
            cnt[slot] = 0;
            n_distinct += 1;
            const uint64_t h = skm_key_hash<KW>(c, lut, hp);
            if (sg.dl_keys) skm_dl_push<KW>(sg, &dl_cur, dl_org, dl_lim, c, h);
            skm_route_item(rs, lo, cur, h, seen);
        });
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dl_close();
        if (sg.dl_keys && !sg.dl_chunk && dl_cur > sg.dl_cap_wg) atomicAdd(&sg.ctr[SKM_CTR_DL_RAN_OUT], 1ull);
    }
    if (threadIdx.x < (uint32_t)rs.ndest)
        rs.seg_count[(uint64_t)threadIdx.x * rs.nwg + blockIdx.x] = (uint32_t)min((uint64_t)cur[threadIdx.x], rs.seg_cap);
    n_distinct = wave_sum_u64(n_distinct);
    if ((threadIdx.x & 63) == 0 && n_distinct) atomicAdd(&sg.ctr[SKM_CTR_DISTINCT], (unsigned long long)n_distinct);
}

// loose records: one item of count 1 per k-mer occurrence, through the overflow list
template <int KW>
__global__ __launch_bounds__(256) void k_skm_loose_route(SkmGeom sg, HashParams hp, KvRouteSink rs)
{
    __shared__ uint32_t lut[256];
    __shared__ uint64_t lo[SKM_ROUTE_MAX_DEST];
    __shared__ uint32_t dcount[SKM_ROUTE_MAX_DEST];      // items of this workgroup per destination
    __shared__ uint32_t wg_items, wg_cur;
    __shared__ unsigned long long wg_base;
    if (sg.ctr[SKM_CTR_FAIL] != 0) return;
    lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    if (threadIdx.x < SKM_ROUTE_MAX_DEST) { lo[threadIdx.x] = rs.bs * (uint64_t)threadIdx.x; dcount[threadIdx.x] = 0; }
    if (threadIdx.x == 0) { wg_items = 0; wg_cur = 0; }
    __syncthreads();
    const uint64_t n = skm_loose_len(sg);
    // Every item here goes to the sink's overflow list.  Its slots are reserved ONCE per workgroup (the k-mers of the workgroup's records
    // are counted first: one header each) and dealt out through an LDS cursor, the per-destination totals are kept in LDS and added once
    // at the end: a returning device atomic per item -- then per wave -- made this kernel 25 and 10 ms for the 4.5 M loose k-mers of a
    // 75 M-read sample's owner, against 11 ms for the combine itself.
    {
        uint32_t mine = 0;
        for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
            mine += skm_hdr_n(sg.loose[i * (uint64_t)sg.lrecw]);
        if (mine) atomicAdd(&wg_items, mine);
    }
    __syncthreads();
    if (threadIdx.x == 0) wg_base = wg_items ? atomicAdd(&rs.ctr[ROUTE_CTR_OVERFLOW], (unsigned long long)wg_items) : 0ull;
    __syncthreads();
    // (This loop and the one of k_skm_loose_set_hits -- a thread per record that rolls through the record's k-mers -- are alike and stay
    // written out twice.  As one function that takes the per-k-mer body, in every form tried (header by value, by record pointer, the
    // length handed in or fetched inside) they cost 1 to 6 VGPRs more in each of the four instances, and the KW = 1 ones moved bw out of
    // the LDS the compiler parks it in; no occupancy changes, but the rule for this file is: no instance above what it had.)
    const int k = sg.k;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t *rec = sg.loose + i * (uint64_t)sg.lrecw;
        uint64_t bw[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? rec[1 + t] : 0ull;
        const uint32_t nk = skm_hdr_n(rec[0]);
        SkmKey<KW> fw = skm_first_kmer<KW>(bw, k);
        SkmKey<KW> rc = skm_revcomp<KW>(fw, k);
        for (uint32_t j = 0; j < nk; ++j) {
            if (j) skm_roll<KW>(fw, rc, skm_base_at(bw, j + (uint32_t)k - 1u), k);
            const uint64_t h = skm_key_hash<KW>(skm_canonical<KW>(fw, rc), lut, hp);
            const unsigned long long o = wg_base + atomicAdd(&wg_cur, 1u);
            if (o >= rs.ovf_cap) continue;
            uint32_t d = 0;
            for (int b = 1; b < rs.ndest; ++b) d += h >= lo[b] ? 1u : 0u;
            if (h == UINT64_MAX) d = 0xffu;             // (the top hash value belongs to no band: the slot stays, marked -- k_route_tail skips it)
            else atomicAdd(&dcount[d], 1u);
            *(ulonglong2 *)(rs.ovf + 2 * o) = make_ulonglong2(h, 1ull);
            rs.ovf_dest[o] = (uint8_t)d;
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)rs.ndest && dcount[threadIdx.x]) atomicAdd(&rs.ctr[ROUTE_CTR_DEST0 + threadIdx.x], (unsigned long long)dcount[threadIdx.x]);
}

// ---- S6: novel ------------------------------------------------------------------------------------------
__device__ __forceinline__ void skm_mark(const NovelParams &p, const ReadsDev &rd, uint64_t pos, uint64_t stride)
{
    const uint64_t read = pos / stride;
    const uint64_t off = pos - read * stride;
    if ((rd.flags[read] & 1) || read < p.first_read) return;     // the scan skips these reads (kevlar/novel.py:134-139)
    const uint64_t bit = read * p.mask_stride + off;
    atomicOr(&p.mask[bit >> 5], 1u << (bit & 31));
}

template <int KW, int TS>
__global__ __launch_bounds__(SKM_THREADS3, 6) void k_skm_novel(SkmGeom sg, ReadsDev rd, NovelParams p, SkmAblSet abls)
{
    __shared__ SkmTable<KW, TS> tb;
    __shared__ uint32_t flag[TS / 32];           // bit per slot: the key is interesting
    __shared__ uint32_t rej[TS / 32];            // bit per slot: a control's abundance list rejects the key (no probe needed)
    __shared__ NovelShared ns;
    __shared__ uint32_t next_bucket, any_hit;
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    uint32_t *lut = dyn, *scratch = dyn + 256;
    if (threadIdx.x < 256) lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    load_descs(ns, p);
    if (threadIdx.x == 0) next_bucket = skm_first_bucket<SKM_CTR_TICKET_SCAN>(sg);
    for (uint32_t taken = 0; taken < sg.quota3; ++taken) {
        __syncthreads();
        const uint32_t b = next_bucket;
        if (b >= sg.n_buckets) break;
        skm_table_clear(tb);
        if (threadIdx.x < TS / 32) { flag[threadIdx.x] = 0; rej[threadIdx.x] = 0; }
        __syncthreads();
        if (threadIdx.x == 0) {
            skm_next_bucket<SKM_CTR_TICKET_SCAN, true, true>(sg, b, taken, next_bucket);      // (the count pass's early exit, for a scan that cut the batch itself)
            any_hit = 0;
        }
        // collect the distinct k-mers
        skm_walk_bucket<KW, true, 0, false>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t) {
            const int slot = skm_cacheable<KW>(c) ? skm_table_insert(tb, c) : -1;
            return slot < 0;
        });
        // the k-mers of this bucket that a control is known to hold more than ctrl_max times (KvAbundList): they go into the
        // same table, marked; whichever of them the case sample has too is then skipped by the evaluation.  A full table
        // only costs the shortcut for that key.
        // (this loop over the rejected entries stands in k_skm_novel_list too.  As one function that takes the insert as its body -- the set
        // by reference or by value, or only the inner loop shared -- it changed no register count but grew this kernel by 750 (KW = 1) and
        // 1650 (KW = 2) instructions and the list scan by 350: both keep the loop written out, and with it the parent's code.)
        for (int a = 0; a < abls.n; ++a) {
            const uint32_t a0 = abls.bstart[a][b], an = abls.bcount[a][b];
            for (uint32_t i = threadIdx.x; i < an; i += SKM_THREADS3) {
                if ((int)min((uint32_t)abls.cnts[a][a0 + i], abls.maxv[a]) <= abls.ctrl_max) continue;
                const SkmKey<KW> c = skm_key_load<KW>(abls.keys[a], a0 + i);
                const int slot = skm_table_insert(tb, c);
                if (slot >= 0) atomicOr(&rej[slot >> 5], 1u << (slot & 31));
            }
        }
        __syncthreads();
        // evaluate each of them once
        skm_for_occupied<TS>(tb.key[0], (uint16_t *)scratch, skm_wave_scratch_words(sg.sbw) * 2u, [&](uint32_t slot) {
            const uint64_t h = skm_key_hash<KW>(skm_table_key(tb, slot), lut, p.hp);
            if (band_pass(p, h) && novel_test_fast(ns, p, h, nullptr, 0ull)) { atomicOr(&flag[slot >> 5], 1u << (slot & 31)); any_hit = 1; }
        }, rej);            // (keys a control's list rejects are not queued: 25 M of 106 M at config 2, lanes that used to sit out their wave's hashes)
        __syncthreads();
        if (any_hit == 0) continue;
        // mark every occurrence of an interesting k-mer (an occurrence whose key is absent went to the loose list)
        skm_walk_bucket<KW, true, 0, false>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t pos) {
            if (!skm_cacheable<KW>(c)) return false;
            const int slot = skm_table_find(tb, c);
            if (slot >= 0 && ((flag[slot >> 5] >> (slot & 31)) & 1u)) skm_mark(p, rd, pos, sg.stride);
            return false;
        });
    }
}

// bits[w] bit j = (tab[32 w + j] >= case_min), byte counters: the first probe of the list scan as a bit map (NovelParams::case0_bits)
__global__ __launch_bounds__(256) void k_case_bits(const uint8_t *__restrict__ tab, uint64_t size, int case_min, uint32_t *__restrict__ bits)
{
    const uint64_t n_words = (size + 31) >> 5;
    for (uint64_t w = blockIdx.x * 256ull + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256ull) {
        uint32_t out = 0;
        if (w * 32 + 32 <= size) {
            const uint4 a = ((const uint4 *)tab)[2 * w], b = ((const uint4 *)tab)[2 * w + 1];
            const uint32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) out |= ((int)((q[i] >> (8 * j)) & 0xffu) >= case_min ? 1u : 0u) << (4 * i + j);
        } else {
            for (uint64_t j = w * 32; j < size; ++j) out |= ((int)tab[j] >= case_min ? 1u : 0u) << (uint32_t)(j - w * 32);
        }
        bits[w] = out;
    }
}

// The scan of a batch whose count pass left a distinct list (SkmGeom::dl_*): nothing is combined and nothing is hashed again.
// Per bucket: (1) the controls' abundance-list entries that exceed ctrl_max go into one small LDS table (the k-mers no probe is
// needed for); (2) every entry of the distinct list that is not in there gets ONE probe -- table 0 of the first case sample, where
// a sequencing-error k-mer ends -- four entries per thread in flight and no barrier anywhere, and the few that pass are queued;
// (3) the queue is dealt one candidate per thread for the rest of kmer_is_interesting() (a dozen dependent probes: paid once per
// bucket, side by side, instead of once per wave and round); the interesting ones go into a second table, and (4) only if there
// are any are the bucket's records walked, to mark their occurrences.  Occurrences that missed the count pass's LDS tables are in
// the loose list already (k_skm_loose_novel evaluates them one by one).  A bucket's list has at most as many entries as the count
// kernel's LDS table has slots.
template <int KW, int TSM>
__global__ __launch_bounds__(SKM_THREADS3, 6) void k_skm_novel_list(SkmGeom sg, ReadsDev rd, NovelParams p, SkmAblSet abls)
{
    constexpr uint32_t E = 4;                    // entries a thread has in flight (2 / 4 / 6 measured: 2.64 / 2.6-2.8 / 2.52 ms, within the spread between runs)
    __shared__ SkmTable<KW, TSM> rtb;            // rejected by a control's list
    __shared__ SkmTable<KW, TSM> itb;            // interesting
    __shared__ NovelShared ns;
    __shared__ uint16_t cand[SKM_LIST_MAX];      // entries (relative to the bucket's first) that passed the first probe
    __shared__ uint32_t next_bucket, n_int, n_cand;
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    uint32_t *scratch = dyn;
    load_descs(ns, p);
    skm_table_clear(itb);
    if (threadIdx.x == 0) { next_bucket = skm_first_bucket<SKM_CTR_TICKET_SCAN>(sg); n_int = 0; n_cand = 0; }
    auto mark_pass = [&](uint32_t b) {
        skm_walk_bucket<KW, true, 0, false>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t pos) {
            if (skm_cacheable<KW>(c) && skm_table_find(itb, c) >= 0) skm_mark(p, rd, pos, sg.stride);
            return false;
        });
        __syncthreads();
        skm_table_clear(itb);
        if (threadIdx.x == 0) n_int = 0;
        __syncthreads();
    };
    for (uint32_t taken = 0; taken < sg.quota3; ++taken) {
        __syncthreads();
        const uint32_t b = next_bucket;
        if (b >= sg.n_buckets) break;
        skm_table_clear(rtb);
        __syncthreads();
        if (threadIdx.x == 0) {
            skm_next_bucket<SKM_CTR_TICKET_SCAN, true, false>(sg, b, taken, next_bucket);
            n_cand = 0;
        }
        // the first list entries are requested before the controls' lists are worked in: they arrive meanwhile
        const uint32_t e0 = sg.dl_bstart[b], en = min(sg.dl_bcount[b], SKM_LIST_MAX);
        SkmKey<KW> c[E];
        uint64_t h[E];
        auto request = [&](uint32_t base) {
#pragma unroll
            for (uint32_t u = 0; u < E; ++u) {
                const uint32_t i = base + u * SKM_THREADS3 + threadIdx.x;
                const bool in = i < en;
                c[u] = skm_key_load<KW>(sg.dl_keys, e0 + i, in);
                h[u] = in ? sg.dl_hash[e0 + i] : 0ull;
            }
        };
        request(0);
        // (the loop of k_skm_novel, which says why it is written out twice)
        for (int a = 0; a < abls.n; ++a) {
            const uint32_t a0 = abls.bstart[a][b], an = abls.bcount[a][b];
            for (uint32_t i = threadIdx.x; i < an; i += SKM_THREADS3) {
                if ((int)min((uint32_t)abls.cnts[a][a0 + i], abls.maxv[a]) <= abls.ctrl_max) continue;
                const SkmKey<KW> c = skm_key_load<KW>(abls.keys[a], a0 + i);
                (void)skm_table_insert(rtb, c);              // (a full table only costs the shortcut for that key)
            }
        }
        __syncthreads();
        for (uint32_t e0 = 0; e0 < en; e0 += E * SKM_THREADS3) {
            if (e0) request(e0);
            bool live[E];
            uint32_t v[E];
#pragma unroll
            for (uint32_t u = 0; u < E; ++u) {
                live[u] = e0 + u * SKM_THREADS3 + threadIdx.x < en && skm_table_find(rtb, c[u]) < 0 && band_pass(p, h[u]);
                if (p.case0_bits) {
                    const uint64_t bin = fastmod(h[u], ns.d[0].size, ns.d[0].magic);
                    const __attribute__((address_space(1))) uint32_t *bits = (const __attribute__((address_space(1))) uint32_t *)p.case0_bits;
                    v[u] = live[u] && ((bits[bin >> 5] >> (uint32_t)(bin & 31u)) & 1u) ? (uint32_t)p.case_min : 0u;
                } else {
                    v[u] = live[u] ? probe(ns, 0, 0, h[u]) : 0u;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < E; ++u)
                if (live[u] && (int)v[u] >= p.case_min) cand[atomicAdd(&n_cand, 1u)] = (uint16_t)(e0 + u * SKM_THREADS3 + threadIdx.x);
        }
        __syncthreads();
        const uint32_t nc = n_cand;
        for (uint32_t j0 = 0; j0 < nc; j0 += SKM_THREADS3) {
            const uint32_t j = j0 + threadIdx.x;
            if (j < nc) {
                const uint32_t i = cand[j];
                const SkmKey<KW> c = skm_key_load<KW>(sg.dl_keys, e0 + i);
                const uint64_t h = sg.dl_hash[e0 + i];
                if (novel_test_wide(ns, p, h)) {
                    if (skm_table_insert(itb, c) < 0) sg.ctr[SKM_CTR_FAIL] = 1;          // (cannot happen below half full; the caller then redoes the scan the other way)
                    atomicAdd(&n_int, 1u);
                    if (p.ab_keys) (void)ab_claim(p, h, p.ncase + p.nctrl);      // a place for its abundances (k_ab_fill), for the kernel that reports the hits
                }
            }
            __syncthreads();
            // a bucket with more interesting k-mers than a quarter of the table (a case sample without controls to speak of)
            // marks in instalments
            if (n_int > TSM / 4 && j0 + SKM_THREADS3 < nc) mark_pass(b);
        }
        if (n_int != 0) mark_pass(b);
    }
}

// the abundances of the k-mers k_skm_novel_list claimed a slot for (a dozen probes each, side by side, off the scan's critical path:
// inside the scan they were a chain of round trips in front of a workgroup barrier, 0.25 ms)
__global__ __launch_bounds__(256) void k_ab_fill(NovelParams p)
{
    __shared__ NovelShared ns;
    load_descs(ns, p);
    __syncthreads();
    const int S = p.ncase + p.nctrl;
    // the slots that were claimed are on a list (ab_claim) -- some 10^5 of the table's 8 M at config 2, whose walk was 0.11 ms; a list
    // that ran out of room sends the kernel over the whole table as before
    const unsigned int listed = p.ab_list ? *p.ab_count : 0xffffffffu;
    if (listed <= p.ab_list_cap) {
        for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < listed; i += (uint64_t)gridDim.x * 256ull) {
            const uint64_t slot = p.ab_list[i];
            hit_abundances(ns, p, (uint64_t)p.ab_keys[slot], p.ab_vals + slot * (uint64_t)S);
        }
        return;
    }
    for (uint64_t slot = blockIdx.x * 256ull + threadIdx.x; slot <= p.ab_mask; slot += (uint64_t)gridDim.x * 256ull) {
        const unsigned long long h = p.ab_keys[slot];
        if (h != 0ull) hit_abundances(ns, p, (uint64_t)h, p.ab_vals + slot * (uint64_t)S);
    }
}

template <int KW>
__global__ __launch_bounds__(256) void k_skm_loose_novel(SkmGeom sg, ReadsDev rd, NovelParams p)
{
    __shared__ uint32_t lut[256];
    __shared__ NovelShared ns;
    lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    load_descs(ns, p);
    __syncthreads();
    const int k = sg.k;
    skm_loose_walk_wave<KW>(sg, [&](const SkmKey<KW> &fw, bool live, uint64_t hdr, uint32_t j) {
        if (!live) return;
        const uint64_t h = skm_key_hash<KW>(skm_canonical<KW>(fw, skm_revcomp<KW>(fw, k)), lut, p.hp);
        if (band_pass(p, h) && novel_test_fast(ns, p, h, nullptr, 0ull)) skm_mark(p, rd, skm_hdr_pos_of(hdr, j), sg.stride);
    });
}

// ---- the scan answered by the owner of the minimizer buckets (minimizer-sharded exchange, kv_skm_mex_scan_set) ----------------
// After kv_skm_mex_route(keep_scan) this rank holds every occurrence of the k-mers of its buckets -- from whichever shard, with the
// global (read, offset) of each in the record headers -- and key + hash of every distinct one (the distinct list k_skm_route left).
// Once the band owners' verdicts have been gathered into the set of interesting hashes, the hits are these: per bucket, the list
// entries that are members go into a small LDS table with their slot of the set; only if there are any is the bucket walked, and every
// occurrence of a member leaves as (read << 16 | offset, the S abundances the set carries) -- the form kv_hits_from_tagged sorts.
// Hits are staged in LDS and appended with one update of the device-wide counter per flush (that counter takes ~90 updates per
// microsecond however they are issued); a bucket with more hits than the stage holds appends the rest one by one.
struct SetHitSink {
    unsigned long long *tags;
    uint8_t *abund;
    unsigned long long *count;
    uint64_t cap;
};
__device__ __forceinline__ void set_hit_store(const NovelParams &p, const SetHitSink &out, uint64_t at, unsigned long long tag, uint64_t slot)
{
    if (at >= out.cap) return;
    const int S = p.ncase + p.nctrl;
    out.tags[at] = tag;
    for (int c = 0; c < S; ++c) out.abund[at * (uint64_t)S + c] = p.set_abund[slot * (uint64_t)S + c];
}
#define SKM_HIT_STAGE 1024u
template <int KW, int TSM>
__global__ __launch_bounds__(SKM_THREADS3, 6) void k_skm_set_hits(SkmGeom sg, NovelParams p, SetHitSink out)
{
    __shared__ SkmTable<KW, TSM> itb;            // the bucket's members of the set
    __shared__ uint32_t islot[TSM];              // their slots of the set
    __shared__ unsigned long long htag[SKM_HIT_STAGE];
    __shared__ uint32_t hslot[SKM_HIT_STAGE];
    __shared__ uint32_t next_bucket, n_int, n_hit;
    __shared__ unsigned long long flush_base;
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    uint32_t *scratch = dyn;
    skm_table_clear(itb);
    if (threadIdx.x == 0) { next_bucket = skm_first_bucket<SKM_CTR_TICKET_SCAN>(sg); n_int = 0; n_hit = 0; }
    for (uint32_t taken = 0; taken < sg.quota3; ++taken) {
        __syncthreads();
        const uint32_t b = next_bucket;
        if (b >= sg.n_buckets) break;
        __syncthreads();
        if (threadIdx.x == 0) skm_next_bucket<SKM_CTR_TICKET_SCAN, false, false>(sg, b, taken, next_bucket);      // (a raised flag does not end this pass)
        const uint32_t e0 = sg.dl_bstart[b], en = sg.dl_bcount[b];
        for (uint32_t i = threadIdx.x; i < en; i += SKM_THREADS3) {
            const uint64_t h = sg.dl_hash[e0 + i];
            const uint64_t slot = set_find(p, h);
            if (slot == KV_SET_NONE) continue;
            const int at = skm_table_insert(itb, skm_key_load<KW>(sg.dl_keys, e0 + i));
            if (at < 0) { sg.ctr[SKM_CTR_FAIL] = 1; continue; }            // more members than the table takes: the caller scans the other way
            islot[at] = (uint32_t)slot;
            atomicAdd(&n_int, 1u);
        }
        __syncthreads();
        if (n_int == 0) continue;
        skm_walk_bucket<KW, true, 0, false>(sg, b, scratch, [&](const SkmKey<KW> &c, uint64_t pos) {
            if (!skm_cacheable<KW>(c)) return false;
            const int at = skm_table_find(itb, c);
            if (at < 0) return false;
            const uint64_t read = pos / sg.stride;
            const unsigned long long tag = ((unsigned long long)read << 16) | (unsigned long long)(pos - read * sg.stride);
            const uint32_t i = atomicAdd(&n_hit, 1u);
            if (i < SKM_HIT_STAGE) { htag[i] = tag; hslot[i] = islot[at]; }
            else set_hit_store(p, out, atomicAdd(out.count, 1ull), tag, islot[at]);
            return false;
        });
        __syncthreads();
        const uint32_t staged = min(n_hit, SKM_HIT_STAGE);
        if (threadIdx.x == 0) flush_base = atomicAdd(out.count, (unsigned long long)staged);
        skm_table_clear(itb);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < staged; i += SKM_THREADS3) set_hit_store(p, out, flush_base + i, htag[i], hslot[i]);
        if (threadIdx.x == 0) { n_int = 0; n_hit = 0; }
    }
}

// the occurrences that travelled alone (records of the loose list: one k-mer each from the combine, whole records from the split)
template <int KW>
__global__ __launch_bounds__(256) void k_skm_loose_set_hits(SkmGeom sg, NovelParams p, SetHitSink out)
{
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = skm_ascii4(threadIdx.x);
    __syncthreads();
    const uint64_t n = skm_loose_len(sg);
    const int k = sg.k;
    // (the loop of k_skm_loose_route, which says why it is written out twice)
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t *rec = sg.loose + i * (uint64_t)sg.lrecw;
        uint64_t bw[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bw[t] = t < sg.nbw ? rec[1 + t] : 0ull;
        const uint32_t nk = skm_hdr_n(rec[0]);
        SkmKey<KW> fw = skm_first_kmer<KW>(bw, k);
        SkmKey<KW> rc = skm_revcomp<KW>(fw, k);
        for (uint32_t j = 0; j < nk; ++j) {
            if (j) skm_roll<KW>(fw, rc, skm_base_at(bw, j + (uint32_t)k - 1u), k);
            const uint64_t slot = set_find(p, skm_key_hash<KW>(skm_canonical<KW>(fw, rc), lut, p.hp));
            if (slot == KV_SET_NONE) continue;
            const uint64_t pos = skm_hdr_pos_of(rec[0], j), read = pos / sg.stride;
            set_hit_store(p, out, atomicAdd(out.count, 1ull), ((unsigned long long)read << 16) | (unsigned long long)(pos - read * sg.stride), slot);
        }
    }
}

__global__ void k_skm_forward_flag(const unsigned long long *skm_ctr, unsigned long long *bin_ctr)
{
    if (skm_ctr[SKM_CTR_FAIL] != 0) bin_ctr[BIN_CTR_FAIL] = 1;
}

// hits per tile = set bits of the tile's range of the mask (what k_novel_mark counts while it marks)
__global__ __launch_bounds__(64) void k_tile_hits(ReadsDev rd, NovelParams p)
{
    const TileDesc td = rd.tile[blockIdx.x];
    uint64_t b0, b1;
    if (td.seg) {
        b0 = (uint64_t)td.first * p.mask_stride + td.seg_start;
        b1 = min(b0 + (uint64_t)KV_SEG_BASES, ((uint64_t)td.first + 1) * p.mask_stride);
    } else {
        b0 = (uint64_t)td.first * p.mask_stride;
        b1 = ((uint64_t)td.first + td.count) * p.mask_stride;
    }
    uint64_t n = 0;
    for (uint64_t w = (b0 >> 5) + threadIdx.x; w < ((b1 + 31) >> 5); w += 64) {
        uint32_t bits = p.mask[w];
        const uint64_t wlo = w << 5;
        if (wlo < b0) bits &= ~0u << (uint32_t)(b0 - wlo);
        if (wlo + 32 > b1) bits &= b1 > wlo ? (~0u >> (uint32_t)(wlo + 32 - b1)) : 0u;
        n += (uint32_t)__popc(bits);
    }
    n = wave_sum_u64(n);
    if (threadIdx.x == 0) p.tile_count[blockIdx.x] = (uint32_t)n;
}

}  // namespace
