// kv_gunzip_plan.h -- the host arithmetic of the parallel gzip decoder (kv_gunzip.hip), free of HIP: which compressed bytes a
// segment takes, which found block starts become stretches, where long stretches are cut, how much room each decoder gets, which
// results form the text (the chain rule) and how the text is cut into CRC-32 ranges.  Plain C++17: kv_gunzip.hip includes it for
// the structs its kernels share with the host and calls these functions between its launches; tests/harness/gunzip_plan_host.cpp
// compiles it for the host, and tests/test_gunzip_plan.py holds it to a Python restatement and a simulated decoder, without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#define GZ_FIND_KEEP 4u              // block starts kept per chunk
#define GZ_MARGIN (4ull << 20)       // bytes behind a segment in which the next segment's first block is looked for
#define GZ_MAX_REPAIRS 200u          // stretches of one segment that may be decoded again
#define GZ_MAX_CAP 0x7ffffff0u       // symbols of room one stretch can have

enum { GZ_LANDED = 0, GZ_END = 1, GZ_BAD = 2, GZ_FULL = 3, GZ_SHORT = 4 };

struct GzJob {
    uint64_t start_bit;              // first symbol (or block header) to decode, relative to the compressed buffer
    uint64_t target_idx;             // starts[target_idx]: the first start behind start_bit; the stretch stops ON the first start it meets
    uint64_t out_off;                // symbols
    uint64_t header_bit;             // header of the block start_bit lies in (== start_bit for a stretch that begins with a block)
    uint32_t out_cap;
    uint32_t pad;
};
struct GzGuess {
    uint64_t header_bit;             // a found block start ...
    uint64_t guess_bit;              // ... and a place inside that block near which a symbol boundary is wanted
};
struct GzResult {
    uint64_t end_bit;
    uint32_t n_out;
    uint16_t status;
    uint16_t members;                // member trailers the stretch passed,
    uint32_t isize_sum;              // ... the sum of their ISIZE fields,
    uint32_t trailer_at;             // ... how many symbols the stretch had produced at the first one
    uint32_t trailer_crc;            // ... and the CRC-32 that one announces
    uint32_t pad;
};

static inline uint64_t gz_round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// ---- the compressed bytes of a segment, and behind them a margin in which the next segment's first block is looked for
struct GzExtent {
    uint64_t first_byte, seg_end, upto;       // in the file: the buffer is [first_byte, upto), the segment ends at seg_end
    uint64_t n_bytes;
    uint32_t n_chunks;
    bool to_file_end, is_file_end;            // the segment / the buffer reaches the end of the file
    uint64_t start_rel, seg_end_rel;          // bits in the buffer: where the last segment ended, where this one may
};
static inline GzExtent gz_segment_extent(uint64_t pos_bit, uint64_t file_size, uint64_t want_text, double ratio, uint32_t chunk_bytes)
{
    GzExtent x;
    x.first_byte = (pos_bit >> 3) & ~255ull;
    const uint64_t seg = std::max<uint64_t>((uint64_t)((double)want_text / ratio), 4ull * chunk_bytes);
    x.seg_end = std::min<uint64_t>(gz_round_up(x.first_byte + seg, chunk_bytes), file_size);
    x.upto = std::min<uint64_t>(x.seg_end + GZ_MARGIN, file_size);
    x.to_file_end = x.seg_end == file_size;
    x.is_file_end = x.upto == file_size;
    x.n_bytes = x.upto - x.first_byte;
    x.n_chunks = (uint32_t)((x.n_bytes + chunk_bytes - 1) / chunk_bytes);
    x.start_rel = pos_bit - x.first_byte * 8;
    x.seg_end_rel = (x.seg_end - x.first_byte) * 8;
    return x;
}

// ---- stretches: from the exact position the last segment ended at, then from every found start up to the first one behind
// the segment
struct GzStarts {
    std::vector<uint64_t> starts;             // ascending; starts[0] is exact
    std::vector<uint64_t> headers;            // headers[i]: the block header stretch i takes its codes from
    bool have_terminal = false;               // the last start lies behind the segment: reaching it (stop_rel) ends the segment
    uint64_t stop_rel = ~0ull;
    size_t n_first() const { return have_terminal ? starts.size() - 1 : starts.size(); }      // stretches decoded in the first launch
};
// cand: what k_gz_find kept, GZ_FIND_KEEP per chunk, ~0 for none.  false: no block start within the margin (none before the
// end of the file is fine: the last stretch runs to the end)
static inline bool gz_starts(const GzExtent &x, const unsigned long long *cand, uint64_t n_cand, GzStarts *s)
{
    s->starts.assign(1, x.start_rel);
    s->have_terminal = false;
    for (uint64_t c = 0; c < n_cand && !s->have_terminal; ++c) {
        if (cand[c] == ~0ull || cand[c] <= x.start_rel) continue;
        s->starts.push_back(cand[c]);
        if (!x.to_file_end && cand[c] >= x.seg_end_rel) s->have_terminal = true;
    }
    s->headers = s->starts;
    s->stop_rel = s->have_terminal ? s->starts.back() : ~0ull;
    return x.to_file_end || s->have_terminal || x.is_file_end;
}

// ---- long stretches are cut: places inside their first block near which k_gz_sync looks for a symbol boundary.
// Only when the block starts alone leave the device short of work (fewer than 24 stretches per CU: wanted_stretches is 32 per
// CU), and then as many pieces as make 32 per CU: every cut costs a header to parse, a tail to resolve and a decoder that looks
// for its target between symbols too (k_gz_decode<.., true>, ~15 % more instructions per symbol)
static inline std::vector<GzGuess> gz_cut_guesses(const GzExtent &x, const GzStarts &s, uint64_t wanted_stretches, uint64_t max_guesses)
{
    const std::vector<uint64_t> &starts = s.starts;
    // (bits of compressed data a piece should have; 0: no cutting)
    const uint64_t piece = starts.size() * 4 >= wanted_stretches * 3 ? 0 : std::max<uint64_t>(4096ull * 8ull, (x.seg_end_rel - x.start_rel) / wanted_stretches);
    std::vector<GzGuess> guesses;
    const size_t n_blocks = s.n_first();
    for (size_t j = 0; j < n_blocks && piece; ++j) {
        const uint64_t next = j + 1 < starts.size() ? starts[j + 1] : x.n_bytes * 8;
        const uint64_t span = next - starts[j];
        const uint64_t cuts = std::min<uint64_t>(8, span / piece);
        for (uint64_t i = 1; i < cuts; ++i) {
            GzGuess gs;
            gs.header_bit = starts[j];
            gs.guess_bit = starts[j] + i * (span / cuts);
            if (guesses.size() < max_guesses) guesses.push_back(gs);
        }
    }
    return guesses;
}

// the boundaries k_gz_sync found (found[i] for guesses[i], ~0: none) join the starts, sorted and without duplicates; returns
// how many were taken
static inline uint64_t gz_merge_cuts(GzStarts *s, const std::vector<GzGuess> &guesses, const unsigned long long *found)
{
    std::vector<uint64_t> &starts = s->starts, &headers = s->headers;
    uint64_t taken = 0;
    std::vector<std::pair<uint64_t, uint64_t>> all;             // (start, header)
    for (size_t i = 0; i < starts.size(); ++i) all.emplace_back(starts[i], starts[i]);
    for (size_t i = 0; i < guesses.size(); ++i) {
        if (found[i] == ~0ull || found[i] <= guesses[i].header_bit || found[i] >= s->stop_rel) continue;
        // (a boundary behind the next block start is of no use: the stretch before it stops at that start)
        const auto nx = std::upper_bound(starts.begin(), starts.end(), guesses[i].header_bit);
        if (nx != starts.end() && found[i] >= *nx) continue;
        all.emplace_back(found[i], guesses[i].header_bit);
        taken += 1;
    }
    std::sort(all.begin(), all.end());
    starts.clear(); headers.clear();
    for (const auto &a : all)
        if (starts.empty() || a.first != starts.back()) { starts.push_back(a.first); headers.push_back(a.second); }
    return taken;
}

// ---- one job per stretch of the first launch, and the room each gets in the symbol buffer
struct GzPlan {
    std::vector<GzJob> jobs;
    uint64_t total_cap = 0;                   // symbols the first launch's jobs take; the repairs' room lies behind it
    uint64_t repair_room = 0;
    bool exact = false;                       // does any stretch begin inside a block?
    double factor = 0;
    // symbols of room for a stretch of `bits` of compressed data
    uint32_t room(uint64_t bits) const { return (uint32_t)std::min<uint64_t>((uint64_t)((double)(bits / 8 + 1) * factor) + 16384, GZ_MAX_CAP); }
};
static inline GzPlan gz_plan_jobs(const GzStarts &s, uint64_t n_bytes, double ratio)
{
    const std::vector<uint64_t> &starts = s.starts, &headers = s.headers;
    GzPlan p;
    for (size_t i = 0; i < starts.size() && !p.exact; ++i) p.exact = headers[i] != starts[i];
    p.factor = std::min(std::max(2.5 * ratio, 8.0), 64.0);
    p.jobs.resize(s.n_first());
    for (size_t j = 0; j < p.jobs.size(); ++j) {
        // room: up to the next stretch that begins with a block (the starts inside this block may turn out not to be any, and
        // the stretch then runs on over them)
        size_t nb = j + 1;
        while (nb < starts.size() && headers[nb] != starts[nb]) ++nb;
        const uint64_t next = nb < starts.size() ? starts[nb] : n_bytes * 8;
        p.jobs[j].start_bit = starts[j];
        p.jobs[j].header_bit = headers[j];
        p.jobs[j].target_idx = j + 1;                   // (starts[] on the device ends with ~0)
        p.jobs[j].out_off = p.total_cap;
        p.jobs[j].out_cap = p.room(next - starts[j]);
        p.jobs[j].pad = 0;
        p.total_cap += gz_round_up(p.jobs[j].out_cap, 64);
    }
    p.repair_room = std::max<uint64_t>(256ull << 20, p.total_cap / 4);
    return p;
}

// ---- the chain: stretch 0 starts at a known block; a later one counts iff a good stretch ends exactly on its start; a start
// that was run over was a false positive and its output is dropped; a gap, or a stretch out of room, is decoded again
enum { GZ_WALK_OK = 0, GZ_WALK_REPAIRS = 1, GZ_WALK_BAD = 2, GZ_WALK_SHORT = 3, GZ_WALK_DEVICE = 4 };
struct GzChain {
    std::vector<uint64_t> v_off, v_base;      // of every accepted stretch: where its symbols are, where its text goes
    std::vector<uint32_t> v_n;
    std::vector<std::pair<uint64_t, uint32_t>> ends;      // (text offset a member ends at, the CRC-32 its trailer holds)
    uint64_t text = 0, end_rel = 0;           // bytes of text; the bit the last accepted stretch ended on
    uint32_t isize_seg = 0, repairs = 0;
    bool ended = false, crc_lost = false;     // the stream ends here; a stretch passed more than one member end
    int fail = GZ_WALK_OK;                    // GZ_WALK_REPAIRS: too many / too large repairs; BAD, SHORT: what a decoder met
    uint64_t fail_bit = 0;                    // ... and where, in the buffer
    int device_rc = 0;                        // GZ_WALK_DEVICE: what decode_again returned
};
// results[j] answers plan.jobs[j]; decode_again(job, &result) decodes one job on the device, 0 for done
template <typename DecodeAgain>
static inline GzChain gz_walk_chain(const GzStarts &s, uint64_t n_bytes, const GzPlan &plan, const GzResult *results, DecodeAgain decode_again)
{
    const std::vector<uint64_t> &starts = s.starts;
    const uint64_t stop_rel = s.stop_rel, total_cap = plan.total_cap;
    GzChain c;
    uint64_t repair_used = 0;
    GzJob cur_job = plan.jobs[0];
    GzResult cur = results[0];
    auto accept = [&]() {                              // cur is part of the text
        c.v_off.push_back(cur_job.out_off); c.v_n.push_back(cur.n_out); c.v_base.push_back(c.text);
        if (cur.members >= 1) c.ends.emplace_back(c.text + cur.trailer_at, cur.trailer_crc);
        if (cur.members > 1) c.crc_lost = true;
        c.text += cur.n_out;
        c.isize_seg += cur.isize_sum;
    };
    auto failed = [&](int why, uint64_t bit) { c.fail = why; c.fail_bit = bit; return c; };
    for (;;) {
        // (The second condition cannot come from k_gz_decode as it is written: it reports GZ_LANDED only where gz_met_start matched
        // an entry of starts[] at or behind the job's target_idx, which is never 0, or at or behind terminal_bit = stop_rel.  The
        // arm is kept for a decoder that stops at any block boundary behind a start it ran over; tests reach it with a made-up result.)
        if (cur.status == GZ_FULL || (cur.status == GZ_LANDED && cur.end_bit < stop_rel && !std::binary_search(starts.begin() + 1, starts.end(), cur.end_bit))) {
            // out of room, or the stretch ran over a false start and stopped at a block nobody began at: decode again, from
            // this stretch's start (for room) or from where it stopped, as a stretch of its own
            GzJob again;
            if (cur.status == GZ_FULL) {
                if (cur_job.out_off >= total_cap) repair_used = cur_job.out_off - total_cap;        // the failed attempt's room is free again
                again = cur_job;
                again.out_cap = (uint32_t)std::min<uint64_t>((uint64_t)cur_job.out_cap * 32, GZ_MAX_CAP);
            } else {
                accept();
                again.start_bit = cur.end_bit;
                again.header_bit = cur.end_bit;
                const auto nx = std::upper_bound(starts.begin() + 1, starts.end(), cur.end_bit);
                again.target_idx = (uint64_t)(nx - starts.begin());
                const uint64_t next = nx == starts.end() ? n_bytes * 8 : *nx;
                again.out_cap = plan.room(next - again.start_bit);
            }
            again.pad = 0;
            again.out_off = total_cap + repair_used;
            repair_used += gz_round_up(again.out_cap, 64);
            if (++c.repairs > GZ_MAX_REPAIRS || repair_used > plan.repair_room || (cur.status == GZ_FULL && cur_job.out_cap >= GZ_MAX_CAP))
                return failed(GZ_WALK_REPAIRS, cur_job.start_bit);
            c.device_rc = decode_again(again, &cur);
            if (c.device_rc != 0) return failed(GZ_WALK_DEVICE, again.start_bit);
            cur_job = again;
            continue;
        }
        if (cur.status == GZ_BAD || cur.status == GZ_SHORT) return failed(cur.status == GZ_BAD ? GZ_WALK_BAD : GZ_WALK_SHORT, cur.end_bit);
        accept();
        c.end_rel = cur.end_bit;
        if (cur.status == GZ_END) { c.ended = true; break; }
        if (cur.end_bit >= stop_rel) break;
        const size_t k = (size_t)(std::lower_bound(starts.begin() + 1, starts.end(), cur.end_bit) - starts.begin());     // exists: checked above
        cur_job = plan.jobs[k];
        cur = results[k];
    }
    return c;
}

// ---- the text member by member (ends from the decoders), every member in slices of `slice` bytes for k_gz_crc: one thread
// each, joined on the host.  closes[r]: index into `ends` + 1 for the range that ends a member, else 0
struct GzCrcRanges {
    std::vector<uint64_t> start;
    std::vector<uint32_t> len, closes;
};
static inline GzCrcRanges gz_crc_ranges(uint64_t text, const std::vector<std::pair<uint64_t, uint32_t>> &ends, uint32_t slice)
{
    GzCrcRanges r;
    uint64_t at = 0;
    size_t e = 0;
    while (at < text || e < ends.size()) {
        const uint64_t stop = e < ends.size() ? ends[e].first : text;
        if (at == stop) {                          // a member that ends here without (more) text: an empty range closes it
            if (e >= ends.size()) break;
            r.start.push_back(at); r.len.push_back(0); r.closes.push_back((uint32_t)++e);
            continue;
        }
        const uint32_t n = (uint32_t)std::min<uint64_t>(stop - at, slice);
        r.start.push_back(at); r.len.push_back(n);
        at += n;
        r.closes.push_back(at == stop && e < ends.size() ? (uint32_t)++e : 0u);
    }
    return r;
}
