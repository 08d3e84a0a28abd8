// Host-side harness for kevlar_amd/csrc/kv_gunzip_plan.h (compiled as plain C++ by tests/test_gunzip_plan.py): the segment plan,
// the chain walk and the CRC ranges of the gzip decoder behind a C ABI, so that Python can compare them with a restatement of the
// rules and run the walk against a simulated decoder.  Vectors come back in caller-provided arrays of `cap` entries; every
// function returns (or reports) the full count, so a caller can tell that its arrays were too small.
#include <stdint.h>
#include <string.h>
#include "../../kevlar_amd/csrc/kv_gunzip_plan.h"

namespace {
GzStarts starts_of(const uint64_t *starts, const uint64_t *headers, uint64_t n, int have_terminal)
{
    GzStarts s;
    s.starts.assign(starts, starts + n);
    s.headers.assign(headers, headers + n);
    s.have_terminal = have_terminal != 0;
    s.stop_rel = s.have_terminal ? s.starts.back() : ~0ull;
    return s;
}
void put(const std::vector<uint64_t> &v, uint64_t *out, uint64_t cap)
{
    for (uint64_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
// out[0 .. 9]: GZ_FIND_KEEP, GZ_MARGIN, GZ_MAX_REPAIRS, GZ_MAX_CAP, the five statuses, sizeof(GzJob), then sizeof(GzGuess), sizeof(GzResult)
void h_gz_constants(uint64_t *out)
{
    const uint64_t c[12] = {GZ_FIND_KEEP, GZ_MARGIN, GZ_MAX_REPAIRS, GZ_MAX_CAP, GZ_LANDED, GZ_END, GZ_BAD, GZ_FULL, GZ_SHORT, sizeof(GzJob), sizeof(GzGuess), sizeof(GzResult)};
    memcpy(out, c, sizeof(c));
}

// out[0 .. 10]: first_byte, seg_end, upto, n_bytes, n_chunks, to_file_end, is_file_end, start_rel, seg_end_rel
void h_gz_extent(uint64_t pos_bit, uint64_t file_size, uint64_t want_text, double ratio, uint32_t chunk_bytes, uint64_t *out)
{
    const GzExtent x = gz_segment_extent(pos_bit, file_size, want_text, ratio, chunk_bytes);
    const uint64_t v[9] = {x.first_byte, x.seg_end, x.upto, x.n_bytes, x.n_chunks, x.to_file_end, x.is_file_end, x.start_rel, x.seg_end_rel};
    memcpy(out, v, sizeof(v));
}

// scalars[0 .. 2]: number of starts, have_terminal, stop_rel; returns 0 for "no block start within the margin"
int h_gz_starts(uint64_t pos_bit, uint64_t file_size, uint64_t want_text, double ratio, uint32_t chunk_bytes, const unsigned long long *cand, uint64_t n_cand,
                uint64_t *starts, uint64_t *headers, uint64_t cap, uint64_t *scalars)
{
    GzStarts s;
    const bool ok = gz_starts(gz_segment_extent(pos_bit, file_size, want_text, ratio, chunk_bytes), cand, n_cand, &s);
    put(s.starts, starts, cap);
    put(s.headers, headers, cap);
    scalars[0] = s.starts.size(); scalars[1] = s.have_terminal; scalars[2] = s.stop_rel;
    return ok ? 1 : 0;
}

// guesses: (header_bit, guess_bit) pairs; returns their number
uint64_t h_gz_guesses(uint64_t pos_bit, uint64_t file_size, uint64_t want_text, double ratio, uint32_t chunk_bytes, const uint64_t *starts, uint64_t n_starts,
                      int have_terminal, uint64_t wanted_stretches, uint64_t max_guesses, uint64_t *guesses, uint64_t cap)
{
    const std::vector<GzGuess> g = gz_cut_guesses(gz_segment_extent(pos_bit, file_size, want_text, ratio, chunk_bytes), starts_of(starts, starts, n_starts, have_terminal),
                                                  wanted_stretches, max_guesses);
    for (uint64_t i = 0; i < g.size() && i < cap; ++i) { guesses[2 * i] = g[i].header_bit; guesses[2 * i + 1] = g[i].guess_bit; }
    return g.size();
}

// the starts with the found boundaries merged in; *n_out = their number; returns the number of cuts taken
uint64_t h_gz_merge(const uint64_t *starts, uint64_t n_starts, int have_terminal, const uint64_t *guesses, const unsigned long long *found, uint64_t n_guesses,
                    uint64_t *starts_out, uint64_t *headers_out, uint64_t cap, uint64_t *n_out)
{
    GzStarts s = starts_of(starts, starts, n_starts, have_terminal);
    std::vector<GzGuess> g(n_guesses);
    for (uint64_t i = 0; i < n_guesses; ++i) { g[i].header_bit = guesses[2 * i]; g[i].guess_bit = guesses[2 * i + 1]; }
    const uint64_t taken = gz_merge_cuts(&s, g, found);
    put(s.starts, starts_out, cap);
    put(s.headers, headers_out, cap);
    *n_out = s.starts.size();
    return taken;
}

// scalars[0 .. 3]: number of jobs, total_cap, repair_room, exact
void h_gz_plan(const uint64_t *starts, const uint64_t *headers, uint64_t n_starts, int have_terminal, uint64_t n_bytes, double ratio, GzJob *jobs, uint64_t cap,
               uint64_t *scalars)
{
    const GzPlan p = gz_plan_jobs(starts_of(starts, headers, n_starts, have_terminal), n_bytes, ratio);
    for (uint64_t j = 0; j < p.jobs.size() && j < cap; ++j) jobs[j] = p.jobs[j];
    scalars[0] = p.jobs.size(); scalars[1] = p.total_cap; scalars[2] = p.repair_room; scalars[3] = p.exact;
}

uint32_t h_gz_room(double ratio, uint64_t bits)
{
    GzPlan p;
    p.factor = std::min(std::max(2.5 * ratio, 8.0), 64.0);
    return p.room(bits);
}

// The walk over the plan of these starts; `decode` answers every job, those of the first launch (in order) and then each repair.
// v: (out_off, n_out, text base) per accepted stretch; ends: (text offset, crc) per member end.
// scalars[0 .. 10]: accepted stretches, member ends, text, end_rel, isize_seg, repairs, ended, crc_lost, fail, fail_bit, device_rc
void h_gz_walk(const uint64_t *starts, const uint64_t *headers, uint64_t n_starts, int have_terminal, uint64_t n_bytes, double ratio,
               int (*decode)(const GzJob *, GzResult *), uint64_t *v, uint64_t v_cap, uint64_t *ends, uint64_t ends_cap, uint64_t *scalars)
{
    const GzStarts s = starts_of(starts, headers, n_starts, have_terminal);
    const GzPlan p = gz_plan_jobs(s, n_bytes, ratio);
    std::vector<GzResult> results(p.jobs.size());
    for (size_t j = 0; j < p.jobs.size(); ++j) decode(&p.jobs[j], &results[j]);
    const GzChain c = gz_walk_chain(s, n_bytes, p, results.data(), [decode](const GzJob &job, GzResult *out) { return decode(&job, out); });
    for (uint64_t i = 0; i < c.v_off.size() && i < v_cap; ++i) { v[3 * i] = c.v_off[i]; v[3 * i + 1] = c.v_n[i]; v[3 * i + 2] = c.v_base[i]; }
    for (uint64_t i = 0; i < c.ends.size() && i < ends_cap; ++i) { ends[2 * i] = c.ends[i].first; ends[2 * i + 1] = c.ends[i].second; }
    const uint64_t out[11] = {c.v_off.size(), c.ends.size(), c.text, c.end_rel, c.isize_seg, c.repairs, c.ended, c.crc_lost, (uint64_t)c.fail, c.fail_bit, (uint64_t)c.device_rc};
    memcpy(scalars, out, sizeof(out));
}

// ranges: (start, len, closes) each; returns their number
uint64_t h_gz_crc_ranges(uint64_t text, const uint64_t *end_at, uint64_t n_ends, uint32_t slice, uint64_t *ranges, uint64_t cap)
{
    std::vector<std::pair<uint64_t, uint32_t>> ends;
    for (uint64_t i = 0; i < n_ends; ++i) ends.emplace_back(end_at[i], 0u);
    const GzCrcRanges r = gz_crc_ranges(text, ends, slice);
    for (uint64_t i = 0; i < r.start.size() && i < cap; ++i) { ranges[3 * i] = r.start[i]; ranges[3 * i + 1] = r.len[i]; ranges[3 * i + 2] = r.closes[i]; }
    return r.start.size();
}
}
