// Host-side harness for kevlar_amd/csrc/kv_genome_plan.h (compiled as plain C++ by tests/test_genome_reference.py): the byte
// classes, the per-line rule, the carry from one segment to the next (through gn_model_segment, which runs the kernels' steps a
// line at a time), the segment takes, the buffer growth and the scan chunks behind a C ABI, so that Python can cut a file anywhere
// and compare with the parser the device replaces.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../kevlar_amd/csrc/kv_genome_plan.h"

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
    const uint64_t c[8] = {GN_CHUNK, GN_THREADS, GN_MAX_TRAIL, GN_MAX_ID, GN_SEGMENT_DEFAULT, GN_SEGMENT_MAX, GN_SEPARATOR, GN_F_DECLINE};
    memcpy(out, c, sizeof(c));
}

int h_is_strip(uint32_t c) { return gn_is_strip(c); }
int h_ends_id(uint32_t c) { return gn_ends_id(c); }
uint32_t h_byte_flags(uint32_t c) { return gn_byte_flags(c); }
uint32_t h_check_bytes(const uint8_t *t, uint64_t n) { return gn_check_bytes(t, n); }

// out[0..7] = kind, pay_off, pay_len, is_def, defline, id_open, held, flags
void h_classify(const uint8_t *text, uint64_t a, uint64_t b, int cont, int cont_def, int cont_id, uint32_t *out)
{
    const GnLine l = gn_classify(text, a, b, cont != 0, cont_def != 0, cont_id != 0);
    const uint32_t v[8] = {l.kind, l.pay_off, l.pay_len, l.is_def, l.defline, l.id_open, l.held, l.flags};
    memcpy(out, v, sizeof(v));
}

uint32_t h_out_bytes(uint32_t kind, uint32_t is_def, uint32_t pay_len, uint64_t records_before) { return gn_out_bytes(kind, is_def, pay_len, records_before); }

// The file data[0, n) in segments that end at cuts[0] < cuts[1] < ... (and at n).  Returns the KV_* code; on KV_OK text_out (room
// for n bytes) and ids_out (room for n) are filled, seq_start / id_off hold one entry per record (room for n + 1), scalars[0..5] =
// text bytes, id bytes, records, text seen, segments, the most bytes held back.
int h_model(const uint8_t *data, uint64_t n, const uint64_t *cuts, uint64_t n_cuts, uint8_t *text_out, uint8_t *ids_out, uint64_t *seq_start,
            uint64_t *id_off, uint64_t *scalars)
{
    g_error[0] = 0;
    GnModel m;
    uint64_t at = 0, segments = 0, most_held = 0;
    for (uint64_t k = 0; k <= n_cuts; ++k) {
        const uint64_t end = k < n_cuts ? cuts[k] : n;
        if (end == at && !(k == n_cuts && n == 0)) continue;
        if (end == at) break;
        KV_STEP(gn_model_segment(m, data + at, end - at));
        most_held = m.carry.held > most_held ? m.carry.held : most_held;
        at = end;
        ++segments;
    }
    KV_STEP(gn_carry_finish(m.carry));
    KV_REQUIRE(m.text.size() == m.carry.out_off && m.ids.size() == m.carry.id_off && m.seq_start.size() == m.carry.n_records, KV_ERR_ARG,
               "the model's carry and its output disagree");
    memcpy(text_out, m.text.data(), m.text.size());
    memcpy(ids_out, m.ids.data(), m.ids.size());
    for (size_t r = 0; r < m.seq_start.size(); ++r) { seq_start[r] = m.seq_start[r]; id_off[r] = m.id_off[r]; }
    scalars[0] = m.text.size(); scalars[1] = m.ids.size(); scalars[2] = m.carry.n_records; scalars[3] = m.carry.text_seen; scalars[4] = segments;
    scalars[5] = most_held;
    return KV_OK;
}

uint64_t h_segment_text(uint64_t asked) { return gn_segment_text(asked); }
uint64_t h_plain_take(uint64_t pos, uint64_t size, uint64_t segment) { return gn_plain_take(pos, size, segment); }
uint64_t h_bgzf_take(const uint32_t *isize, uint64_t n_members, uint64_t m0, uint64_t segment, uint64_t *text_bytes)
{
    return gn_bgzf_take(isize, n_members, m0, segment, text_bytes);
}
uint64_t h_grow(uint64_t cap, uint64_t need) { return gn_grow(cap, need); }
void h_scan_plan(uint64_t total, uint64_t z, uint64_t chunk_bytes, uint64_t *out)
{
    const GnScanPlan p = gn_scan_plan(total, z, chunk_bytes);
    out[0] = p.step; out[1] = p.len; out[2] = p.n_chunks;
}
}
