// kv_genome_plan.h -- the host rules of the device FASTA splitter (kv_genome.hip), free of HIP: the byte classes, what one line
// contributes, what travels from one pass over the text (a segment) to the next, how the input is cut into segments, how the
// joined text's buffer grows and how a resident genome is cut into scan chunks.  The per-line rule is marked GN_HD: the kernels
// of kv_genome.hip call the same functions, and gn_model_segment() below runs them a line at a time on the host, so a CPU test
// can cut a file anywhere and compare with the parser it replaces.  Plain C++17: tests/harness/genome_plan_host.cpp compiles it
// for the host, tests/test_genome_reference.py checks the edges.
//
// The rule on bytes: lines end at LF; a line is taken without its trailing run of space, TAB, VT, FF and
// CR; a line whose first byte is '>' is a defline and its id the bytes behind the '>' up to the first space or TAB; the stripped
// lines between two deflines, concatenated, are a record's sequence; text in front of the first defline is nothing.  The joined
// text is the sequences in file order with one GN_SEPARATOR between neighbours.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kvsketch.h"
#include "kv_require.h"

#if defined(__HIPCC__)
#define GN_HD __host__ __device__ __forceinline__
#else
#define GN_HD static inline
#endif

#define GN_CHUNK 16384u                      // bytes of text per workgroup of the line and copy kernels
#define GN_THREADS 256
#define GN_MAX_TRAIL 4096u                   // longest run of strippable bytes at a line end (or at a segment end) that is followed; a longer one declines
#define GN_MAX_ID 4096u                      // longest stretch of id bytes one line part may hold; a longer one declines
#define GN_SEGMENT_DEFAULT (256ull << 20)    // text bytes per pass when the caller names none
#define GN_SEGMENT_MAX (1ull << 30)          // (a line part's length is a 32-bit count)
#define GN_SEPARATOR 0x3eu                   // '>' between two sequences of the joined text: kevlar_amd.localize.SEPARATOR

// what a line (part) contributes
enum { GN_NONE = 0, GN_SEQ = 1, GN_ID = 2 };

// why a file is not for the device, and GN_F_CR_LAST: the segment's last byte is a CR (a decline only when the file ends there)
#define GN_F_HIGH 1u            // a byte >= 0x80: the text layer decodes it
#define GN_F_SEP 2u             // 0x1c-0x1f: str.rstrip() strips them too
#define GN_F_NUL 4u
#define GN_F_CR 8u              // a CR not followed by LF: universal newlines would end a line there
#define GN_F_TRAIL 16u          // more than GN_MAX_TRAIL strippable bytes on end
#define GN_F_IDLEN 32u          // more than GN_MAX_ID id bytes in one line part
#define GN_F_CR_LAST 64u
#define GN_F_DECLINE (GN_F_HIGH | GN_F_SEP | GN_F_NUL | GN_F_CR | GN_F_TRAIL | GN_F_IDLEN)

// space, TAB, VT, FF, CR: what str.rstrip() takes off a line among the bytes the device accepts (LF ends the line)
GN_HD bool gn_is_strip(uint32_t c) { return c == 0x20u || c == 0x09u || (c - 0x0bu) <= 2u; }
GN_HD bool gn_ends_id(uint32_t c) { return c == 0x20u || c == 0x09u; }
// the decline flag of one byte (CR is judged with its successor: gn_cr_flag)
GN_HD uint32_t gn_byte_flags(uint32_t c)
{
    return (c >= 0x80u ? GN_F_HIGH : 0u) | ((c - 0x1cu) <= 3u ? GN_F_SEP : 0u) | (c == 0u ? GN_F_NUL : 0u);
}
// a CR at byte i of n: fine in front of LF, GN_F_CR_LAST as the segment's last byte, else a decline
GN_HD uint32_t gn_cr_flag(bool has_next, uint32_t next) { return !has_next ? GN_F_CR_LAST : next == 0x0au ? 0u : GN_F_CR; }

struct GnLine {
    uint32_t kind;        // GN_NONE / GN_SEQ / GN_ID: where the payload goes
    uint32_t pay_off;     // the payload begins this many bytes behind the line (part)'s first byte
    uint32_t pay_len;
    uint32_t is_def;      // a defline BEGINS here: one more record
    uint32_t defline;     // the line (part) belongs to a defline
    uint32_t id_open;     // ... whose id has not met its blank yet
    uint32_t held;        // strippable bytes on end (what a segment's last line holds back)
    uint32_t flags;       // GN_F_TRAIL / GN_F_IDLEN
};

// One line (part): raw bytes text[a, b), the LF not among them.  cont: the line began in an earlier segment, as a defline
// (cont_def) whose id was still open (cont_id) or as something else.  A lane walks at most GN_MAX_TRAIL + 1 bytes backwards and
// GN_MAX_ID + 1 forwards, however long the line is.
template <typename Text>
GN_HD GnLine gn_classify(const Text text, uint64_t a, uint64_t b, bool cont, bool cont_def, bool cont_id)
{
    GnLine r;
    r.kind = GN_NONE; r.pay_off = 0; r.pay_len = 0; r.is_def = 0; r.defline = 0; r.id_open = 0; r.flags = 0;
    uint64_t e = b;
    while (e > a && b - e <= GN_MAX_TRAIL && gn_is_strip(text[e - 1])) --e;
    if (b - e > GN_MAX_TRAIL) r.flags |= GN_F_TRAIL;
    r.held = (uint32_t)(b - e);
    const bool fresh_def = !cont && b > a && text[a] == '>';
    if (fresh_def || (cont && cont_def)) {
        r.is_def = fresh_def ? 1u : 0u;
        r.defline = 1;
        if (fresh_def || cont_id) {
            const uint64_t i0 = a + (fresh_def ? 1u : 0u);
            uint64_t i = i0;
            while (i < e && i - i0 <= GN_MAX_ID && !gn_ends_id(text[i])) ++i;
            if (i - i0 > GN_MAX_ID) r.flags |= GN_F_IDLEN;
            r.kind = GN_ID;
            r.pay_off = (uint32_t)(i0 - a);
            r.pay_len = (uint32_t)(i - i0);
            r.id_open = i == e ? 1u : 0u;
        }
    } else {
        r.kind = GN_SEQ;
        r.pay_len = (uint32_t)(e - a);
    }
    return r;
}

// bytes of joined text a line owns, given the records begun in front of it (all segments): a defline owns the separator in front
// of its record, unless the record is the genome's first; a sequence line owns its payload once a defline has been seen
GN_HD uint32_t gn_out_bytes(uint32_t kind, uint32_t is_def, uint32_t pay_len, uint64_t records_before)
{
    if (is_def) return records_before > 0 ? 1u : 0u;
    return kind == GN_SEQ && records_before > 0 ? pay_len : 0u;
}

// what travels from one segment to the next
struct GnCarry {
    uint32_t mid_line = 0;      // the segment ended inside a line
    uint32_t mid_defline = 0;   // ... a defline
    uint32_t id_open = 0;       // ... whose id may go on
    uint32_t held = 0;          // strippable bytes at the segment's end, held back: they come again in front of the next segment,
                                // where they are interior if payload follows and dropped if LF (or the end of the file) does
    uint32_t cr_last = 0;       // the last byte seen is a CR
    uint64_t out_off = 0;       // joined text so far
    uint64_t id_off = 0;        // id bytes so far
    uint64_t n_records = 0;
    uint64_t text_seen = 0;     // bytes of the file's text consumed (the held ones not counted twice)
};

// what a pass over one segment found: n bytes (the held ones in front included)
struct GnSegmentResult {
    uint64_t n = 0;
    uint64_t last_raw = 0;      // raw length of the segment's last line (part)
    uint32_t last_defline = 0, last_id_open = 0, last_held = 0;
    uint32_t flags = 0;
    uint64_t n_defs = 0, id_bytes = 0, out_bytes = 0;
};

// the carry behind a segment, or KV_ERR_TYPE with the reason when the file is not for the device
inline int gn_carry_next(GnCarry &c, const GnSegmentResult &s)
{
    KV_REQUIRE(!(s.flags & GN_F_HIGH), KV_ERR_TYPE, "reference FASTA: a byte >= 0x80 (read on the host)");
    KV_REQUIRE(!(s.flags & GN_F_SEP), KV_ERR_TYPE, "reference FASTA: one of the bytes 0x1c-0x1f (read on the host)");
    KV_REQUIRE(!(s.flags & GN_F_NUL), KV_ERR_TYPE, "reference FASTA: a NUL byte (read on the host)");
    KV_REQUIRE(!(s.flags & GN_F_CR), KV_ERR_TYPE, "reference FASTA: a CR that no LF follows (read on the host)");
    KV_REQUIRE(!(s.flags & GN_F_TRAIL), KV_ERR_TYPE, "reference FASTA: more than %u blanks at a line end (read on the host)", GN_MAX_TRAIL);
    KV_REQUIRE(!(s.flags & GN_F_IDLEN), KV_ERR_TYPE, "reference FASTA: a sequence id of more than %u bytes (read on the host)", GN_MAX_ID);
    KV_REQUIRE(s.n >= c.held && s.last_held <= s.last_raw && s.last_raw <= s.n, KV_ERR_ARG, "gn_carry_next: impossible segment result");
    c.text_seen += s.n - c.held;
    c.mid_line = s.last_raw > 0 ? 1u : 0u;
    c.mid_defline = c.mid_line ? s.last_defline : 0u;
    c.id_open = c.mid_defline ? s.last_id_open : 0u;
    c.held = c.mid_line ? s.last_held : 0u;
    c.cr_last = (s.flags & GN_F_CR_LAST) ? 1u : 0u;
    c.out_off += s.out_bytes;
    c.id_off += s.id_bytes;
    c.n_records += s.n_defs;
    return KV_OK;
}

// the file has ended: held bytes are dropped, but a CR on the very end would have been a line end of its own
inline int gn_carry_finish(const GnCarry &c)
{
    KV_REQUIRE(!c.cr_last, KV_ERR_TYPE, "reference FASTA: a CR that no LF follows (read on the host)");
    return KV_OK;
}

// text bytes per pass
inline uint64_t gn_segment_text(uint64_t asked) { return asked == 0 ? GN_SEGMENT_DEFAULT : asked > GN_SEGMENT_MAX ? GN_SEGMENT_MAX : asked; }
// fresh bytes of an uncompressed file's next segment
inline uint64_t gn_plain_take(uint64_t pos, uint64_t size, uint64_t segment) { return size - pos < segment ? size - pos : segment; }
// members [m0, m1) of a blocked gzip file's next segment: whole members while they fit, one at least
inline uint64_t gn_bgzf_take(const uint32_t *isize, uint64_t n_members, uint64_t m0, uint64_t segment, uint64_t *text_bytes)
{
    uint64_t m1 = m0, n = 0;
    while (m1 < n_members && (m1 == m0 || n + isize[m1] <= segment)) n += isize[m1++];
    *text_bytes = n;
    return m1;
}
// the joined text never outgrows the file's text (a record's separator is paid for by its '>'), so a file of known text size gets
// its buffer once; a gzip stream's grows by doubling
inline uint64_t gn_grow(uint64_t cap, uint64_t need)
{
    uint64_t c = cap < 4096 ? 4096 : cap;
    while (c < need) c *= 2;
    return c;
}

// Scan chunks of a resident text of `total` bytes for seeds of length z: chunk k holds the windows that start in
// [k * step, (k + 1) * step), so it is step + z - 1 bytes long (the text's end cuts the last).  step = chunk_bytes - (z - 1) as for
// an uploaded text, rounded down to a multiple of 16 where that leaves one: such chunks begin on the 16-byte boundaries the scan
// kernel loads from and are scanned where they lie; others are copied to an aligned buffer first.  chunk_bytes 0: the whole text.
struct GnScanPlan { uint64_t step, len, n_chunks; };
inline GnScanPlan gn_scan_plan(uint64_t total, uint64_t z, uint64_t chunk_bytes)
{
    GnScanPlan p;
    if (chunk_bytes == 0 || chunk_bytes >= total) {
        p.step = p.len = total;
        p.n_chunks = total < z ? 0 : 1;
        return p;
    }
    if (chunk_bytes < z) chunk_bytes = z;
    p.step = chunk_bytes - (z - 1);
    if (p.step >= 16) p.step &= ~15ull;
    p.len = p.step + z - 1;
    p.n_chunks = total < z ? 0 : (total - z + 1 + p.step - 1) / p.step;
    return p;
}

// ---- the splitter a line at a time, on the host: what the kernels compute for one segment, in the same steps ------------------
struct GnModel {
    GnCarry carry;
    std::string held;                    // the bytes held back
    std::string text, ids;               // joined text, id blob
    std::vector<uint64_t> seq_start, id_off;     // per record
};

inline uint32_t gn_check_bytes(const uint8_t *t, uint64_t n)
{
    uint32_t flags = 0;
    for (uint64_t i = 0; i < n; ++i) {
        flags |= gn_byte_flags(t[i]);
        if (t[i] == 0x0du) flags |= gn_cr_flag(i + 1 < n, i + 1 < n ? t[i + 1] : 0u);
    }
    return flags;
}

// one segment of `n_fresh` bytes behind the held ones
inline int gn_model_segment(GnModel &m, const uint8_t *fresh, uint64_t n_fresh)
{
    std::string seg = m.held;
    seg.append((const char *)fresh, (size_t)n_fresh);
    const uint8_t *t = (const uint8_t *)seg.data();
    const uint64_t n = seg.size();
    GnSegmentResult s;
    s.n = n;
    s.flags = gn_check_bytes(t, n);
    uint64_t a = 0, line = 0;
    for (;;) {
        uint64_t b = a;
        while (b < n && t[b] != 0x0au) ++b;
        const bool cont = line == 0 && m.carry.mid_line;
        const GnLine l = gn_classify(t, a, b, cont, cont && m.carry.mid_defline, cont && m.carry.id_open);
        s.flags |= l.flags;
        const uint64_t before = m.carry.n_records + s.n_defs;
        const uint32_t out = gn_out_bytes(l.kind, l.is_def, l.pay_len, before);
        if (l.is_def) {
            if (out) m.text.push_back((char)GN_SEPARATOR);
            m.seq_start.push_back(m.text.size());
            m.id_off.push_back(m.ids.size());
            ++s.n_defs;
        } else if (out) m.text.append((const char *)t + a + l.pay_off, l.pay_len);
        if (l.kind == GN_ID) { m.ids.append((const char *)t + a + l.pay_off, l.pay_len); s.id_bytes += l.pay_len; }
        s.out_bytes += out;
        if (b == n) { s.last_raw = b - a; s.last_defline = l.defline; s.last_id_open = l.id_open; s.last_held = l.held; break; }
        a = b + 1;
        ++line;
    }
    // (the last line's payload ends in front of the bytes it holds back: gn_classify left them out of pay_len)
    KV_STEP(gn_carry_next(m.carry, s));
    m.held.assign(seg, (size_t)(n - m.carry.held), (size_t)m.carry.held);
    return KV_OK;
}
