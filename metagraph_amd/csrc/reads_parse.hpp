// reads_parse.hpp — FASTA / FASTQ text to the read arrays of mgx_align_batch (seqs, offsets) and the name arrays of
// mgx_format_tsv_batch (names, name_offsets), without a per-record step on the host (host side: mgx_parse_reads in
// mgx_parse.hip; DESIGN 3.12 states the grammar).
//
// Written against the wave interface (wave.hpp): tests/test_reads_parse_model.py compiles this very file for the host
// (tests/emu/wave.hpp) and compares its arrays with a restatement of the grammar.  Every function below is the work of one
// lane; the passes, in order (a scan by the caller between them):
//   line    rp_line_count: a lane reads a span of RP_SPAN bytes as four 16-byte loads, keeps the span's '\n' positions as a
//           64-bit mask and their number.  [scan of the numbers]  rp_line_table: a lane turns its mask into entries of
//           line_begin[] — the text is not read again.
//   class   rp_classify: a lane per line: header / sequence / ignored, payload and name lengths, the grammar's checks (the
//           smallest offending line begin: an atomic min on one word).  [scan of (sequence bytes, name bytes, headers)]
//           rp_records: a lane per line: offsets[r] / name_offsets[r] at every header line, and the end of what this chunk
//           consumes (complete records only unless the chunk is final).
//   copy    rp_copy16: a lane per 16 destination bytes (work is split by bytes: a 5 Mbp line is 300 000 lanes' work): a
//           binary search over the scanned table, between two lines the caller knows to bracket it (the kernel: found once
//           per wavefront), finds the line of its first byte; the 16 bytes are re-aligned from aligned dword loads of the
//           source and leave as one aligned 16-byte store.  Pieces that span lines are put together byte by byte.
#pragma once
#include "wave.hpp"

namespace mgx {

enum : uint32_t { RP_FASTA = 1, RP_FASTQ = 2 };
constexpr uint32_t RP_SPAN = 64;
constexpr uint32_t RP_NO_ERROR = 0xFFFFFFFFu;

// what a line adds: sequence bytes, name bytes, records (1 at a header line); after the exclusive scan: what lies in front of it
struct alignas(16) RpSum { uint64_t seq; uint32_t name, rec; };

struct RpCounters {
    uint32_t err_pos;           // begin of the first line that breaks the grammar (atomic min; RP_NO_ERROR: none)
    uint32_t last_nonempty;     // 1 + the index of the last line with a payload (atomic max of rp_classify's values)
    uint32_t trunc_pos;         // FASTQ: begin of the first line behind the last whole group of four lines
    uint32_t pad;
    uint64_t consumed;          // bytes of the records handed out (the begin of the first line that is not theirs)
    uint64_t n_records, seq_bytes, name_bytes;
};

struct RpChunk {
    const char *text;           // n bytes, n < 2^32
    uint64_t n;
    uint32_t mis;               // text's address & 15: span s holds positions 64 s - mis .. 64 s - mis + 63
    uint32_t n_spans;
    uint64_t *mask;             // n_spans
    uint32_t *span_count;       // n_spans (+ a closing 0 for the scan)
    const uint32_t *span_first; // the scan of span_count
    uint32_t *line_begin;       // line i = text[line_begin[i] .. line_begin[i + 1] - 1); n_lines + 1 entries (an unterminated last line ends at n: entry n + 1)
    uint32_t n_lines;           // the lines this parse looks at (an unterminated last line only in a final chunk)
    uint32_t format;            // RP_FASTA / RP_FASTQ
    uint32_t final_chunk, pad;
    RpSum *items;               // n_lines + 1 (the last one zero): rp_classify
    const RpSum *sums;          // the exclusive scan of items
    RpCounters *ctr;
    uint64_t *offsets, *name_offsets;
    char *seqs, *names;         // 16-byte aligned, 16 bytes of room behind seq_bytes / name_bytes
    uint64_t seq_bytes, name_bytes;
};

// ---- line pass -------------------------------------------------------------------------------------------------------------
// bit x of the result: byte x of w is '\n' (exact zero-byte test, no carry crosses a byte; the multiply gathers the four bits)
MGX_DEV uint32_t rp_newlines4(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);       // 0x80 in every zero byte of x
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

MGX_DEV uint64_t rp_span_mask(const RpChunk &c, uint32_t s) {
    const int64_t p0 = (int64_t)s * RP_SPAN - (int64_t)c.mis;
    uint64_t m = 0;
    if (p0 >= 0 && (uint64_t)p0 + RP_SPAN <= c.n) {
        const uint4 *q = reinterpret_cast<const uint4 *>(c.text + p0);
        for (int x = 0; x < 4; ++x) {
            const uint4 v = gld(q + x);
            const uint32_t b = rp_newlines4(v.x) | rp_newlines4(v.y) << 4 | rp_newlines4(v.z) << 8 | rp_newlines4(v.w) << 12;
            m |= (uint64_t)b << (16 * x);
        }
    } else {
        for (uint32_t j = 0; j < RP_SPAN; ++j) {
            const int64_t p = p0 + j;
            if (p >= 0 && (uint64_t)p < c.n && gld(c.text + p) == '\n') m |= 1ull << j;
        }
    }
    return m;
}

MGX_DEV void rp_line_count(const RpChunk &c, uint32_t s) {
    const uint64_t m = rp_span_mask(c, s);
    gst(c.mask + s, m);
    gst(c.span_count + s, (uint32_t)popc64(m));
}

MGX_DEV void rp_line_table(const RpChunk &c, uint32_t s) {
    uint64_t m = gld(c.mask + s);
    uint32_t at = gld(c.span_first + s);
    if (s == 0) gst(c.line_begin, 0u);
    while (m) {
        const int j = ctz64(m);
        m &= m - 1;
        gst(c.line_begin + ++at, (uint32_t)((uint64_t)s * RP_SPAN + (uint32_t)j - c.mis + 1u));
    }
    // what ends an unterminated last line: as if a '\n' stood at text[n] (n < 2^32 - 1 keeps n + 1 in the word)
    if (s + 1 == c.n_spans) gst(c.line_begin + at + 1, (uint32_t)(c.n + 1));
}

// ---- classify --------------------------------------------------------------------------------------------------------------
MGX_DEV void rp_error(const RpChunk &c, uint32_t pos) {
#if MGX_WAVE_EMU
    if (pos < c.ctr->err_pos) c.ctr->err_pos = pos;
#else
    atomicMin(&c.ctr->err_pos, pos);
#endif
}

// line i without its '\n' and without a '\r' directly in front of that
MGX_DEV void rp_line(const RpChunk &c, uint32_t i, uint32_t *b, uint32_t *e) {
    *b = gld(c.line_begin + i);
    *e = gld(c.line_begin + i + 1) - 1u;
    if (*e < c.n && *e > *b && gld(c.text + *e - 1) == '\r') --*e;
}

MGX_DEV bool rp_isspace(char ch) { const uint8_t u = (uint8_t)ch; return u == ' ' || (u >= 9 && u <= 13); }

MGX_DEV uint32_t rp_name_len(const RpChunk &c, uint32_t b, uint32_t e) {
    uint32_t p = b + 1;
    while (p < e && !rp_isspace(gld(c.text + p))) ++p;
    return p - (b + 1);
}

// -> i + 1 if line i has a payload, else 0: the caller keeps the maximum in ctr->last_nonempty (one atomic per wavefront)
MGX_DEV uint32_t rp_classify(const RpChunk &c, uint32_t i) {
    RpSum it = { 0, 0, 0 };
    uint32_t nonempty = 0;
    if (i < c.n_lines) {
        uint32_t b, e;
        rp_line(c, i, &b, &e);
        const uint32_t len = e - b;
        const char c0 = len ? gld(c.text + b) : (char)0;
        if (len) nonempty = i + 1;
        if (c.format == RP_FASTA) {
            if (c0 == '>') { it.rec = 1; it.name = rp_name_len(c, b, e); }
            else if (len) {
                it.seq = len;
                if (c0 == '@' || c0 == '+') rp_error(c, b);                  // kseq would end the record here
            }
        } else {
            switch (i & 3u) {
            case 0:
                if (c0 == '@') { it.rec = 1; it.name = rp_name_len(c, b, e); } else rp_error(c, b);
                break;
            case 1:
                if (c0 == '@' || c0 == '+' || c0 == '>') rp_error(c, b);
                it.seq = len;
                if (i + 2 < c.n_lines) {
                    uint32_t qb, qe;
                    rp_line(c, i + 2, &qb, &qe);
                    if (qe - qb != len) rp_error(c, qb);
                }
                break;
            case 2:
                if (c0 != '+') rp_error(c, b);
                break;
            default: break;
            }
        }
    }
    gst(c.items + i, it);
    return nonempty;
}

// ---- records: lanes 0 .. n_lines ------------------------------------------------------------------------------------------
MGX_DEV void rp_records(const RpChunk &c, uint32_t i) {
    const uint64_t seq = gld(&c.sums[i].seq);
    const uint32_t name = gld(&c.sums[i].name), rec = gld(&c.sums[i].rec);
    const uint32_t n_rec = gld(&c.sums[c.n_lines].rec);
    const bool header = i < c.n_lines && gld(&c.sums[i + 1].rec) != rec;
    bool end;
    if (c.format == RP_FASTQ) {
        // whole groups of four lines, up to the one with the last non-empty line: empty lines behind it are nobody's
        const uint32_t groups = c.n_lines >> 2, used = (gld(&c.ctr->last_nonempty) + 3u) >> 2;
        end = i == 4u * (used < groups ? used : groups);
        if (i == 4u * groups) gst(&c.ctr->trunc_pos, gld(c.line_begin + i));
    } else {
        // sequence in front of the first header (a forced format): not a record's
        if (i < c.n_lines && !header && rec == 0 && gld(&c.sums[i + 1].seq) != seq) rp_error(c, gld(c.line_begin + i));
        // a record is complete when another header line follows it; in a final chunk the last one is, too
        end = c.final_chunk ? i == c.n_lines : (header && rec + 1 == n_rec);
    }
    // offsets[r] at record r's header line; offsets[n_records] at the end line (in a refused or unfinished tail it need not be a header)
    if (header || end || i == 0) { gst(c.offsets + rec, seq); gst(c.name_offsets + rec, (uint64_t)name); }
    if (end) {
        const uint64_t at = gld(c.line_begin + i);
        gst(&c.ctr->consumed, at < c.n ? at : c.n);
        gst(&c.ctr->n_records, (uint64_t)rec); gst(&c.ctr->seq_bytes, seq); gst(&c.ctr->name_bytes, (uint64_t)name);
    }
}

// ---- copy: destination bytes 16 t .. 16 t + 15 of the sequences (field 0) or the names (field 1) -------------------------
template <int FIELD>
MGX_DEV uint64_t rp_key(const RpChunk &c, uint32_t line) {
    if constexpr (FIELD) return gld(&c.sums[line].name); else return gld(&c.sums[line].seq);
}

// the line of byte d among lines lo .. hi - 1, given key(lo) <= d < key(hi): the last one with key(line) <= d
template <int FIELD>
MGX_DEV uint32_t rp_find_line(const RpChunk &c, uint64_t d, uint32_t lo, uint32_t hi) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rp_key<FIELD>(c, mid) <= d) lo = mid; else hi = mid;
    }
    return lo;
}

// what lanes 0 and 63 of a wavefront look up for all of its lanes: the line of the first byte of lane 0 (t_first) and of lane 63
// (or of the field's last byte, if that comes first)
template <int FIELD>
MGX_DEV uint32_t rp_wave_line(const RpChunk &c, uint64_t t_first, bool last) {
    const uint64_t limit = FIELD ? c.name_bytes : c.seq_bytes, d_last = 16 * (t_first + 63);
    return rp_find_line<FIELD>(c, last ? (d_last < limit ? d_last : limit - 1) : 16 * t_first, 0, c.n_lines);
}

// lo, hi: lines known to bracket byte 16 t (key(lo) <= 16 t < key(hi)); 0 and n_lines always do (key(0) = 0, 16 t < limit <= key(n_lines)).
// k_parse_copy narrows them per wavefront, so that the search over the whole table runs once per 1 KB and not once per 16 bytes.
template <int FIELD>
MGX_DEV void rp_copy16(const RpChunk &c, uint64_t t, uint32_t lo, uint32_t hi) {
    const uint64_t limit = FIELD ? c.name_bytes : c.seq_bytes, d = 16 * t;
    lo = rp_find_line<FIELD>(c, d, lo, hi);
    uint32_t line = lo;
    uint64_t k0 = rp_key<FIELD>(c, line), k1 = rp_key<FIELD>(c, line + 1);
    uint32_t w[4] = { 0, 0, 0, 0 };
    if (d + 16 <= k1 && d + 16 <= limit) {
        const char *s = c.text + gld(c.line_begin + line) + FIELD + (d - k0);
        const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
        const uint32_t *sa = reinterpret_cast<const uint32_t *>(s - sh);
        uint32_t a = gld(sa);
        for (int x = 0; x < 4; ++x) {
            if (sh) {
                const uint32_t nx = gld(sa + x + 1);
                w[x] = (uint32_t)((((uint64_t)nx << 32) | a) >> (8u * sh));
                a = nx;
            } else {
                w[x] = a;
                if (x < 3) a = gld(sa + x + 1);
            }
        }
    } else {
        for (uint32_t j = 0; j < 16; ++j) {
            const uint64_t pos = d + j;
            if (pos >= limit) break;
            while (k1 <= pos) { ++line; k0 = k1; k1 = rp_key<FIELD>(c, line + 1); }
            const uint8_t ch = (uint8_t)gld(c.text + gld(c.line_begin + line) + FIELD + (pos - k0));
            w[j >> 2] |= (uint32_t)ch << (8u * (j & 3u));
        }
    }
    uint4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    gst(reinterpret_cast<uint4 *>((FIELD ? c.names : c.seqs) + d), v);
}

// a sub-batch's offsets, starting at 0: lanes 0 .. n
MGX_DEV void rp_rebase(const uint64_t *offsets, uint64_t first, uint64_t *out, uint64_t i) {
    gst(out + i, gld(offsets + first + i) - gld(offsets + first));
}

// ---- host side of a parse (shared with the test's host model) ---------------------------------------------------------------
// The format: the first byte of the first non-empty line ('>' FASTA, '@' FASTQ).  at(p) = text[p].
// -> RP_FASTA / RP_FASTQ, 0 (no non-empty line yet) or -1 (another byte; *pos = the line's begin)
template <class At>
inline int rp_detect_format(At at, uint64_t n, bool final_chunk, uint64_t *pos) {
    uint64_t p = 0;
    while (p < n) {
        const char ch = at(p);
        if (ch == '\n') { ++p; continue; }
        if (ch == '\r' && p + 1 < n && at(p + 1) == '\n') { p += 2; continue; }
        if (ch == '\r' && p + 1 == n && !final_chunk) return 0;          // (its '\n' may be the next chunk's first byte)
        *pos = p;
        return ch == '>' ? (int)RP_FASTA : ch == '@' ? (int)RP_FASTQ : -1;
    }
    return 0;
}

// what the counters of the classify / records passes say about the chunk: null, or what is wrong (*pos = the line's begin)
inline const char *rp_verdict(uint32_t format, uint32_t n_lines, bool final_chunk, const RpCounters &k, uint64_t *pos) {
    uint64_t first = ~0ull;
    const char *what = nullptr;
    if (k.err_pos != RP_NO_ERROR && k.err_pos < k.consumed) {
        first = k.err_pos;
        what = format == RP_FASTQ ? "a FASTQ record is not four lines '@name', sequence, '+', quality of the sequence's length"
                                  : "a FASTA sequence line begins with '@' or '+', or stands in front of the first header";
    }
    if (format == RP_FASTQ && final_chunk && ((k.last_nonempty + 3u) >> 2) > (n_lines >> 2) && k.trunc_pos < first) {
        first = k.trunc_pos;
        what = "the last FASTQ record has fewer than four lines";
    }
    *pos = first;
    return what;
}

} // namespace mgx
