// tsv_format.hpp — the TSV text of an alignment batch (cli/align.cpp:262-285, restated by mgx_format_tsv_labeled in mgx_text.hip),
// from what mgx_align_batch_device leaves in device memory: the ReadResult records, the output stream (align_types.hpp:51-64,
// host_common.hpp:153-159) and the raw read bytes; plus the headers and the label names the caller hands over.
//
// Written against the wave interface (wave.hpp): tests/test_tsv_format_model.py compiles this very file for the host
// (tests/emu/wave.hpp) and compares its bytes with the host formatter's.  Two passes:
//   size    tf_line_size: one query per lane walks the query's alignments and adds up the characters of its line; an exclusive
//           scan over the batch (the caller's) turns the lengths into line_begin.
//   write   tf_write_line: one wavefront per query.  The three bulk copies (header, normalised query, path spelling) are
//           lane-strided; their body goes out as 4-byte stores to the 4-byte aligned part of the destination, a lane per dword
//           (256 contiguous bytes per wave instruction), the source re-aligned from two aligned dword loads; only the up to three
//           bytes in front of and behind that part are byte stores.  CIGAR runs and labels: a lane per run / label, placed by
//           a wavefront prefix sum of their widths.  The few scalar fields (orientation, score, matches, offset) are lane 0's.
// A query whose record carries ST_CAPACITY (the device records are pre-retry) gets a line of length 0 and is listed in
// cap_list: the host aligns it again and formats its line (mgx_format_tsv_batch).
#pragma once
#include "wave.hpp"
#include "align_types.hpp"

namespace mgx {

struct TfBatch {
    const ReadResult *results;
    const uint32_t *stream;
    const char *seqs;                // the raw reads, query q = seqs[offsets[q] .. offsets[q + 1])
    const uint64_t *offsets;
    const char *headers;             // header q = headers[header_offsets[q] .. header_offsets[q + 1])
    const uint64_t *header_offsets;
    const char *name_bytes;          // label l < n_names prints as name_bytes[name_begin[l] .. name_begin[l + 1]); others as numbers
    const uint32_t *name_begin;      // n_names + 1 (null when n_names == 0)
    uint64_t *line_len;              // size pass: n_queries lengths (the scan's input)
    const uint64_t *line_begin;      // write pass: n_queries + 1 byte offsets into text
    char *text;
    uint32_t *cap_list;              // size pass: the queries left to the host, in any order ...
    unsigned long long *cap_count;   // ... and how many
    uint64_t n_queries;
    uint32_t n_names;
    int32_t min_path_score;
    uint32_t labeled;                // the stream carries a label list behind every alignment
    uint32_t pad;
};

MGX_DEV uint32_t tf_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
         : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
MGX_DEV uint32_t tf_digits_signed(int32_t v) { return v < 0 ? 1u + tf_digits(0u - (uint32_t)v) : tf_digits((uint32_t)v); }

// the nd = tf_digits(v) characters of v, last digit first
MGX_DEV void tf_put_u32(char *dst, uint32_t v, uint32_t nd) {
    for (uint32_t i = nd; i-- > 0;) { gst(dst + i, (char)('0' + v % 10u)); v /= 10u; }
}
MGX_DEV void tf_put_i32(char *dst, int32_t v, uint32_t nd) {
    if (v < 0) { gst(dst, '-'); tf_put_u32(dst + 1, 0u - (uint32_t)v, nd - 1); }
    else tf_put_u32(dst, (uint32_t)v, nd);
}

// the query as AlignmentResults keeps it: toupper in the C locale (a-z only), bytes >= 0x80 become 127
MGX_DEV char tf_norm1(char ch) {
    const uint8_t c = (uint8_t)ch;
    return (char)(c >= 0x80 ? 127 : (c >= 'a' && c <= 'z') ? c - 32 : c);
}
// ... four bytes at a time (no carry crosses a byte: the 7-bit fields stay below 0x100)
MGX_DEV uint32_t tf_norm4(uint32_t w) {
    const uint32_t low7 = w & 0x7F7F7F7Fu;
    const uint32_t lower = (low7 + 0x1F1F1F1Fu) & ~(low7 + 0x05050505u) & ~w & 0x80808080u;      // bit 7 of every a-z byte
    const uint32_t high = ((w & 0x80808080u) >> 7) * 0xFFu;                                        // 0xFF in every byte >= 0x80
    return ((w ^ (lower >> 2)) & ~high) | (high & 0x7F7F7F7Fu);
}

// characters a label takes
MGX_DEV uint32_t tf_label_width(const TfBatch &b, uint32_t lbl) {
    return lbl < b.n_names ? gld(b.name_begin + lbl + 1) - gld(b.name_begin + lbl) : tf_digits(lbl);
}

// the scalars of alignment a of a record (a == 0: the record's own; else six words of the stream at *at, which moves past them)
// (U: the value is the same on every lane of the wavefront — the write pass — and goes to a scalar register)
template <bool U, class T> MGX_DEV T tf_ld(const T *p) { if constexpr (U) return uni(gld(p)); else return gld(p); }

struct TfAln { int32_t score; uint32_t offset, n_nodes, n_cigar, seq_len, orientation; };
template <bool U>
MGX_DEV TfAln tf_aln_header(const TfBatch &b, const ReadResult &r, int32_t a, uint64_t *at) {
    TfAln h = { r.score, r.offset, r.n_nodes, r.n_cigar, r.seq_len, r.orientation };
    if (a) {
        const uint32_t *w = b.stream + *at;
        h.score = (int32_t)tf_ld<U>(w); h.offset = tf_ld<U>(w + 1); h.n_nodes = tf_ld<U>(w + 2); h.n_cigar = tf_ld<U>(w + 3);
        h.seq_len = tf_ld<U>(w + 4); h.orientation = tf_ld<U>(w + 5);
        *at += 6;
    }
    return h;
}

// (the fields the formatters read; the record's tail is parity-test material)
template <bool U>
MGX_DEV ReadResult tf_record_at(const ReadResult *p) {
    ReadResult r;
    r.status = tf_ld<U>(&p->status); r.n_alignments = tf_ld<U>(&p->n_alignments); r.score = tf_ld<U>(&p->score);
    r.offset = tf_ld<U>(&p->offset); r.n_nodes = tf_ld<U>(&p->n_nodes); r.n_cigar = tf_ld<U>(&p->n_cigar);
    r.seq_len = tf_ld<U>(&p->seq_len); r.orientation = tf_ld<U>(&p->orientation); r.stream_off = tf_ld<U>(&p->stream_off);
    return r;
}
template <bool U>
MGX_DEV ReadResult tf_record(const TfBatch &b, uint64_t q) { return tf_record_at<U>(b.results + q); }

MGX_DEV bool tf_has_alignments(const ReadResult &r) { return r.status == ST_OK && r.n_alignments > 0; }

// the "no alignment" tail: "\t*\t*\t" min_path_score "\t*\t*\t*\n"
MGX_DEV uint32_t tf_star_width(int32_t min_path_score) { return 5u + tf_digits_signed(min_path_score) + 7u; }

// ---- size pass: the length of query q's line; 0 and an entry of cap_list for a capacity-status record -------------------
MGX_DEV uint64_t tf_line_size(const TfBatch &b, uint64_t q) {
    const ReadResult r = tf_record<false>(b, q);
    if (r.status == ST_CAPACITY) {
#if MGX_WAVE_EMU
        const unsigned long long at = (*b.cap_count)++;
#else
        const unsigned long long at = atomicAdd(b.cap_count, 1ull);
#endif
        gst(b.cap_list + at, (uint32_t)q);
        return 0;
    }
    uint64_t len = (gld(b.header_offsets + q + 1) - gld(b.header_offsets + q)) + 1u + (gld(b.offsets + q + 1) - gld(b.offsets + q));
    if (!tf_has_alignments(r)) return len + tf_star_width(b.min_path_score);
    uint64_t at = r.stream_off;
    for (int32_t a = 0; a < r.n_alignments; ++a) {
        const TfAln h = tf_aln_header<false>(b, r, a, &at);
        const uint32_t *cg = b.stream + at + h.n_nodes;
        uint32_t matches = 0;
        for (uint32_t x = 0; x < h.n_cigar; ++x) {
            const uint32_t w = gld(cg + x);
            if ((w & 7u) == OP_MATCH) matches += w >> 3;
            len += tf_digits(w >> 3) + 1u;
        }
        // "\t+\t" path '\t' score '\t' matches '\t' cigar '\t' offset
        len += 3u + h.seq_len + 1u + tf_digits_signed(h.score) + 1u + tf_digits(matches) + 1u + 1u + tf_digits(h.offset);
        at += (uint64_t)h.n_nodes + h.n_cigar + ((uint64_t)h.seq_len + 3) / 4;
        if (b.labeled) {
            const uint32_t nl = gld(b.stream + at);
            for (uint32_t x = 0; x < nl; ++x) len += 1u + tf_label_width(b, gld(b.stream + at + 1 + x));     // '\t' or ';' + the label
            at += 1 + (uint64_t)nl;
        }
    }
    return len + 1u;                 // '\n'
}

// ---- write pass ----------------------------------------------------------------------------------------------------------
// dst[0 .. n) = src[0 .. n), normalised on the way if `norm`; the whole wavefront.  The aligned dwords that hold src's first
// and last byte are read whole (never a dword without a byte of src in it).
MGX_DEV void tf_copy(char *dst, const char *src, uint32_t n, bool norm) {
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
    const uint32_t head = mis ? (4u - mis < n ? 4u - mis : n) : 0u;
    const uint32_t body = (n - head) >> 2, tail = (n - head) & 3u;
    const char *s = src + head;
    char *d = dst + head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(s - sh);
    FOR_LANES(l) {
        if ((uint32_t)l < head) { const char c = gld(src + l); gst(dst + l, norm ? tf_norm1(c) : c); }
        for (uint32_t i = (uint32_t)l; i < body; i += WAVE) {
            uint32_t w = gld(sa + i);
            if (sh) w = (uint32_t)((((uint64_t)gld(sa + i + 1) << 32) | w) >> (8u * sh));
            gst(reinterpret_cast<uint32_t *>(d) + i, norm ? tf_norm4(w) : w);
        }
        if ((uint32_t)l < tail) { const char c = gld(s + 4u * body + l); gst(d + 4u * body + l, norm ? tf_norm1(c) : c); }
    }
}

// the line of query q at text + line_begin[q]; the whole wavefront (q is wave-uniform).  Returns the characters written.
MGX_DEV uint64_t tf_write_line(const TfBatch &b, uint64_t q) {
    const ReadResult r = tf_record<true>(b, q);
    if (r.status == ST_CAPACITY) return 0;            // the host's
    char *out = b.text + tf_ld<true>(b.line_begin + q);
    const uint64_t hb = tf_ld<true>(b.header_offsets + q), sb = tf_ld<true>(b.offsets + q);
    const uint32_t hlen = (uint32_t)(tf_ld<true>(b.header_offsets + q + 1) - hb), qlen = (uint32_t)(tf_ld<true>(b.offsets + q + 1) - sb);
    uint64_t pos = 0;
    tf_copy(out, b.headers + hb, hlen, false);
    pos += hlen;
    FOR_LANES(l) { if (l == 0) gst(out + pos, '\t'); }
    pos += 1;
    tf_copy(out + pos, b.seqs + sb, qlen, true);
    pos += qlen;
    if (!tf_has_alignments(r)) {
        const uint32_t nd = tf_digits_signed(b.min_path_score);
        FOR_LANES(l) {
            if (l == 0) {
                char *p = out + pos;
                gst(p, '\t'); gst(p + 1, '*'); gst(p + 2, '\t'); gst(p + 3, '*'); gst(p + 4, '\t');
                tf_put_i32(p + 5, b.min_path_score, nd);
                p += 5 + nd;
                gst(p, '\t'); gst(p + 1, '*'); gst(p + 2, '\t'); gst(p + 3, '*'); gst(p + 4, '\t'); gst(p + 5, '*'); gst(p + 6, '\n');
            }
        }
        return pos + 5 + nd + 7;
    }
    uint64_t at = r.stream_off;
    for (int32_t a = 0; a < r.n_alignments; ++a) {
        const TfAln h = tf_aln_header<true>(b, r, a, &at);
        const uint32_t *cg = b.stream + at + h.n_nodes;
        // num_matches (host_common.hpp:187-197) comes in front of the CIGAR: one pass over the runs for it
        uint32_t matches = 0;
        for (uint32_t base = 0; base < h.n_cigar; base += WAVE) {
            LV<int32_t> m;
            FOR_LANES(l) {
                const uint32_t x = base + (uint32_t)l;
                const uint32_t w = x < h.n_cigar ? gld(cg + x) : 0u;
                m[l] = (w & 7u) == OP_MATCH ? (int32_t)(w >> 3) : 0;
            }
            matches += (uint32_t)uni(wave_sum(m));
        }
        const uint32_t nd_score = tf_digits_signed(h.score), nd_matches = tf_digits(matches), nd_offset = tf_digits(h.offset);
        FOR_LANES(l) {
            if (l == 0) { char *p = out + pos; gst(p, '\t'); gst(p + 1, h.orientation ? '-' : '+'); gst(p + 2, '\t'); }
        }
        pos += 3;
        tf_copy(out + pos, reinterpret_cast<const char *>(cg + h.n_cigar), h.seq_len, false);
        pos += h.seq_len;
        FOR_LANES(l) {
            if (l == 0) {
                char *p = out + pos;
                gst(p, '\t'); tf_put_i32(p + 1, h.score, nd_score);
                p += 1 + nd_score;
                gst(p, '\t'); tf_put_u32(p + 1, matches, nd_matches);
                gst(p + 1 + nd_matches, '\t');
            }
        }
        pos += 3 + nd_score + nd_matches;
        for (uint32_t base = 0; base < h.n_cigar; base += WAVE) {
            LV<int32_t> wd;
            LV<uint32_t> run;
            FOR_LANES(l) {
                const uint32_t x = base + (uint32_t)l;
                run[l] = x < h.n_cigar ? gld(cg + x) : 0u;
                wd[l] = x < h.n_cigar ? (int32_t)tf_digits(run[l] >> 3) + 1 : 0;
            }
            const LV<int32_t> first = wave_prefix_sum_excl(wd);
            FOR_LANES(l) {
                if (wd[l]) {
                    char *p = out + pos + first[l];
                    tf_put_u32(p, run[l] >> 3, (uint32_t)wd[l] - 1u);
                    const uint32_t op = run[l] & 7u;
                    gst(p + wd[l] - 1, op == 0 ? 'S' : op == 1 ? 'X' : op == 2 ? '=' : op == 3 ? 'D' : op == 4 ? 'I' : 'G');
                }
            }
            pos += (uint32_t)uni(wave_sum(wd));
        }
        FOR_LANES(l) {
            if (l == 0) { gst(out + pos, '\t'); tf_put_u32(out + pos + 1, h.offset, nd_offset); }
        }
        pos += 1 + nd_offset;
        at += (uint64_t)h.n_nodes + h.n_cigar + ((uint64_t)h.seq_len + 3) / 4;
        if (b.labeled) {
            const uint32_t nl = tf_ld<true>(b.stream + at);
            const uint32_t *lb = b.stream + at + 1;
            // '\t' in front of the first label, ';' in front of every other one: each label is one more character than its width
            for (uint32_t base = 0; base < nl; base += WAVE) {
                LV<int32_t> wd;
                LV<uint32_t> lbl;
                FOR_LANES(l) {
                    const uint32_t x = base + (uint32_t)l;
                    lbl[l] = x < nl ? gld(lb + x) : 0u;
                    wd[l] = x < nl ? (int32_t)tf_label_width(b, lbl[l]) + 1 : 0;
                }
                const LV<int32_t> first = wave_prefix_sum_excl(wd);
                FOR_LANES(l) {
                    if (wd[l]) {
                        char *p = out + pos + first[l];
                        gst(p, base + (uint32_t)l == 0 ? '\t' : ';');
                        if (lbl[l] < b.n_names) {
                            const char *nm = b.name_bytes + gld(b.name_begin + lbl[l]);
                            for (int32_t i = 0; i + 1 < wd[l]; ++i) gst(p + 1 + i, gld(nm + i));
                        } else tf_put_u32(p + 1, lbl[l], (uint32_t)wd[l] - 1u);
                    }
                }
                pos += (uint32_t)uni(wave_sum(wd));
            }
            at += 1 + (uint64_t)nl;
        }
    }
    FOR_LANES(l) { if (l == 0) gst(out + pos, '\n'); }
    return pos + 1;
}

} // namespace mgx
