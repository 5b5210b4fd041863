// json_format.hpp — the text of `metagraph align --json` for an alignment batch (cli/align.cpp:287-305, Alignment::to_json and
// path_json; restated by mgx_format_json in mgx_text.hip), from what mgx_align_batch_device leaves in device memory: the ReadResult
// records, the output stream (align_types.hpp:51-64, host_common.hpp:153-159) and the raw read bytes; plus the caller's headers.
//
// Written against the wave interface (wave.hpp): tests/test_json_format_model.py compiles this very file for the host
// (tests/emu/wave.hpp) and compares its bytes with the host formatter's.  Two passes over ONE walk, jf_line<W>: a wavefront per
// query either counts the characters of the query's lines (W = false: the size pass; an exclusive scan over the range, the
// caller's, turns the lengths into line_begin) or stores them (W = true).  Every width the write pass places text by is computed
// by the function the size pass added up, so the two cannot disagree.
//   strings   (name, sequence, ref_sequence): a lane per byte, 64 at a time; escaped width, wavefront prefix sum, store.
//   CIGAR     a lane per run, as tsv_format.hpp does.
//   mapping   the first node's object is serial (it covers up to k characters and any number of runs) and is lane 0's; every
//             further node is a lane, 64 at a time.  Node ni >= 1 owns one position of a node-consuming run (X, =, D) and the
//             insertion / clip run directly in front of that position: a prefix sum of the node-consuming lengths over 64 runs
//             gives every run its first position, each lane finds its run by a six-step binary search over those (cross-lane
//             reads), computes the width of its object, and a second prefix sum places the objects.
//   identity  "%.17g" of num_matches / length in integer arithmetic (jf_identity), lane 0's.
// What is taken for granted about a record (true of what the extension kernels write; mgx.h says so at mgx_format_json_batch):
// offset < k; behind the first node's k characters no insertion / clip run follows another one while nodes are left; num_matches
// <= the aligned query's length; and n_nodes is what the CIGAR pays for — the first node takes k - offset node-consuming
// positions, every other node one — or less.  (With MORE nodes than that, path_json's loop prints one more object that carries a
// trailing insertion / clip run alone; the lanes print objects for positions only.)  For a record outside these the size and the
// write pass still agree with each other — no byte is written outside the line — but the text is not mgx_format_json's.
// A query whose record carries ST_CAPACITY gets length 0 and is listed in cap_list, as in tsv_format.hpp.
#pragma once
#include "wave.hpp"
#include "align_types.hpp"
#include "tsv_format.hpp"

namespace mgx {

struct JfBatch {
    const ReadResult *results;       // the whole staged batch
    const uint32_t *stream;
    const char *seqs;                // the raw reads, query q = seqs[offsets[q] .. offsets[q + 1])
    const uint64_t *offsets;
    const char *headers;             // the RANGE's headers: query first + i has headers[header_offsets[i] - header_from ..
    const uint64_t *header_offsets;  //                                                      header_offsets[i + 1] - header_from)
    uint64_t *line_len;              // size pass: n_queries lengths, by i (the scan's input)
    const uint64_t *line_begin;      // write pass: n_queries + 1 byte offsets into text, by i
    char *text;
    uint32_t *cap_list;              // size pass: the i left to the host, in any order ...
    unsigned long long *cap_count;   // ... and how many
    uint64_t first, n_queries;       // the range: queries first .. first + n_queries of the batch
    uint32_t k;
    uint32_t labeled;                // the stream carries a label list behind every alignment (skipped: JSON has no labels)
    uint64_t header_from;            // what the caller's offsets start from (header_offsets[0])
};

// the strand a line prints from: the normalised query (tf_norm1) or its reverse complement (reverse_complement.hpp:31-62)
struct JfStrand { const char *seq; uint32_t qlen, rc; };

MGX_DEV char jf_complement(char ch) {
    const uint8_t c = (uint8_t)ch;
    const char *up = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
    return (c >= 'A' && c <= 'Z') ? up[c - 'A'] : (c >= 'a' && c <= 'z') ? (char)(up[c - 'a'] + 32) : c == 96 ? (char)64 : ch;
}
// character i of the strand (0 beyond its end: never the case for a record as described above)
MGX_DEV char jf_strand_byte(const JfStrand &s, uint32_t i) {
    if (i >= s.qlen) return 0;
    return s.rc ? jf_complement(tf_norm1(gld(s.seq + (s.qlen - 1u - i)))) : tf_norm1(gld(s.seq + i));
}

// json_string's escapes: \" \\ \b \f \n \r \t, \u00XX for the other bytes below 0x20 and all from 0x7F
MGX_DEV uint32_t jf_esc_width(char ch) {
    const uint8_t c = (uint8_t)ch;
    if (c == '"' || c == '\\' || (c >= 8 && c <= 13 && c != 11)) return 2u;
    return (c < 0x20 || c >= 0x7F) ? 6u : 1u;
}
MGX_DEV void jf_esc_put(char *p, char ch, uint32_t wd) {
    const uint8_t c = (uint8_t)ch;
    if (wd == 1u) { gst(p, ch); return; }
    gst(p, '\\');
    if (wd == 2u) { gst(p + 1, c == '"' ? '"' : c == '\\' ? '\\' : c == 8 ? 'b' : c == 12 ? 'f' : c == 10 ? 'n' : c == 13 ? 'r' : 't'); return; }
    const uint32_t hi = c >> 4, lo = c & 15u;
    gst(p + 1, 'u'); gst(p + 2, '0'); gst(p + 3, '0');
    gst(p + 4, (char)(hi < 10 ? '0' + hi : 'A' + hi - 10)); gst(p + 5, (char)(lo < 10 ? '0' + lo : 'A' + lo - 10));
}

// value of lane `src` of x, src differing from lane to lane; every lane of the wavefront calls it together
MGX_DEV int32_t jf_gather(const LV<int32_t> &x, int src) {
#if MGX_WAVE_EMU
    return x[src & (WAVE - 1)];
#else
    return __builtin_amdgcn_ds_bpermute((src & (WAVE - 1)) << 2, x.v);
#endif
}

// ---- pieces one lane writes at p + w (W) or only measures; each returns the characters it takes ------------------------------
template <bool W> MGX_DEV uint32_t jf_put(char *p, uint32_t w, const char *s, uint32_t n) {
    if constexpr (W) for (uint32_t i = 0; i < n; ++i) gst(p + w + i, s[i]);
    return n;
}
#define JF_PUT(s) w += jf_put<W>(p, w, s, (uint32_t)sizeof(s) - 1u)
template <bool W> MGX_DEV uint32_t jf_put_num(char *p, uint32_t w, uint32_t v) {
    const uint32_t nd = tf_digits(v);
    if constexpr (W) tf_put_u32(p + w, v, nd);
    return nd;
}
// "..." of n characters of the strand from `at`
template <bool W> MGX_DEV uint32_t jf_put_strand(char *p, uint32_t w0, const JfStrand &s, uint32_t at, uint32_t n) {
    uint32_t w = w0;
    JF_PUT("\"");
    for (uint32_t i = 0; i < n; ++i) {
        const char c = jf_strand_byte(s, at + i);
        const uint32_t wd = jf_esc_width(c);
        if constexpr (W) jf_esc_put(p + w, c, wd);
        w += wd;
    }
    JF_PUT("\"");
    return w - w0;
}
// one edit object (json_edit): keys from_length, sequence, to_length — those that are set; a ',' in front of all but the first
template <bool W> MGX_DEV uint32_t jf_put_edit(char *p, uint32_t w0, bool first, bool has_from, uint32_t from_len, bool has_seq, const JfStrand &s,
                                               uint32_t at, uint32_t n, bool has_to, uint32_t to_len) {
    uint32_t w = w0;
    if (!first) JF_PUT(",");
    JF_PUT("{");
    if (has_from) { JF_PUT("\"from_length\":"); w += jf_put_num<W>(p, w, from_len); }
    if (has_seq) {
        if (has_from) JF_PUT(",");
        JF_PUT("\"sequence\":");
        w += jf_put_strand<W>(p, w, s, at, n);
    }
    if (has_to) {
        if (has_from || has_seq) JF_PUT(",");
        JF_PUT("\"to_length\":");
        w += jf_put_num<W>(p, w, to_len);
    }
    JF_PUT("}");
    return w - w0;
}

// where the CIGAR and the strand stand behind the first node's object
struct JfCursor { uint32_t ci, c_off, qs; };

// the first node's object: the `cur < k` loop of path_json.  U: every lane runs it with the same values (the count); else lane 0.
template <bool W, bool U>
MGX_DEV uint32_t jf_first_object(char *p, const uint32_t *cg, uint32_t n_cigar, uint32_t k, uint32_t offset, uint32_t node0,
                                 const JfStrand &s, uint32_t clipping, JfCursor *end) {
    uint32_t w = 0, ci = 0, qs = clipping;
    if (n_cigar && (tf_ld<U>(cg) & 7u) == OP_CLIPPED) ++ci;
    uint64_t c_off = 0, cur = offset;
    bool first = true;
    JF_PUT("{\"edit\":[");
    while (cur < k && ci < n_cigar) {
        const uint32_t run = tf_ld<U>(cg + ci), len = run >> 3, op = run & 7u;
        if (op == OP_CLIPPED) { ++ci; c_off = 0; continue; }           // trailing clip
        uint64_t next_pos = cur + (len - c_off);
        if (next_pos > k) next_pos = k;
        const uint32_t ns = (uint32_t)(next_pos - cur);
        if (op == OP_MISMATCH) { w += jf_put_edit<W>(p, w, first, true, ns, true, s, qs, ns, true, ns); qs += ns; first = false; }
        else if (op == OP_INSERTION) { w += jf_put_edit<W>(p, w, first, false, 0, true, s, qs, ns, true, ns); qs += ns; next_pos = cur; first = false; }
        else if (op == OP_DELETION) { w += jf_put_edit<W>(p, w, first, true, ns, false, s, 0, 0, false, 0); first = false; }
        else if (op == OP_MATCH) { w += jf_put_edit<W>(p, w, first, true, ns, false, s, 0, 0, true, ns); qs += ns; first = false; }
        c_off += ns;
        cur = next_pos;
        if (c_off == len) { ++ci; c_off = 0; }
    }
    JF_PUT("],\"position\":{\"node_id\":");
    w += jf_put_num<W>(p, w, node0);
    if (offset) { JF_PUT(",\"offset\":"); w += jf_put_num<W>(p, w, offset); }
    JF_PUT("},\"rank\":1}");
    end->ci = ci; end->c_off = (uint32_t)c_off; end->qs = qs;
    return w;
}

// the object of node ni >= 1 (rank ni + 1): the insertion it owns, if any (ins_len characters of the strand from ins_at), then its
// one position of a run of operator op (the strand's character at q_at, if it has one)
template <bool W>
MGX_DEV uint32_t jf_node_object(char *p, uint32_t node, uint32_t rank, uint32_t k, uint32_t op, bool has_ins, uint32_t ins_at,
                                uint32_t ins_len, uint32_t q_at, const JfStrand &s) {
    uint32_t w = 0;
    JF_PUT(",{\"edit\":[");
    if (has_ins) w += jf_put_edit<W>(p, w, true, false, 0, true, s, ins_at, ins_len, true, ins_len);
    if (op == OP_MISMATCH) w += jf_put_edit<W>(p, w, !has_ins, true, 1, true, s, q_at, 1, true, 1);
    else if (op == OP_DELETION) w += jf_put_edit<W>(p, w, !has_ins, true, 1, false, s, 0, 0, false, 0);
    else if (op == OP_MATCH) w += jf_put_edit<W>(p, w, !has_ins, true, 1, false, s, 0, 0, true, 1);
    JF_PUT("],\"position\":{\"node_id\":");
    w += jf_put_num<W>(p, w, node);
    JF_PUT(",\"offset\":");
    w += jf_put_num<W>(p, w, k - 1u);
    JF_PUT("},\"rank\":");
    w += jf_put_num<W>(p, w, rank);
    JF_PUT("}");
    return w;
}

// ---- identity: snprintf("%.17g", (double)m / (double)len), ".0" appended when that has none of ".eEn"; 0 <= m <= len -----------
// Integer arithmetic only.  The double nearest to m / len is M / 2^E, M < 2^53 + 1, by long division (round half to even); its
// exact decimal expansion comes from a 128-bit binary fraction (four 32-bit limbs) multiplied by ten, digit by digit; the 17th
// significant digit is rounded on the exact remainder (half to even), as glibc does.  len < 2^32 keeps E <= 84 < 128 - 54.
template <bool W> MGX_DEV uint32_t jf_identity(char *p, uint32_t m, uint32_t len) {
    uint32_t w = 0;
    if (len == 0 || m == 0) { JF_PUT("0.0"); return w; }
    if (m >= len) { JF_PUT("1.0"); return w; }
    uint64_t r = m, M = 1;
    uint32_t E = 52;
    while (r < len) { r <<= 1; ++E; }
    r -= len;
    for (int i = 0; i < 52; ++i) {
        r <<= 1;
        M <<= 1;
        if (r >= len) { r -= len; M |= 1u; }
    }
    if (2 * r > len || (2 * r == len && (M & 1u))) ++M;
    // F / 2^128 = M / 2^E: limbs f[3] (most significant) .. f[0]
    const uint32_t sh = 128u - E;                      // 44 .. 75
    uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;
    {
        // (M << sh) as 128 bits: the low 64 and the high 64
        const uint64_t lo64 = sh >= 64u ? 0 : M << sh;
        const uint64_t hi64 = sh >= 64u ? M << (sh - 64u) : M >> (64u - sh);
        f0 = (uint32_t)lo64; f1 = (uint32_t)(lo64 >> 32); f2 = (uint32_t)hi64; f3 = (uint32_t)(hi64 >> 32);
    }
    auto times10 = [&]() -> uint32_t {
        uint64_t c = (uint64_t)f0 * 10u; f0 = (uint32_t)c; c >>= 32;
        c += (uint64_t)f1 * 10u; f1 = (uint32_t)c; c >>= 32;
        c += (uint64_t)f2 * 10u; f2 = (uint32_t)c; c >>= 32;
        c += (uint64_t)f3 * 10u; f3 = (uint32_t)c; c >>= 32;
        return (uint32_t)c;
    };
    int32_t X = -1;                                     // the decimal exponent of the first significant digit
    uint32_t d = times10();
    while (d == 0) { d = times10(); --X; }
    uint64_t D = d;
    for (int i = 1; i < 17; ++i) D = D * 10u + times10();
    const bool above = f3 > 0x80000000u || (f3 == 0x80000000u && (f0 | f1 | f2) != 0), tie = f3 == 0x80000000u && (f0 | f1 | f2) == 0;
    if (above || (tie && (D & 1u))) ++D;
    if (D == 100000000000000000ull) { D = 10000000000000000ull; ++X; }
    uint32_t nsig = 17;
    while (D % 10u == 0) { D /= 10u; --nsig; }
    // %g: exponent form when X < -4 (X >= 17 cannot be), else fixed; trailing zeros are gone already
    if (X < -4) {
        const uint32_t ex = (uint32_t)-X, total = nsig + (nsig > 1 ? 1u : 0u) + 2u + (ex < 100 ? 2u : 3u);
        if constexpr (W) {
            uint64_t v = D;
            for (uint32_t i = nsig; i-- > 1;) { gst(p + 1 + i, (char)('0' + v % 10u)); v /= 10u; }
            gst(p, (char)('0' + v));
            if (nsig > 1) gst(p + 1, '.');
            char *e = p + nsig + (nsig > 1 ? 1u : 0u);
            gst(e, 'e'); gst(e + 1, '-');
            if (ex < 100) { gst(e + 2, (char)('0' + ex / 10u)); gst(e + 3, (char)('0' + ex % 10u)); }
            else tf_put_u32(e + 2, ex, 3);
        }
        return total;
    }
    if (X >= 0) {                                       // d[.ddd], ".0" behind a lone digit (not reached for m < len)
        if constexpr (W) {
            uint64_t v = D;
            for (uint32_t i = nsig; i-- > 1;) { gst(p + 1 + i, (char)('0' + v % 10u)); v /= 10u; }
            gst(p, (char)('0' + v)); gst(p + 1, '.');
            if (nsig == 1) gst(p + 2, '0');
        }
        return nsig == 1 ? 3u : nsig + 1u;
    }
    const uint32_t zeros = (uint32_t)(-X - 1);
    if constexpr (W) {
        gst(p, '0'); gst(p + 1, '.');
        for (uint32_t i = 0; i < zeros; ++i) gst(p + 2 + i, '0');
        uint64_t v = D;
        for (uint32_t i = nsig; i-- > 0;) { gst(p + 2 + zeros + i, (char)('0' + v % 10u)); v /= 10u; }
    }
    return 2u + zeros + nsig;
}

// ---- pieces the whole wavefront writes at o.out + o.pos --------------------------------------------------------------------
template <bool W> struct JfOut { char *out; uint64_t pos; };

template <bool W> MGX_DEV void jf_lit(JfOut<W> &o, const char *s, uint32_t n) {
    if constexpr (W) {
        FOR_LANES(l) { for (uint32_t i = (uint32_t)l; i < n; i += WAVE) gst(o.out + o.pos + i, s[i]); }
    }
    o.pos += n;
}
#define JF_LIT(s) jf_lit<W>(o, s, (uint32_t)sizeof(s) - 1u)

template <bool W> MGX_DEV void jf_num(JfOut<W> &o, uint32_t v) {
    const uint32_t nd = tf_digits(v);
    if constexpr (W) { FOR_LANES(l) { if (l == 0) tf_put_u32(o.out + o.pos, v, nd); } }
    o.pos += nd;
}

// "..." of src[0 .. n), escaped: raw bytes (s == nullptr) or the strand's characters from 0
template <bool W> MGX_DEV void jf_string(JfOut<W> &o, const char *src, const JfStrand *s, uint32_t n) {
    JF_LIT("\"");
    for (uint32_t base = 0; base < n; base += WAVE) {
        LV<int32_t> wd;
        LV<char> ch;
        FOR_LANES(l) {
            const uint32_t i = base + (uint32_t)l;
            ch[l] = i < n ? (s ? jf_strand_byte(*s, i) : gld(src + i)) : (char)0;
            wd[l] = i < n ? (int32_t)jf_esc_width(ch[l]) : 0;
        }
        if constexpr (W) {
            const LV<int32_t> first = wave_prefix_sum_excl(wd);
            FOR_LANES(l) { if (wd[l]) jf_esc_put(o.out + o.pos + first[l], ch[l], (uint32_t)wd[l]); }
        }
        o.pos += (uint32_t)uni(wave_sum(wd));
    }
    JF_LIT("\"");
}

// one alignment's line
template <bool W>
MGX_DEV void jf_alignment(JfOut<W> &o, const JfBatch &b, const TfAln &h, const uint32_t *nodes, bool secondary, const char *header,
                          uint32_t hlen, const char *seq, uint32_t qlen) {
    const uint32_t *cg = nodes + h.n_nodes;
    const JfStrand s = { seq, qlen, h.orientation ? 1u : 0u };
    // num_matches, clipping, end_clipping as HostResults::decode derives them
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
    uint32_t clipping = 0, end_clipping = 0;
    if (h.n_cigar) {
        const uint32_t f = tf_ld<true>(cg), e = tf_ld<true>(cg + h.n_cigar - 1);
        clipping = (f & 7u) == OP_CLIPPED ? f >> 3 : 0u;
        end_clipping = (e & 7u) == OP_CLIPPED ? e >> 3 : 0u;
    }
    const uint32_t qv_len = qlen - clipping - end_clipping;

    JF_LIT("{\"annotation\":{\"cigar\":\"");
    for (uint32_t base = 0; base < h.n_cigar; base += WAVE) {
        LV<int32_t> wd;
        LV<uint32_t> run;
        FOR_LANES(l) {
            const uint32_t x = base + (uint32_t)l;
            run[l] = x < h.n_cigar ? gld(cg + x) : 0u;
            wd[l] = x < h.n_cigar ? (int32_t)tf_digits(run[l] >> 3) + 1 : 0;
        }
        if constexpr (W) {
            const LV<int32_t> first = wave_prefix_sum_excl(wd);
            FOR_LANES(l) {
                if (wd[l]) {
                    char *p = o.out + o.pos + first[l];
                    tf_put_u32(p, run[l] >> 3, (uint32_t)wd[l] - 1u);
                    const uint32_t op = run[l] & 7u;
                    gst(p + wd[l] - 1, op == 0 ? 'S' : op == 1 ? 'X' : op == 2 ? '=' : op == 3 ? 'D' : op == 4 ? 'I' : 'G');
                }
            }
        }
        o.pos += (uint32_t)uni(wave_sum(wd));
    }
    JF_LIT("\"");
    if (h.seq_len) {
        JF_LIT(",\"ref_sequence\":");
        jf_string<W>(o, reinterpret_cast<const char *>(cg + h.n_cigar), nullptr, h.seq_len);
    }
    JF_LIT("},\"identity\":");
    {
        const uint32_t wd = jf_identity<false>(nullptr, matches, qv_len);
        if constexpr (W) { FOR_LANES(l) { if (l == 0) jf_identity<true>(o.out + o.pos, matches, qv_len); } }
        o.pos += wd;
    }
    if (secondary) JF_LIT(",\"is_secondary\":true");
    JF_LIT(",\"name\":");
    jf_string<W>(o, header, nullptr, hlen);
    if (h.n_nodes) {
        JF_LIT(",\"path\":{");
        if (tf_ld<true>(nodes) == tf_ld<true>(nodes + h.n_nodes - 1)) JF_LIT("\"is_circular\":true,");
        JF_LIT("\"length\":");
        jf_num<W>(o, h.n_nodes);
        JF_LIT(",\"mapping\":[");
        // the first node: counted by every lane alike, written by lane 0
        JfCursor c0;
        const uint32_t node0 = tf_ld<true>(nodes);
        const uint32_t w0 = jf_first_object<false, true>(nullptr, cg, h.n_cigar, b.k, h.offset, node0, s, clipping, &c0);
        if constexpr (W) {
            FOR_LANES(l) {
                if (l == 0) { JfCursor unused; jf_first_object<true, false>(o.out + o.pos, cg, h.n_cigar, b.k, h.offset, node0, s, clipping, &unused); }
            }
        }
        o.pos += w0;
        // the further nodes.  Position t (0-based) behind the first node's characters belongs to node t + 1.  Runs in chunks of 64
        // from c0.ci (that run counts with what is left of it); nbase / qbase: positions / strand characters in front of the chunk
        const uint32_t n_pos_max = h.n_nodes - 1u;
        uint32_t nbase = 0, qbase = c0.qs;
        int32_t prev_run = 7;                            // the run in front of the chunk (len << 3 | op); 7: none
        for (uint32_t base = c0.ci; base < h.n_cigar && nbase < n_pos_max; base += WAVE) {
            LV<int32_t> run, cons, qcons;
            FOR_LANES(l) {
                const uint32_t x = base + (uint32_t)l;
                uint32_t len = 0, op = 7u;
                if (x < h.n_cigar) {
                    const uint32_t w = gld(cg + x);
                    len = (w >> 3) - (x == c0.ci ? c0.c_off : 0u);
                    op = w & 7u;
                }
                run[l] = (int32_t)(len << 3 | op);
                cons[l] = (op == OP_MISMATCH || op == OP_MATCH || op == OP_DELETION || op == 5u) ? (int32_t)len : 0;
                qcons[l] = (op == OP_MISMATCH || op == OP_MATCH || op == OP_INSERTION || op == OP_CLIPPED) ? (int32_t)len : 0;
            }
            const LV<int32_t> nst = wave_prefix_sum_excl(cons), qst = wave_prefix_sum_excl(qcons);
            const uint32_t ctot = (uint32_t)uni(wave_sum(cons)), qtot = (uint32_t)uni(wave_sum(qcons));
            const uint32_t t_end = ctot < n_pos_max - nbase ? nbase + ctot : n_pos_max;
            for (uint32_t tb = nbase; tb < t_end; tb += WAVE) {
                LV<int32_t> wd;
                LV<uint32_t> v_node, v_op, v_ins_at, v_ins_len, v_q_at;
                LV<bool> v_ins;
                FOR_LANES(l) {
                    const uint32_t t = tb + (uint32_t)l;
                    const bool valid = t < t_end;
                    const int32_t rel = valid ? (int32_t)(t - nbase) : 0;
                    // the last run whose first position is <= rel (runs that take no position share it with the run behind them)
                    int lo = 0;
                    for (int step = WAVE / 2; step; step >>= 1) {
                        const int32_t v = jf_gather(nst, lo + step);
                        if (v <= rel) lo += step;
                    }
                    const uint32_t rw = (uint32_t)jf_gather(run, lo), pw_in = (uint32_t)jf_gather(run, lo + WAVE - 1);
                    const uint32_t pw = lo ? pw_in : (uint32_t)prev_run;
                    const uint32_t idx = (uint32_t)(rel - jf_gather(nst, lo)), q_run = qbase + (uint32_t)jf_gather(qst, lo);
                    const uint32_t op = rw & 7u, pop = pw & 7u;
                    v_op[l] = op;
                    v_ins[l] = idx == 0 && (pop == OP_INSERTION || pop == OP_CLIPPED);
                    v_ins_len[l] = pw >> 3;
                    v_ins_at[l] = q_run - (pw >> 3);
                    v_q_at[l] = q_run + idx;
                    v_node[l] = valid ? gld(nodes + 1 + t) : 0u;
                    wd[l] = valid ? (int32_t)jf_node_object<false>(nullptr, v_node[l], t + 2u, b.k, op, v_ins[l], v_ins_at[l], v_ins_len[l], v_q_at[l], s) : 0;
                }
                if constexpr (W) {
                    const LV<int32_t> first = wave_prefix_sum_excl(wd);
                    FOR_LANES(l) {
                        if (wd[l])
                            jf_node_object<true>(o.out + o.pos + first[l], v_node[l], tb + (uint32_t)l + 2u, b.k, v_op[l], v_ins[l], v_ins_at[l],
                                                 v_ins_len[l], v_q_at[l], s);
                    }
                }
                o.pos += (uint32_t)uni(wave_sum(wd));
            }
            nbase += ctot; qbase += qtot;
            prev_run = wave_bcast(run, WAVE - 1);
        }
        JF_LIT("],\"name\":\"\"}");
    }
    if (clipping) { JF_LIT(",\"query_position\":"); jf_num<W>(o, clipping); }
    if (qv_len) JF_LIT(",\"read_mapped\":true"); else JF_LIT(",\"read_mapped\":false");
    if (h.orientation) JF_LIT(",\"read_on_reverse_strand\":true");
    JF_LIT(",\"score\":");
    {
        const uint32_t nd = tf_digits_signed(h.score);
        if constexpr (W) { FOR_LANES(l) { if (l == 0) tf_put_i32(o.out + o.pos, h.score, nd); } }
        o.pos += nd;
    }
    JF_LIT(",\"sequence\":");
    jf_string<W>(o, nullptr, &s, qlen);
    if (clipping) JF_LIT(",\"soft_clipped\":true");
    JF_LIT("}\n");
}

// The lines of query first + i, the whole wavefront (i is wave-uniform).  W: stored at text + line_begin[i]; else only measured,
// and a capacity-status record is listed in cap_list.  Returns the characters (0 for a capacity-status record: the host's).
template <bool W>
MGX_DEV uint64_t jf_line(const JfBatch &b, uint64_t i) {
    const uint64_t q = b.first + i;
    const ReadResult r = tf_record_at<true>(b.results + q);
    if (r.status == ST_CAPACITY) {
        if constexpr (!W) {
            FOR_LANES(l) {
                if (l == 0) {
#if MGX_WAVE_EMU
                    const unsigned long long at = (*b.cap_count)++;
#else
                    const unsigned long long at = atomicAdd(b.cap_count, 1ull);
#endif
                    gst(b.cap_list + at, (uint32_t)i);
                }
            }
        }
        return 0;
    }
    JfOut<W> o = { nullptr, 0 };
    if constexpr (W) o.out = b.text + tf_ld<true>(b.line_begin + i);
    const uint64_t hb = tf_ld<true>(b.header_offsets + i), sb = tf_ld<true>(b.offsets + q);
    const uint32_t hlen = (uint32_t)(tf_ld<true>(b.header_offsets + i + 1) - hb), qlen = (uint32_t)(tf_ld<true>(b.offsets + q + 1) - sb);
    const char *header = b.headers + (hb - b.header_from), *seq = b.seqs + sb;
    if (!tf_has_alignments(r)) {
        // Alignment().to_json: an empty alignment carries its name and an empty sequence
        JF_LIT("{\"name\":");
        jf_string<W>(o, header, nullptr, hlen);
        JF_LIT(",\"sequence\":\"\"}\n");
        return o.pos;
    }
    uint64_t at = r.stream_off;
    for (int32_t a = 0; a < r.n_alignments; ++a) {
        TfAln h = { r.score, r.offset, r.n_nodes, r.n_cigar, r.seq_len, r.orientation };
        if (a) {
            const uint32_t *w = b.stream + at;
            h.score = (int32_t)tf_ld<true>(w); h.offset = tf_ld<true>(w + 1); h.n_nodes = tf_ld<true>(w + 2); h.n_cigar = tf_ld<true>(w + 3);
            h.seq_len = tf_ld<true>(w + 4); h.orientation = tf_ld<true>(w + 5);
            at += 6;
        }
        jf_alignment<W>(o, b, h, b.stream + at, a != 0, header, hlen, seq, qlen);
        at += (uint64_t)h.n_nodes + h.n_cigar + ((uint64_t)h.seq_len + 3) / 4;
        if (b.labeled) at += 1 + (uint64_t)tf_ld<true>(b.stream + at);
    }
    return o.pos;
}

#undef JF_LIT
#undef JF_PUT

} // namespace mgx
