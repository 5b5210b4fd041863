// map_format.hpp — the text of `metagraph align --map` for a whole batch (cli/align.cpp:91-173, restated per query by mgx_format_map
// in mgx_mapsum.hip), from what mgx_map_summary_batch leaves in device memory: the 12-byte count records, the 64-bit node array,
// node_begin and the raw read bytes; plus the headers the caller hands over and a presence threshold per k-mer count.
//
// Written against the wave interface (wave.hpp) like tsv_format.hpp: tests/test_map_format_model.py compiles this very file for
// the host (tests/emu/wave.hpp) and compares its bytes with mgx_format_map's.  Two passes:
//   size    COUNT_KMERS / QUERY_PRESENCE / FILTER_PRESENT: mf_line_size, one query per lane (a few loads and digit counts).
//           NODES: mf_nodes_size, one wavefront per query — the lanes take 64 windows at a time (one coalesced load of 64 nodes),
//           count their lines' characters and wave_sum adds them up.  An exclusive scan (the caller's) gives line_begin.
//   write   mf_write_line, one wavefront per query (QUERY_PRESENCE: mf_write_presence, one query per lane: its text is 2 bytes).
//           NODES: 64 windows per round, a lane per line placed by wave_prefix_sum_excl of the widths; the window's characters go
//           out as 4-byte stores to the aligned part of the line (mf_copy_lane, the technique of tf_copy within one lane).
//           Headers and whole queries (COUNT_KMERS, FILTER_PRESENT) are tf_copy's.
// Nothing is normalised: the reference prints the query's bytes as they came (lower case, N, bytes >= 0x80), so tf_copy runs
// with norm = false and the 4-byte normaliser of the TSV path has no business here.
// Presence is a comparison of integers: the host tabulates the threshold for every k-mer count of the batch with mgx_map_present's
// own double expressions (mgx_format_map_batch); no floating-point instruction exists on this path.
// Every offset and byte count is 64-bit (a NODES text passes 4 GB at about a million reads); the characters of one round of 64
// lines (at most 64 * (window + 23)) are 32-bit.
#pragma once
#include "wave.hpp"
#include "tsv_format.hpp"

namespace mgx {

enum { MF_NODES = 0, MF_COUNT_KMERS = 1, MF_QUERY_PRESENCE = 2, MF_FILTER_PRESENT = 3 };      // MGX_MAP_FMT_*

struct MfBatch {
    const uint32_t *counts;          // n_queries records of (n_discovered, n_kmers, n_unique)
    const uint64_t *nodes;           // NODES: the merged node array
    const uint64_t *node_begin;      // n_queries + 1
    const char *seqs;                // the raw reads, query q = seqs[offsets[q] .. offsets[q + 1])
    const uint64_t *offsets;
    const char *headers;             // header q = headers[header_offsets[q] .. header_offsets[q + 1])
    const uint64_t *header_offsets;
    const uint64_t *threshold;       // max_kmers + 1: full k max_missing[n_kmers], sub-k min_discovered[n_kmers]
    uint64_t *line_len;              // size pass: n_queries lengths (the scan's input)
    const uint64_t *line_begin;      // write pass: n_queries + 1 byte offsets into text
    char *text;
    uint64_t n_queries;
    uint32_t max_kmers;              // the last entry of `threshold`
    uint32_t k;
    uint32_t window;                 // characters per line of NODES: k, or map_length < k
    uint32_t sub_k;                  // map_length < k: the second presence formula
    int32_t format;
    uint32_t pad;
};

MGX_DEV uint32_t mf_digits64(uint64_t v) {
    if (v <= 0xFFFFFFFFull) return tf_digits((uint32_t)v);
    uint32_t nd = 10;
    for (uint64_t p = 10000000000ull; nd < 20 && v >= p; p *= 10ull) ++nd;       // (p is 10^19 at the last comparison)
    return nd;
}

// the nd = mf_digits64(v) characters of v, last digit first; 32-bit arithmetic once the value fits
MGX_DEV void mf_put_u64(char *dst, uint64_t v, uint32_t nd) {
    while (v > 0xFFFFFFFFull) { --nd; gst(dst + nd, (char)('0' + (uint32_t)(v % 10ull))); v /= 10ull; }
    tf_put_u32(dst, (uint32_t)v, nd);
}

struct MfCounts { uint32_t n_discovered, n_kmers, n_unique; };
template <bool U>
MGX_DEV MfCounts mf_counts(const MfBatch &b, uint64_t q) {
    const uint32_t *p = b.counts + 3 * q;
    MfCounts c = { tf_ld<U>(p), tf_ld<U>(p + 1), tf_ld<U>(p + 2) };
    return c;
}

// The threshold of a k-mer count, on the host: mgx_map_present's own expressions (mgx_mapsum.hip), evaluated nowhere else —
// full k: (size_t)(n_kmers * (1 - f)) k-mers may be missing; sub-k: (size_t)(n_kmers - n_kmers * (1 - f)) must be discovered
inline uint64_t mf_threshold_host(size_t n_kmers, double discovery_fraction, bool sub_k) {
    return sub_k ? (size_t)(n_kmers - n_kmers * (1 - discovery_fraction)) : (size_t)(n_kmers * (1 - discovery_fraction));
}

// mgx_map_present with the double expression looked up: full k (sequence_graph.cpp:65-89) absent below k characters, else present
// iff n_kmers - n_discovered <= max_missing[n_kmers]; sub-k (cli/align.cpp:139-149) present iff n_discovered >= min_discovered[n_kmers]
template <bool U>
MGX_DEV bool mf_present(const MfBatch &b, const MfCounts &c, uint64_t query_len) {
    const uint64_t t = tf_ld<U>(b.threshold + (c.n_kmers < b.max_kmers ? c.n_kmers : b.max_kmers));
    if (b.sub_k) return (uint64_t)c.n_discovered >= t;
    if (query_len < b.k) return false;
    return (uint64_t)c.n_kmers - (uint64_t)c.n_discovered <= t;
}

// the windows of query q that NODES prints: all of node_begin's, cut by the host formatter's guard w + window <= query_len
template <bool U>
MGX_DEV uint64_t mf_windows(const MfBatch &b, uint64_t q, uint64_t query_len) {
    const uint64_t n = tf_ld<U>(b.node_begin + q + 1) - tf_ld<U>(b.node_begin + q);
    const uint64_t fit = query_len >= b.window ? query_len - b.window + 1 : 0;
    return n < fit ? n : fit;
}

// ---- size pass -----------------------------------------------------------------------------------------------------------
// COUNT_KMERS, QUERY_PRESENCE, FILTER_PRESENT: the length of query q's text; one lane
MGX_DEV uint64_t mf_line_size(const MfBatch &b, uint64_t q) {
    if (b.format == MF_QUERY_PRESENCE) return 2;
    const MfCounts c = mf_counts<false>(b, q);
    const uint64_t hlen = gld(b.header_offsets + q + 1) - gld(b.header_offsets + q);
    if (b.format == MF_COUNT_KMERS) return hlen + 1u + tf_digits(c.n_discovered) + 1u + tf_digits(c.n_kmers) + 1u + tf_digits(c.n_unique) + 1u;
    const uint64_t qlen = gld(b.offsets + q + 1) - gld(b.offsets + q);
    return mf_present<false>(b, c, qlen) ? hlen + qlen + 3u : 0u;            // '>' header '\n' query '\n'
}

// NODES: the whole wavefront (q is wave-uniform)
MGX_DEV uint64_t mf_nodes_size(const MfBatch &b, uint64_t q) {
    const uint64_t qlen = tf_ld<true>(b.offsets + q + 1) - tf_ld<true>(b.offsets + q);
    const uint64_t nv = mf_windows<true>(b, q, qlen);
    const uint64_t *nodes = b.nodes + tf_ld<true>(b.node_begin + q);
    uint64_t len = 0;
    for (uint64_t base = 0; base < nv; base += WAVE) {
        LV<int32_t> wd;
        FOR_LANES(l) {
            const uint64_t w = base + (uint64_t)l;
            wd[l] = w < nv ? (int32_t)(b.window + 2u + mf_digits64(gld(nodes + w)) + 1u) : 0;
        }
        len += (uint32_t)uni(wave_sum(wd));
    }
    return len;
}

// ---- write pass ----------------------------------------------------------------------------------------------------------
// dst[0 .. n) = src[0 .. n) by ONE lane: bytes up to dst's 4-byte boundary, then whole dwords (the source re-aligned from two
// aligned dword loads, never a dword without a byte of src in it), then the up to three bytes left
MGX_DEV void mf_copy_lane(char *dst, const char *src, uint32_t n) {
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
    const uint32_t head = mis ? (4u - mis < n ? 4u - mis : n) : 0u;
    const uint32_t body = (n - head) >> 2, tail = (n - head) & 3u;
    for (uint32_t i = 0; i < head; ++i) gst(dst + i, gld(src + i));
    const char *s = src + head;
    char *d = dst + head;
    if (body) {
        const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
        const uint32_t *sa = reinterpret_cast<const uint32_t *>(s - sh);
        uint32_t lo = gld(sa);
        for (uint32_t i = 0; i < body; ++i) {
            uint32_t w = lo;
            if (sh) { lo = gld(sa + i + 1); w = (uint32_t)((((uint64_t)lo << 32) | w) >> (8u * sh)); }
            else if (i + 1 < body) lo = gld(sa + i + 1);
            gst(reinterpret_cast<uint32_t *>(d) + i, w);
        }
    }
    for (uint32_t i = 0; i < tail; ++i) gst(d + 4u * body + i, gld(s + 4u * body + i));
}

// ... by the whole wavefront, any length (tf_copy's lengths are 32-bit)
MGX_DEV void mf_copy_wave(char *dst, const char *src, uint64_t n) {
    for (uint64_t at = 0; at < n; at += 0x80000000ull) tf_copy(dst + at, src + at, (uint32_t)(n - at < 0x80000000ull ? n - at : 0x80000000ull), false);
}

// QUERY_PRESENCE: "0\n" / "1\n" at text + 2 q; one lane
MGX_DEV void mf_write_presence(const MfBatch &b, uint64_t q) {
    const MfCounts c = mf_counts<false>(b, q);
    const uint64_t qlen = gld(b.offsets + q + 1) - gld(b.offsets + q);
    char *out = b.text + gld(b.line_begin + q);
    gst(out, mf_present<false>(b, c, qlen) ? '1' : '0');
    gst(out + 1, '\n');
}

// the text of query q at text + line_begin[q]; the whole wavefront (q is wave-uniform).  Returns the characters written.
MGX_DEV uint64_t mf_write_line(const MfBatch &b, uint64_t q) {
    char *out = b.text + tf_ld<true>(b.line_begin + q);
    const uint64_t hb = tf_ld<true>(b.header_offsets + q), sb = tf_ld<true>(b.offsets + q);
    const uint64_t hlen = tf_ld<true>(b.header_offsets + q + 1) - hb, qlen = tf_ld<true>(b.offsets + q + 1) - sb;
    if (b.format == MF_NODES) {
        const uint64_t nv = mf_windows<true>(b, q, qlen);
        const uint64_t *nodes = b.nodes + tf_ld<true>(b.node_begin + q);
        const char *query = b.seqs + sb;
        uint64_t pos = 0;
        for (uint64_t base = 0; base < nv; base += WAVE) {
            LV<int32_t> wd;
            LV<uint64_t> node;
            FOR_LANES(l) {
                const uint64_t w = base + (uint64_t)l;
                node[l] = w < nv ? gld(nodes + w) : 0ull;
                wd[l] = w < nv ? (int32_t)(b.window + 2u + mf_digits64(node[l]) + 1u) : 0;
            }
            const LV<int32_t> first = wave_prefix_sum_excl(wd);
            FOR_LANES(l) {
                if (wd[l]) {
                    char *p = out + pos + (uint32_t)first[l];
                    mf_copy_lane(p, query + base + (uint64_t)l, b.window);
                    p += b.window;
                    const uint32_t nd = (uint32_t)wd[l] - b.window - 3u;
                    gst(p, ':'); gst(p + 1, ' ');
                    mf_put_u64(p + 2, node[l], nd);
                    gst(p + 2 + nd, '\n');
                }
            }
            pos += (uint32_t)uni(wave_sum(wd));
        }
        return pos;
    }
    const MfCounts c = mf_counts<true>(b, q);
    if (b.format == MF_COUNT_KMERS) {
        // header '\t' discovered '/' kmers '/' unique '\n'
        mf_copy_wave(out, b.headers + hb, hlen);
        const uint32_t n1 = tf_digits(c.n_discovered), n2 = tf_digits(c.n_kmers), n3 = tf_digits(c.n_unique);
        FOR_LANES(l) {
            if (l == 0) {
                char *p = out + hlen;
                gst(p, '\t'); tf_put_u32(p + 1, c.n_discovered, n1);
                p += 1 + n1;
                gst(p, '/'); tf_put_u32(p + 1, c.n_kmers, n2);
                p += 1 + n2;
                gst(p, '/'); tf_put_u32(p + 1, c.n_unique, n3);
                gst(p + 1 + n3, '\n');
            }
        }
        return hlen + 4u + n1 + n2 + n3;
    }
    if (b.format == MF_FILTER_PRESENT) {
        if (!mf_present<true>(b, c, qlen)) return 0;
        FOR_LANES(l) { if (l == 0) { gst(out, '>'); gst(out + 1 + hlen, '\n'); gst(out + 2 + hlen + qlen, '\n'); } }
        mf_copy_wave(out + 1, b.headers + hb, hlen);
        mf_copy_wave(out + 2 + hlen, b.seqs + sb, qlen);
        return hlen + qlen + 3u;
    }
    return 0;
}

} // namespace mgx
