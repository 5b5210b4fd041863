// results_decode.hpp — the structured results of an alignment batch in the layout of mgx_results (include/mgx.h), from what
// mgx_align_batch_device leaves in device memory: the ReadResult records and the output stream (align_types.hpp:51-64,
// host_common.hpp:153-159).  What HostResults::decode (host_common.hpp) does with one thread and one push_back per path node,
// CIGAR run and label.
//
// Written against the wave interface (wave.hpp): tests/test_results_decode_model.py compiles this very file for the host
// (tests/emu/wave.hpp) and compares its seven arrays, byte for byte, with mgx_results_from_raw_labeled's.  Two passes:
//   size    rd_query_counts: one query per lane walks the query's alignments and adds up what they take in five arrays
//           (alignments, nodes, CIGAR runs, path characters, labels); five exclusive scans over the batch (the caller's) turn
//           the counts into per-query begins.  The scanned alignment counts are mgx_results.aln_begin.
//   write   rd_write_query: one wavefront per query.  Nodes (widened to 64 bits), CIGAR runs (split into length and operator)
//           and labels are lane-strided; the path characters go through tf_copy, whose dword stores touch only dwords that are
//           wholly the copy's own, so that the bytes of the neighbouring queries are never raced.  num_matches is a wavefront
//           sum; the 72-byte record is lane 0's.
// A record with a status other than ST_OK (the device records are pre-retry) or without alignments takes no room anywhere:
// its query has its status and aln_begin[q] == aln_begin[q + 1].
#pragma once
#include "wave.hpp"
#include "tsv_format.hpp"

namespace mgx {

// mgx_cigar_op and mgx_alignment as the device writes them (mgx_results.hip asserts sizes and offsets against include/mgx.h)
struct RdCigarOp { uint32_t len; uint8_t op; uint8_t pad[3]; };
struct RdAlignment {
    int32_t score;
    uint32_t offset, clipping, end_clipping, num_matches, n_nodes, n_cigar, seq_len;
    uint64_t nodes_begin, cigar_begin, seq_begin;
    uint8_t orientation;
    uint8_t pad[3];
    uint32_t n_labels;
    uint64_t labels_begin;
};
static_assert(sizeof(RdCigarOp) == 8 && sizeof(RdAlignment) == 72, "record layout");

// the five arrays a query's alignments take room in: the order of counts / begins (and of mgx_results_sizes)
enum RdArray { RD_ALN = 0, RD_NODES, RD_CIGAR, RD_SEQ, RD_LABELS, RD_ARRAYS };

struct RdBatch {
    const ReadResult *results;
    const uint32_t *stream;
    uint64_t *counts;                // size pass: array x of query q at counts[x * stride + q], q <= n_queries (the last one: 0)
    const uint64_t *begins;          // write pass: the exclusive sums of counts, same shape; begins[RD_ALN * stride ..] is aln_begin
    RdAlignment *alignments;
    uint64_t *nodes;
    RdCigarOp *cigar;
    char *seqs;
    int32_t *status;                 // n_queries
    uint32_t *labels;
    uint64_t n_queries;
    uint64_t stride;                 // >= n_queries + 1
    uint32_t labeled;                // the stream carries a label list behind every alignment
    uint32_t pad;
};

// ---- size pass: what query q adds to the five arrays (q == n_queries: the scan's closing zeros) ---------------------------------
MGX_DEV void rd_query_counts(const RdBatch &b, uint64_t q) {
    uint64_t c[RD_ARRAYS] = { 0, 0, 0, 0, 0 };
    if (q < b.n_queries) {
        const ReadResult r = tf_record_at<false>(b.results + q);
        if (tf_has_alignments(r)) {
            TfBatch t = {};
            t.stream = b.stream;
            uint64_t at = r.stream_off;
            for (int32_t a = 0; a < r.n_alignments; ++a) {
                const TfAln h = tf_aln_header<false>(t, r, a, &at);
                c[RD_NODES] += h.n_nodes; c[RD_CIGAR] += h.n_cigar; c[RD_SEQ] += h.seq_len;
                at += (uint64_t)h.n_nodes + h.n_cigar + ((uint64_t)h.seq_len + 3) / 4;
                if (b.labeled) {
                    const uint32_t nl = gld(b.stream + at);
                    c[RD_LABELS] += nl;
                    at += 1 + (uint64_t)nl;
                }
            }
            c[RD_ALN] = (uint64_t)r.n_alignments;
        }
    }
    for (int x = 0; x < RD_ARRAYS; ++x) gst(b.counts + (uint64_t)x * b.stride + q, c[x]);
}

// ---- write pass: status[q] and the alignments of query q at begins[.][q]; the whole wavefront (q is wave-uniform) ------------
MGX_DEV void rd_write_query(const RdBatch &b, uint64_t q) {
    const ReadResult r = tf_record_at<true>(b.results + q);
    FOR_LANES(l) { if (l == 0) gst(b.status + q, r.status); }
    if (!tf_has_alignments(r)) return;
    uint64_t ai = tf_ld<true>(b.begins + (uint64_t)RD_ALN * b.stride + q), np = tf_ld<true>(b.begins + (uint64_t)RD_NODES * b.stride + q),
             cp = tf_ld<true>(b.begins + (uint64_t)RD_CIGAR * b.stride + q), sp = tf_ld<true>(b.begins + (uint64_t)RD_SEQ * b.stride + q),
             lp = tf_ld<true>(b.begins + (uint64_t)RD_LABELS * b.stride + q);
    TfBatch t = {};
    t.stream = b.stream;
    uint64_t at = r.stream_off;
    for (int32_t a = 0; a < r.n_alignments; ++a) {
        const TfAln h = tf_aln_header<true>(t, r, a, &at);
        const uint32_t *nd = b.stream + at, *cg = nd + h.n_nodes;
        FOR_LANES(l) {
            for (uint32_t x = (uint32_t)l; x < h.n_nodes; x += WAVE) gst(b.nodes + np + x, (uint64_t)gld(nd + x));
        }
        // the runs: {len, op, 0, 0, 0} as one 8-byte store, a lane per run; num_matches (host_common.hpp:187-197) on the way
        uint32_t matches = 0;
        for (uint32_t base = 0; base < h.n_cigar; base += WAVE) {
            LV<int32_t> m;
            FOR_LANES(l) {
                const uint32_t x = base + (uint32_t)l;
                m[l] = 0;
                if (x < h.n_cigar) {
                    const uint32_t w = gld(cg + x);
                    gst(reinterpret_cast<uint64_t *>(b.cigar + cp + x), (uint64_t)(w >> 3) | ((uint64_t)(w & 7u) << 32));
                    if ((w & 7u) == OP_MATCH) m[l] = (int32_t)(w >> 3);
                }
            }
            matches += (uint32_t)uni(wave_sum(m));
        }
        uint32_t clipping = 0, end_clipping = 0;
        if (h.n_cigar) {
            const uint32_t f = tf_ld<true>(cg), e = tf_ld<true>(cg + h.n_cigar - 1);
            clipping = (f & 7u) == OP_CLIPPED ? f >> 3 : 0u;
            end_clipping = (e & 7u) == OP_CLIPPED ? e >> 3 : 0u;
        }
        tf_copy(b.seqs + sp, reinterpret_cast<const char *>(cg + h.n_cigar), h.seq_len, false);
        at += (uint64_t)h.n_nodes + h.n_cigar + ((uint64_t)h.seq_len + 3) / 4;
        uint32_t nl = 0;
        if (b.labeled) {
            nl = tf_ld<true>(b.stream + at);
            const uint32_t *lb = b.stream + at + 1;
            FOR_LANES(l) {
                for (uint32_t x = (uint32_t)l; x < nl; x += WAVE) gst(b.labels + lp + x, gld(lb + x));
            }
            at += 1 + (uint64_t)nl;
        }
        // the record: all 72 bytes, padding included, as nine 8-byte words (little endian, like everything here)
        FOR_LANES(l) {
            if (l == 0) {
                uint64_t *p = reinterpret_cast<uint64_t *>(b.alignments + ai);
                gst(p + 0, (uint64_t)(uint32_t)h.score | ((uint64_t)h.offset << 32));
                gst(p + 1, (uint64_t)clipping | ((uint64_t)end_clipping << 32));
                gst(p + 2, (uint64_t)matches | ((uint64_t)h.n_nodes << 32));
                gst(p + 3, (uint64_t)h.n_cigar | ((uint64_t)h.seq_len << 32));
                gst(p + 4, np);
                gst(p + 5, cp);
                gst(p + 6, sp);
                gst(p + 7, (uint64_t)(h.orientation & 0xFFu) | ((uint64_t)nl << 32));
                gst(p + 8, b.labeled ? lp : (uint64_t)0);
            }
        }
        ai += 1; np += h.n_nodes; cp += h.n_cigar; sp += h.seq_len; lp += nl;
    }
}

} // namespace mgx
