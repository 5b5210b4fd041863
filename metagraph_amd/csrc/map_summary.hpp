// map_summary.hpp — per-read summary of DeBruijnGraph::map_to_nodes as `metagraph align --map` prints it
// (cli/align.cpp:134-164): n_discovered (non-zero nodes), n_kmers, n_unique (distinct non-zero nodes).
//
// Written against the wave interface (wave.hpp): tests/test_map_summary_model.py compiles this very file for the host
// (tests/emu/wave.hpp) and compares it with a std::set brute force.  One wavefront per read.  The node of k-mer i is made
// from the device mappings by the graph mode's rule (ms_node); the ids of the read then go through a bitonic sorting network
// in a buffer the caller places in LDS, neighbours are compared and the ballots' population counts add up to n_unique.
//   short form  n <= MS_SHORT_MAX k-mers: one sort of the whole read (a 150-bp read: 256 slots, 4 per lane);
//   long form   any n: chunks of MS_CHUNK ids are sorted in LDS and kept, sorted, in a scratch row of global memory; an id of
//               chunk c is new if it differs from its left neighbour and a binary search finds it in none of the chunks before c.
// Counts are exact for every length; nothing is counted with atomics.
#pragma once
#include "wave.hpp"
#include "dev_graph.hpp"

namespace mgx {

enum { MS_MODE_BASIC = 0, MS_MODE_CANONICAL = 1, MS_MODE_PRIMARY = 2 };      // = MGX_MODE_*
constexpr int32_t MS_SHORT_MAX = 256;        // k-mers per read of the short form (4 per lane)
constexpr int32_t MS_CHUNK = 4096;           // ids per sorted chunk of the long form (16 KiB of LDS per wavefront)

struct MsCounts { uint32_t n_discovered, n_kmers, n_unique; };

// What the rules read.  fwd / rc: the read's slices of the mapping kernels' node arrays (rc is not read in BASIC mode).
struct MsRead {
    const uint32_t *fwd, *rc;
    int32_t n;                   // k-mers (or windows) of the read
    int mode;                    // MS_MODE_*
    uint32_t n_edges;            // PRIMARY: ids above it are the wrapper's reverse-complement ids
    const uint64_t *valid;       // CANONICAL: the node mask, applied after the minimum (null: none)
};

// node of k-mer i (DBGSuccinct::map_to_nodes, dbg_succinct.cpp:436-497; CanonicalDBG::get_base_node, canonical_dbg.cpp:148-154)
MGX_DEV uint32_t ms_node(const MsRead &r, int32_t i) {
    const uint32_t f = gld(r.fwd + i);
    if (r.mode == MS_MODE_CANONICAL) {
        // the smaller BOSS index of the k-mer and its reverse complement, 0 if either look-up found nothing; then validate_edge
        const uint32_t c = gld(r.rc + (r.n - 1 - i));
        const uint32_t m = f < c ? f : c;
        if (m && r.valid && !((gld(r.valid + (m >> 6)) >> (m & 63)) & 1)) return 0u;
        return m;
    }
    if (r.mode == MS_MODE_PRIMARY) return f > r.n_edges ? f - r.n_edges : f;
    return f;
}

MGX_DEV int32_t ms_pow2_at_least(int32_t n) { int32_t p = 64; while (p < n) p <<= 1; return p; }

// ascending bitonic sort of buf[0 .. N), N a power of two >= 64: every lane takes the pairs lane, lane + 64, ...
MGX_DEV void ms_sort(uint32_t *buf, int32_t N) {
    for (int32_t size = 2; size <= N; size <<= 1)
        for (int32_t stride = size >> 1; stride >= 1; stride >>= 1) {
            wave_sync();
            FOR_LANES(l) {
                for (int32_t p = l; p < (N >> 1); p += WAVE) {
                    const int32_t lo = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const uint32_t a = buf[lo], b = buf[hi];
                    if ((a > b) == up) { buf[lo] = b; buf[hi] = a; }
                }
            }
        }
    wave_sync();
}

// is id in the ascending array s[0 .. n)?
MGX_DEV bool ms_find(const uint32_t *s, int32_t n, uint32_t id) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (gld(s + mid) < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && gld(s + lo) == id;
}

// Short form.  buf: MS_SHORT_MAX words of LDS owned by this wavefront; out (optional): the read's slice of the merged array.
MGX_DEV MsCounts ms_summary_short(const MsRead &r, uint32_t *buf, uint64_t *out) {
    const int32_t N = ms_pow2_at_least(r.n);
    int32_t found = 0;
    wave_sync();                                 // (the buffer's last reader of the previous read is through)
    FOR_LANES(l) {
        for (int32_t i = l; i < N; i += WAVE) {
            const uint32_t v = i < r.n ? ms_node(r, i) : 0u;
            buf[i] = v;
            if (i < r.n && out) gst(out + i, (uint64_t)v);
        }
    }
    ms_sort(buf, N);
    int32_t uniq = 0;
    for (int32_t base = 0; base < N; base += WAVE) {
        LV<bool> nz, nw;
        FOR_LANES(l) {
            const int32_t i = base + l;
            const uint32_t v = buf[i];
            nz[l] = v != 0;
            nw[l] = v != 0 && (i == 0 || buf[i - 1] != v);
        }
        found += popc64(wave_ballot(nz));
        uniq += popc64(wave_ballot(nw));
    }
    MsCounts c = { (uint32_t)found, (uint32_t)r.n, (uint32_t)uniq };
    return c;
}

// Long form.  buf: MS_CHUNK words of LDS; sorted: r.n words of global scratch owned by this read.
MGX_DEV MsCounts ms_summary_long(const MsRead &r, uint32_t *buf, uint32_t *sorted, uint64_t *out) {
    int32_t found = 0, uniq = 0;
    for (int32_t c0 = 0; c0 < r.n; c0 += MS_CHUNK) {
        const int32_t cn = r.n - c0 < MS_CHUNK ? r.n - c0 : MS_CHUNK;
        const int32_t N = ms_pow2_at_least(cn);
        wave_sync();
        FOR_LANES(l) {
            for (int32_t i = l; i < N; i += WAVE) {
                const uint32_t v = i < cn ? ms_node(r, c0 + i) : 0u;
                buf[i] = v;
                if (i < cn && out) gst(out + c0 + i, (uint64_t)v);
            }
        }
        ms_sort(buf, N);
        // the zeros (missing k-mers and the padding) sort to the front: the chunk's ids are buf[N - nz .. N)
        int32_t nz = 0;
        for (int32_t base = 0; base < N; base += WAVE) {
            LV<bool> p;
            FOR_LANES(l) p[l] = buf[base + l] != 0;
            nz += popc64(wave_ballot(p));
        }
        found += nz;
        for (int32_t base = N - nz; base < N; base += WAVE) {
            LV<bool> nw;
            FOR_LANES(l) {
                const int32_t i = base + l;
                bool fresh = false;
                if (i < N) {
                    const uint32_t v = buf[i];
                    fresh = i == N - nz || buf[i - 1] != v;
                    // the chunks before this one lie in `sorted`, chunk by chunk, zeros in front
                    for (int32_t p0 = 0; fresh && p0 < c0; p0 += MS_CHUNK) fresh = !ms_find(sorted + p0, MS_CHUNK, v);
                    gst(sorted + c0 + (i - (N - cn)), v);
                }
                nw[l] = fresh;
            }
            uniq += popc64(wave_ballot(nw));
        }
        // (a full chunk has N == cn: every slot of it is written above or is a zero)
        FOR_LANES(l) {
            for (int32_t i = N - cn + l; i < N - nz; i += WAVE) gst(sorted + c0 + (i - (N - cn)), 0u);
        }
    }
    MsCounts c = { (uint32_t)found, (uint32_t)r.n, (uint32_t)uniq };
    return c;
}

// ------------------------------------------------------------------------------------------------
// map_length L < k (cli/align.cpp:114-131): the node of one window = the first node that
// call_nodes_with_suffix_matching_longest_prefix(window, ., L) reports (dbg_succinct.cpp:307-393, unbounded branch), 0 if the
// window holds a character outside ACGT, matches over fewer than L characters or only nodes outside the mask.
// The look-up is the suffix seeder's (seed_lane.hpp, sl_index_range and the enumeration behind it) on the read's bytes.
// ------------------------------------------------------------------------------------------------
MGX_DEV uint32_t ms_code(char ch) {                  // KmerExtractorBOSS::encode: 1 .. 4 = ACGT (U = T, either case), 0 = anything else
    switch (ch) {
        case 'A': case 'a': return 1;
        case 'C': case 'c': return 2;
        case 'G': case 'g': return 3;
        case 'T': case 't': case 'U': case 'u': return 4;
        default: return 0;
    }
}

MGX_DEV uint32_t ms_subk_node(const DevGraph &g, const char *w, int32_t len, LineCtr &ctr) {
    uint32_t key = 0;
    const int32_t pl = (int32_t)g.prefix_len;
    for (int32_t t = 0; t < len; ++t) {
        const uint32_t c = ms_code(gld(w + t));
        if (!c) return 0u;
        if (t < pl) key |= (c - 1u) << (2 * t);
    }
    uint64_t rl = 1, ru = 0;
    int32_t it = 1;
    if (pl && pl <= len) {
        prefix_range(g, key, &rl, &ru, ctr);
        if (rl > ru) return 0u;                      // no node's suffix spells the first pl characters
        it = pl;
    } else {
        initial_range(g, ms_code(gld(w)), &rl, &ru);
        if (rl > ru) return 0u;
    }
    for (; it < len; ++it)
        if (!tighten_range(g, &rl, &ru, ms_code(gld(w + it)), ctr)) return 0u;
    // BOSS::index_range's (first, last) = (succ_last(rl), ru); the nodes between them in rank order, each node's incoming
    // edges in the order of call_incoming_to_target, the first one inside the mask
    const uint64_t first = succ_last(g, rl, ctr), last = ru;
    const uint32_t r_begin = first == last ? 0u : rank_last(g, first, ctr);
    const uint32_t r_end = first == last ? 0u : rank_last(g, last, ctr);
    for (uint32_t r = r_begin; r <= r_end; ++r) {
        const uint64_t e = first == last ? first : select_last(g, r, ctr);
        uint64_t inc[5];
        uint32_t fc[5];
        if (incoming<false, false>(g, e, inc, fc, ctr) > 0) return (uint32_t)inc[0];
    }
    return 0u;
}

} // namespace mgx
