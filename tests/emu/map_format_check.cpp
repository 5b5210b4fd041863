// tests/emu/map_format_check.cpp — TEST ONLY: metagraph_amd/csrc/map_format.hpp (the size and the write pass of the batched
// `align --map` formatter) under the host wave model.  It builds count records, node arrays, reads and headers, runs both passes
// the way the kernels of mgx_mapfmt.hip do, and dumps the inputs and the text; tests/test_map_format_model.py formats the same
// data with mgx_format_map / mgx_map_present and compares.  usage: map_format_check <out-prefix>  ->  <out-prefix>.<name>.bin
//
// A dump: 12 u64 (n, format, k, map_length, nodes, seq bytes, header bytes, text bytes, the fraction's bits, 3 x 0), then counts
// (12 n), node_begin (8 (n + 1)), nodes, offsets (8 (n + 1)), seqs, header_offsets (8 (n + 1)), headers, line_begin (8 (n + 1)), text.
#include "wave.hpp"
#include "../../metagraph_amd/csrc/map_format.hpp"

#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace mgx;

struct World {
    uint32_t k = 31, map_length = 0;
    std::vector<uint32_t> counts;                 // 3 per query
    std::vector<uint64_t> node_begin{ 0 }, nodes, offsets{ 0 }, hoff{ 0 };
    std::string seqs, headers;
    uint64_t n() const { return offsets.size() - 1; }
    uint32_t window() const { return map_length && map_length < k ? map_length : k; }
    void add(const std::string &header, const std::string &seq, uint64_t n_windows, uint32_t d, uint32_t nk, uint32_t u) {
        headers += header; hoff.push_back(headers.size());
        seqs += seq; offsets.push_back(seqs.size());
        node_begin.push_back(node_begin.back() + n_windows);
        counts.push_back(d); counts.push_back(nk); counts.push_back(u);
    }
};

template <class T> static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// both passes as k_mapfmt_size / k_mapfmt_write run them (a wavefront per query; QUERY_PRESENCE and the sizes of the formats
// without nodes a lane per query), the exclusive scan in between; dumps the world and the text
static bool run(const std::string &path, World &w, int format, double fraction) {
    const uint64_t n = w.n();
    const bool sub_k = w.map_length && w.map_length < w.k;
    uint32_t max_kmers = 0;
    for (uint64_t q = 0; q < n; ++q) max_kmers = std::max(max_kmers, w.counts[3 * q + 1]);
    const bool presence = format == MF_QUERY_PRESENCE || format == MF_FILTER_PRESENT;
    if (!presence) max_kmers = 0;
    std::vector<uint64_t> threshold((size_t)max_kmers + 1);
    for (size_t i = 0; i <= max_kmers; ++i) threshold[i] = mf_threshold_host(i, fraction, sub_k);
    // the reads and headers with the room behind them the device buffers have (whole dwords are read)
    std::vector<char> seqs(w.seqs.begin(), w.seqs.end()), headers(w.headers.begin(), w.headers.end());
    seqs.resize(seqs.size() + 16, 'Z'); headers.resize(headers.size() + 16, 'Z');
    std::vector<uint64_t> nodes = w.nodes;
    nodes.resize(nodes.size() + 1);
    std::vector<uint32_t> counts = w.counts;
    counts.resize(counts.size() + 3);
    std::vector<uint64_t> len(n + 1, 0), begin(n + 1, 0);
    MfBatch b;
    memset(&b, 0, sizeof(b));
    b.counts = counts.data(); b.nodes = nodes.data(); b.node_begin = w.node_begin.data();
    b.seqs = seqs.data(); b.offsets = w.offsets.data(); b.headers = headers.data(); b.header_offsets = w.hoff.data();
    b.threshold = threshold.data(); b.line_len = len.data(); b.line_begin = begin.data();
    b.n_queries = n; b.max_kmers = max_kmers; b.k = w.k; b.window = w.window(); b.sub_k = sub_k; b.format = format;
    for (uint64_t q = 0; q < n; ++q) len[q] = format == MF_NODES ? mf_nodes_size(b, q) : mf_line_size(b, q);
    for (uint64_t q = 0; q < n; ++q) begin[q + 1] = begin[q] + len[q];
    // (guard bytes around the text: a store outside a line's span shows)
    const uint64_t total = begin[n];
    std::vector<char> text(total + 64, '#');
    b.text = text.data() + 32;
    for (uint64_t q = 0; q < n; ++q) {
        if (format == MF_QUERY_PRESENCE) mf_write_presence(b, q);
        else if (mf_write_line(b, q) != len[q]) { fprintf(stderr, "%s: query %llu: the write pass disagrees with the size pass\n", path.c_str(), (unsigned long long)q); return false; }
    }
    for (int i = 0; i < 32; ++i)
        if (text[i] != '#' || text[32 + total + i] != '#') { fprintf(stderr, "%s: a store outside the text\n", path.c_str()); return false; }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    uint64_t fbits;
    memcpy(&fbits, &fraction, 8);
    const uint64_t hdr[12] = { n, (uint64_t)format, w.k, w.map_length, w.nodes.size(), w.seqs.size(), w.headers.size(), total, fbits, 0, 0, 0 };
    fwrite(hdr, 8, 12, f);
    put(f, w.counts); put(f, w.node_begin); put(f, w.nodes); put(f, w.offsets);
    fwrite(w.seqs.data(), 1, w.seqs.size(), f);
    put(f, w.hoff);
    fwrite(w.headers.data(), 1, w.headers.size(), f);
    put(f, begin);
    fwrite(text.data() + 32, 1, total, f);
    fclose(f);
    return true;
}

// nodes at every digit-count boundary: 0, 9 / 10, 99 / 100, ... up to 10^19, and 2^64 - 1
static std::vector<uint64_t> boundary_nodes() {
    std::vector<uint64_t> v{ 0, 1, 5, 0xFFFFFFFFull, 0x100000000ull, 18446744073709551615ull, 12345678901234567890ull };
    uint64_t p = 10;
    for (int i = 1; i <= 19; ++i) { v.push_back(p - 1); v.push_back(p); v.push_back(p + 1); if (i < 19) p *= 10; }
    return v;
}

// reads with 0, 1, 63, 64, 65, 256, 257 and about 5000 windows (and every count below 70), headers of every length 0 .. 7 and one
// of 1000 bytes, read bytes with lower case, N and bytes >= 0x80; presence worlds carry consistent counts, the others any
static World text_world(uint32_t k, uint32_t map_length, uint64_t seed, bool consistent_counts) {
    World w;
    w.k = k; w.map_length = map_length;
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    static const char qchars[] = "ACGTacgtNnRyx\x80\xff\xc3\x7f@[`{~ 09";
    const std::vector<uint64_t> bn = boundary_nodes();
    const uint32_t window = w.window();
    std::vector<uint64_t> shapes{ 0, 1, 63, 64, 65, 256, 257, 5003 };
    for (uint64_t i = 2; i < 70; ++i) shapes.push_back(i);
    uint64_t node_at = 0;
    for (size_t s = 0; s < shapes.size(); ++s) {
        for (int rep = 0; rep < (shapes[s] > 300 ? 1 : 3); ++rep) {
            const uint64_t nw = shapes[s];
            // no window: an empty read, or one just too short; a window: nw + window - 1 characters
            uint64_t qlen = nw ? nw + window - 1 : (rep == 0 ? 0 : rnd(window));
            uint64_t declared = nw;
            if (nw && rep == 2) { declared = nw + 1 + rnd(5); }             // more node slots than windows fit: the formatter's guard cuts them
            std::string seq;
            for (uint64_t i = 0; i < qlen; ++i) seq += qchars[rnd(sizeof(qchars) - 1)];
            const size_t q = w.n();
            const uint32_t hlen = q % 37 == 5 ? 1000 : (uint32_t)(q % 8);
            std::string header;
            for (uint32_t i = 0; i < hlen; ++i) header += (char)(33 + rnd(94));
            for (uint64_t i = 0; i < declared; ++i) w.nodes.push_back(rnd(3) ? bn[node_at++ % bn.size()] : rng() >> rnd(64));
            uint32_t d, nk, u;
            if (consistent_counts) { nk = (uint32_t)declared; d = (uint32_t)rnd(nk + 1); if (rnd(4) == 0) d = nk; u = d; }
            else {
                static const uint32_t lim[] = { 0, 9, 10, 99, 100, 999999999u, 1000000000u, 4294967295u };
                d = rnd(2) ? lim[rnd(8)] : (uint32_t)rng(); nk = rnd(2) ? lim[rnd(8)] : (uint32_t)rng(); u = rnd(2) ? lim[rnd(8)] : (uint32_t)rng();
            }
            w.add(header, seq, declared, d, nk, u);
        }
    }
    return w;
}

// every (n_discovered, n_kmers) with n_kmers <= 40 and the boundary set of tests/test_map_format.py up to 300; a query of n_kmers
// k-mers is n_kmers + window - 1 long (without k-mers: shorter than the window); plus queries shorter than k that carry counts
static World presence_world(uint32_t k, uint32_t map_length) {
    World w;
    w.k = k; w.map_length = map_length;
    const uint32_t window = w.window();
    for (uint32_t nk = 0; nk <= 300; ++nk) {
        std::vector<uint32_t> found;
        if (nk <= 40) for (uint32_t d = 0; d <= nk; ++d) found.push_back(d);
        else
            for (uint32_t d : { 0u, 1u, nk / 10, nk / 3, nk / 2, (7 * nk) / 10, (7 * nk + 9) / 10, (9 * nk) / 10, nk - 1, nk })
                if (d <= nk) found.push_back(d);
        for (uint32_t d : found) w.add("", std::string(nk ? nk + window - 1 : window - 1, 'A'), nk, d, nk, d);
    }
    for (uint32_t nk : { 1u, 5u, 40u }) w.add("", std::string(k - 1, 'C'), 0, nk, nk, nk);      // query_len < k whatever the counts say
    w.nodes.assign(w.node_begin.back(), 7);
    return w;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string prefix = argv[1];
    static const char *const fmt_name[] = { "nodes", "count", "presence", "filter" };
    static const uint32_t shapes[][2] = { { 31, 0 }, { 31, 21 }, { 31, 11 }, { 31, 3 }, { 11, 11 }, { 21, 0 } };      // k, map_length
    int dumps = 0;
    for (const auto &kl : shapes)
        for (int format = 0; format < 4; ++format) {
            const bool presence = format == MF_QUERY_PRESENCE || format == MF_FILTER_PRESENT;
            World w = text_world(kl[0], kl[1], 1000u * kl[0] + kl[1], presence);
            if (!run(prefix + ".k" + std::to_string(kl[0]) + "_l" + std::to_string(kl[1]) + "." + fmt_name[format] + ".bin", w, format, 0.7)) return 1;
            ++dumps;
        }
    // an empty batch, every format
    for (int format = 0; format < 4; ++format) {
        World w;
        if (!run(prefix + ".empty." + fmt_name[format] + ".bin", w, format, 0.7)) return 1;
        ++dumps;
    }
    // FILTER_PRESENT with nothing present: nothing is discovered and everything is asked for
    {
        World w = text_world(31, 0, 77, true);
        for (uint64_t q = 0; q < w.n(); ++q) { w.counts[3 * q] = 0; w.counts[3 * q + 2] = 0; if (!w.counts[3 * q + 1]) w.counts[3 * q + 1] = 1; }
        if (!run(prefix + ".nothing.filter.bin", w, MF_FILTER_PRESENT, 1.0)) return 1;
        ++dumps;
    }
    // presence: both formulas, seven fractions
    static const double fractions[] = { 0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0 };
    for (int fi = 0; fi < 7; ++fi)
        for (uint32_t map_length : { 0u, 7u }) {
            World w = presence_world(11, map_length);
            if (!run(prefix + ".present_f" + std::to_string(fi) + "_l" + std::to_string(map_length) + ".presence.bin", w, MF_QUERY_PRESENCE, fractions[fi])) return 1;
            ++dumps;
        }
    printf("ok %d dumps\n", dumps);
    return 0;
}
