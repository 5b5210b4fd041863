// tests/emu/tsv_format_check.cpp — TEST ONLY: metagraph_amd/csrc/tsv_format.hpp (the size and the write pass of the batched TSV
// formatter) under the host wave model on random records.  It dumps records, stream, reads, headers, names and the text it
// produced; tests/test_tsv_format_model.py decodes the same records with mgx_results_from_raw_labeled and compares the text with
// mgx_format_tsv_labeled's.  usage: tsv_format_check <out-prefix>  ->  <out-prefix>.<variant>.bin
#include "wave.hpp"
#include "../../metagraph_amd/csrc/tsv_format.hpp"

#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace mgx;

template <class T> static void put(FILE *f, const std::vector<T> &v, size_t n) { if (n) fwrite(v.data(), sizeof(T), n, f); }

static bool variant(const std::string &path, uint64_t seed, bool labeled, int n_names, int32_t min_path_score) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const uint64_t n = 400;
    std::vector<ReadResult> rec(n);
    std::vector<uint32_t> stream;
    std::vector<uint64_t> offsets(1, 0), hoff(1, 0);
    std::string seqs, headers, names;
    std::vector<uint32_t> name_begin(1, 0);
    static const char *const some_names[] = { "strain_A", "", "x", "a-rather-long-label-name/with.punctuation", "B2", "sample;7", "q", "zz" };
    for (int i = 0; i < n_names; ++i) { names += some_names[i % 8]; name_begin.push_back((uint32_t)names.size()); }
    // run lengths of 1 .. 5 digits (and beyond, now and then)
    auto run_len = [&]() -> uint32_t {
        static const uint32_t lim[] = { 10, 100, 1000, 10000, 100000, 1u << 29 };
        const int d = (int)rnd(100) < 3 ? 5 : (int)rnd(5);
        const uint32_t lo = d ? lim[d - 1] : 1;
        return lo + (uint32_t)rnd(lim[d] - lo);
    };
    static const char qchars[] = "ACGTacgtNnRyx\x80\xff\xc3\x7f@[`{~ 09";
    uint64_t cap_query = 137;
    for (uint64_t q = 0; q < n; ++q) {
        // the query: upper and lower case, N, bytes >= 0x80, length 0 now and then
        const uint32_t qlen = q % 29 == 3 ? 0 : (uint32_t)rnd(q % 7 == 0 ? 700 : 180);
        for (uint32_t i = 0; i < qlen; ++i) seqs += qchars[rnd(sizeof(qchars) - 1)];
        offsets.push_back(seqs.size());
        const uint32_t hlen = q % 11 == 0 ? 0 : q % 13 == 0 ? 1000 : (uint32_t)rnd(40);
        for (uint32_t i = 0; i < hlen; ++i) headers += (char)(33 + rnd(94));
        hoff.push_back(headers.size());
        ReadResult &r = rec[q];
        memset(&r, 0, sizeof(r));
        r.n_alignments = qlen == 0 ? 0 : (int32_t)rnd(5);
        r.status = ST_OK;
        if (q == cap_query) { r.status = ST_CAPACITY; r.n_alignments = 2; r.orientation = 0; }      // (what it points to is never read)
        r.stream_off = stream.size();
        if (r.status != ST_OK) continue;
        for (int32_t a = 0; a < r.n_alignments; ++a) {
            const int32_t score = (int32_t)rnd(7) == 0 ? -(int32_t)rnd(100000) : (int32_t)rnd(3000);
            const uint32_t offset = (uint32_t)rnd(4) ? (uint32_t)rnd(31) : (uint32_t)rnd(1u << 31);
            const uint32_t n_nodes = (uint32_t)rnd(6), n_cigar = (uint32_t)rnd(20) == 0 ? 64 + (uint32_t)rnd(140) : (uint32_t)rnd(12);
            const uint32_t seq_len = (uint32_t)rnd(9) == 0 ? 0 : (uint32_t)rnd(320), orientation = (uint32_t)rnd(2);
            if (a == 0) { r.score = score; r.offset = offset; r.n_nodes = n_nodes; r.n_cigar = n_cigar; r.seq_len = seq_len; r.orientation = orientation; }
            else for (uint32_t w : { (uint32_t)score, offset, n_nodes, n_cigar, seq_len, orientation }) stream.push_back(w);
            for (uint32_t x = 0; x < n_nodes; ++x) stream.push_back((uint32_t)rng());
            for (uint32_t x = 0; x < n_cigar; ++x) stream.push_back(run_len() << 3 | (uint32_t)rnd(6));
            std::string path;
            for (uint32_t x = 0; x < seq_len; ++x) path += "ACGTN$"[rnd(6)];
            path.resize((seq_len + 3) / 4 * 4, '#');                      // (padding: must never be printed)
            for (size_t x = 0; x < path.size(); x += 4) { uint32_t w; memcpy(&w, path.data() + x, 4); stream.push_back(w); }
            if (labeled) {
                const uint32_t nl = (uint32_t)rnd(25) == 0 ? 64 + (uint32_t)rnd(80) : (uint32_t)rnd(5);
                stream.push_back(nl);
                // numbers below and above the name count
                for (uint32_t x = 0; x < nl; ++x) stream.push_back((uint32_t)rnd(3) ? (uint32_t)rnd(12) : (uint32_t)rng());
            }
        }
    }
    const uint64_t stream_words = stream.size();
    // the copies read the aligned dwords around their source: room behind every array
    seqs.append(8, '!'); headers.append(8, '!'); names.append(8, '!');
    stream.push_back(0x23232323u);

    std::vector<uint64_t> line_len(n + 1, 0), line_begin(n + 1, 0);
    std::vector<uint32_t> cap_list(n, 0);
    unsigned long long cap_count = 0;
    TfBatch b;
    memset(&b, 0, sizeof(b));
    b.results = rec.data(); b.stream = stream.data(); b.seqs = seqs.data(); b.offsets = offsets.data();
    b.headers = headers.data(); b.header_offsets = hoff.data();
    b.name_bytes = n_names ? names.data() : nullptr; b.name_begin = n_names ? name_begin.data() : nullptr;
    b.line_len = line_len.data(); b.line_begin = line_begin.data();
    b.cap_list = cap_list.data(); b.cap_count = &cap_count;
    b.n_queries = n; b.n_names = (uint32_t)n_names; b.min_path_score = min_path_score; b.labeled = labeled ? 1 : 0;
    for (uint64_t q = 0; q < n; ++q) line_len[q] = tf_line_size(b, q);                   // size pass: a query per lane
    for (uint64_t q = 0; q < n; ++q) line_begin[q + 1] = line_begin[q] + line_len[q];    // the scan
    const char guard = (char)0xA5;
    // the text at every 4-byte alignment of its start (the write pass aligns its stores to the destination)
    std::vector<char> text;
    for (int shift = 0; shift < 4; ++shift) {
        std::vector<char> buf(line_begin[n] + 16, guard);
        b.text = buf.data() + 4 + shift - ((uintptr_t)buf.data() & 3);
        for (uint64_t q = 0; q < n; ++q) {
            const uint64_t wrote = tf_write_line(b, q);                                  // write pass: a wavefront per query
            if (wrote != line_len[q]) { printf("FAIL query %llu: size pass %llu, write pass %llu\n", (unsigned long long)q, (unsigned long long)line_len[q], (unsigned long long)wrote); return false; }
        }
        if (b.text[-1] != guard || b.text[line_begin[n]] != guard) { printf("FAIL: a byte outside the text was written (shift %d)\n", shift); return false; }
        std::vector<char> t(b.text, b.text + line_begin[n]);
        if (shift && t != text) { printf("FAIL: the text depends on its alignment (shift %d)\n", shift); return false; }
        text.swap(t);
    }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint64_t hdr[10] = { n, labeled ? 1u : 0u, stream_words, offsets[n], hoff[n], (uint64_t)n_names, name_begin.back(), line_begin[n],
                               cap_count, (uint64_t)(int64_t)min_path_score };
    fwrite(hdr, 8, 10, f);
    put(f, rec, n); put(f, stream, stream_words); put(f, offsets, n + 1);
    fwrite(seqs.data(), 1, offsets[n], f);
    put(f, hoff, n + 1);
    fwrite(headers.data(), 1, hoff[n], f);
    put(f, name_begin, name_begin.size());
    fwrite(names.data(), 1, name_begin.back(), f);
    put(f, line_begin, n + 1); put(f, text, text.size()); put(f, cap_list, cap_count);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    static_assert(sizeof(ReadResult) == 64, "record layout");
    // the four-byte normalisation against the one-byte rule, every byte value in every position
    for (uint32_t c = 0; c < 256; ++c)
        for (int pos = 0; pos < 4; ++pos) {
            const uint32_t others = 0x61804100u, w = (others & ~(0xFFu << (8 * pos))) | (c << (8 * pos));
            uint32_t want = 0;
            for (int x = 0; x < 4; ++x) want |= (uint32_t)(uint8_t)tf_norm1((char)(w >> (8 * x))) << (8 * x);
            if (tf_norm4(w) != want) { printf("FAIL tf_norm4(%08x) = %08x, want %08x\n", w, tf_norm4(w), want); return 1; }
        }
    const std::string prefix = argv[1];
    if (!variant(prefix + ".plain.bin", 20250101, false, 0, -37)) return 1;
    if (!variant(prefix + ".labeled.bin", 20250102, true, 6, 0)) return 1;
    if (!variant(prefix + ".labeled_numbers.bin", 20250103, true, 0, 12345)) return 1;
    printf("ok 3 variants\n");
    return 0;
}
