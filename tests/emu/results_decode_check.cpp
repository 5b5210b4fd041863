// tests/emu/results_decode_check.cpp — TEST ONLY: metagraph_amd/csrc/results_decode.hpp (the size and the write pass of the
// on-device result decode) under the host wave model on random records.  It dumps records, stream and the seven arrays it
// produced; tests/test_results_decode_model.py decodes the same records with mgx_results_from_raw_labeled and compares them byte
// for byte.  usage: results_decode_check <out-prefix>  ->  <out-prefix>.<variant>.bin
#include "wave.hpp"
#include "../../metagraph_amd/csrc/results_decode.hpp"

#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace mgx;

template <class T> static void put(FILE *f, const std::vector<T> &v, size_t n) { if (n) fwrite(v.data(), sizeof(T), n, f); }

// an output array between two guard zones
template <class T>
struct Guarded {
    std::vector<unsigned char> raw;
    size_t n;
    explicit Guarded(size_t n_) : raw(n_ * sizeof(T) + 128, 0xA5), n(n_) {}
    T *data() { return reinterpret_cast<T *>(raw.data() + 64); }
    bool intact() const {
        for (size_t i = 0; i < 64; ++i) if (raw[i] != 0xA5 || raw[raw.size() - 1 - i] != 0xA5) return false;
        return true;
    }
    void dump(FILE *f) { if (n) fwrite(data(), sizeof(T), n, f); }
};

static bool variant(const std::string &path, uint64_t seed, bool labeled) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const uint64_t n = 300;
    std::vector<ReadResult> rec(n);
    std::vector<uint32_t> stream;
    for (uint64_t q = 0; q < n; ++q) {
        ReadResult &r = rec[q];
        memset(&r, 0, sizeof(r));
        r.status = ST_OK;
        r.n_alignments = q % 9 == 4 ? 0 : (int32_t)rnd(5);                               // (OK records without alignments among them)
        if (q == 5 && r.n_alignments == 0) r.n_alignments = 1;                            // (the query with the huge run, below)
        // the parity-test tail of the record: anything
        r.num_matches_fwd = (uint32_t)rng(); r.n_seeds_rc = (uint32_t)rng(); r.n_columns = (uint32_t)rng();
        if (q == 41 || q == n - 1) { r.status = ST_CAPACITY; r.n_alignments = 2; r.n_nodes = 7; r.n_cigar = 3; r.seq_len = 9; }   // (what it points to is never read)
        r.stream_off = stream.size();
        if (r.status != ST_OK) { r.stream_off = ~0ull >> 8; continue; }
        for (int32_t a = 0; a < r.n_alignments; ++a) {
            const int32_t score = (int32_t)rnd(5) == 0 ? -(int32_t)rnd(100000) - 1 : (int32_t)rnd(3000);
            const uint32_t offset = (uint32_t)rnd(4) ? (uint32_t)rnd(31) : (uint32_t)rng();
            const uint32_t n_nodes = (uint32_t)rnd(15) == 0 ? 65 + (uint32_t)rnd(500) : (uint32_t)rnd(8);
            uint32_t n_cigar = (uint32_t)rnd(15) == 0 ? 65 + (uint32_t)rnd(140) : (uint32_t)rnd(12);
            // path lengths 0 .. 3 and every remainder mod 4 often, so that seq_begin takes every alignment
            const uint32_t seq_len = (uint32_t)rnd(3) == 0 ? (uint32_t)rnd(4) : (uint32_t)rnd(320);
            const uint32_t orientation = (uint32_t)rnd(2);
            const bool huge_run = q == 5 && a == 0;                                      // one run of 2^29 - 1 characters
            if (huge_run && n_cigar < 2) n_cigar = 2;
            if (a == 0) { r.score = score; r.offset = offset; r.n_nodes = n_nodes; r.n_cigar = n_cigar; r.seq_len = seq_len; r.orientation = orientation; }
            else for (uint32_t w : { (uint32_t)score, offset, n_nodes, n_cigar, seq_len, orientation }) stream.push_back(w);
            for (uint32_t x = 0; x < n_nodes; ++x) stream.push_back((uint32_t)rng());
            const bool clip_front = rnd(3) == 0, clip_back = rnd(3) == 0;
            for (uint32_t x = 0; x < n_cigar; ++x) {
                uint32_t op = 1 + (uint32_t)rnd(5), len = 1 + (uint32_t)rnd((uint32_t)rnd(10) == 0 ? 100000 : 160);
                if ((x == 0 && clip_front) || (x + 1 == n_cigar && clip_back)) op = OP_CLIPPED;
                if (huge_run && x == 1) { op = OP_MATCH; len = (1u << 29) - 1; }
                stream.push_back(len << 3 | op);
            }
            std::string p;
            for (uint32_t x = 0; x < seq_len; ++x) p += "ACGTN$"[rnd(6)];
            p.resize((seq_len + 3) / 4 * 4, '#');                                        // (padding: must never be copied)
            for (size_t x = 0; x < p.size(); x += 4) { uint32_t w; memcpy(&w, p.data() + x, 4); stream.push_back(w); }
            if (labeled) {
                const uint32_t nl = (uint32_t)rnd(20) == 0 ? 65 + (uint32_t)rnd(80) : (uint32_t)rnd(4);      // (0: a labeled alignment without a label)
                stream.push_back(nl);
                uint32_t lbl = 0;
                for (uint32_t x = 0; x < nl; ++x) { lbl += 1 + (uint32_t)rnd(9); stream.push_back(lbl); }
            }
        }
    }
    const uint64_t stream_words = stream.size();
    stream.push_back(0x23232323u);           // the copies read the aligned dwords around their source: room behind the stream

    const uint64_t stride = n + 3;           // (not n + 1: the stride is the caller's)
    std::vector<uint64_t> counts(RD_ARRAYS * stride, 0xDEADBEEFull), begins(RD_ARRAYS * stride, 0);
    RdBatch b;
    memset(&b, 0, sizeof(b));
    b.results = rec.data(); b.stream = stream.data(); b.counts = counts.data(); b.begins = begins.data();
    b.n_queries = n; b.stride = stride; b.labeled = labeled ? 1 : 0;
    for (uint64_t q = 0; q <= n; ++q) rd_query_counts(b, q);                             // size pass: a query per lane
    uint64_t totals[RD_ARRAYS];
    for (int x = 0; x < RD_ARRAYS; ++x) {                                                // the scans
        uint64_t s = 0;
        if (counts[x * stride + n] != 0) { printf("FAIL: counts[%d][n] is not zero\n", x); return false; }
        for (uint64_t q = 0; q <= n; ++q) { begins[x * stride + q] = s; s += counts[x * stride + q]; }
        totals[x] = begins[x * stride + n];
    }
    Guarded<RdAlignment> alns(totals[RD_ALN]);
    Guarded<uint64_t> nodes(totals[RD_NODES]);
    Guarded<RdCigarOp> cigar(totals[RD_CIGAR]);
    Guarded<char> seqs(totals[RD_SEQ]);
    Guarded<int32_t> status(n);
    Guarded<uint32_t> labels(totals[RD_LABELS]);
    b.alignments = alns.data(); b.nodes = nodes.data(); b.cigar = cigar.data(); b.seqs = seqs.data(); b.status = status.data();
    b.labels = labels.data();
    for (uint64_t q = 0; q < n; ++q) rd_write_query(b, q);                               // write pass: a wavefront per query
    if (!alns.intact() || !nodes.intact() || !cigar.intact() || !seqs.intact() || !status.intact() || !labels.intact()) {
        printf("FAIL: a byte outside an output array was written\n");
        return false;
    }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint64_t hdr[8] = { n, labeled ? 1u : 0u, stream_words, totals[0], totals[1], totals[2], totals[3], totals[4] };
    fwrite(hdr, 8, 8, f);
    put(f, rec, n); put(f, stream, stream_words);
    fwrite(begins.data() + RD_ALN * stride, 8, n + 1, f);                                // aln_begin
    status.dump(f); alns.dump(f); nodes.dump(f); cigar.dump(f); seqs.dump(f); labels.dump(f);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    static_assert(sizeof(ReadResult) == 64, "record layout");
    const std::string prefix = argv[1];
    if (!variant(prefix + ".plain.bin", 20250201, false)) return 1;
    if (!variant(prefix + ".labeled.bin", 20250202, true)) return 1;
    printf("ok 2 variants\n");
    return 0;
}
