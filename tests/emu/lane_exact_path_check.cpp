// tests/emu/lane_exact_path_check.cpp — TEST ONLY: the path class of the lane extender's exact exit (metagraph_amd/csrc/
// lane_read.hpp: lane_exact_class(), lane_all_nodes(), the LANE_EMIT_EXACT branch of lane_emit()) under the host wave model, on
// hand-made seed headers and node arrays.  Per read length L (L = k, the 16-byte groups of the scan, packed-word and output-word
// boundaries), strand and alignment of the read's node array (it begins 0 .. 3 words behind a 16-byte boundary, so the scan's
// single-word head, its four-node loads and its tail all occur at both ends): a header whose first seed starts at the query's
// first character and ends short of it; every node set -> the path class at level 2, nothing at level 1; a zero at the first
// index only, at the last only, at every index in turn -> refused; the stream exactly large enough (every word checked, the
// guard words untouched) and one word too small (capacity status, no word written).  tests/test_lane_exact_path.py builds this
// program with -fsanitize=address,undefined; every buffer is sized exactly, so a word read or written past its array — or a
// 16-byte load that is not aligned — stops the run.
#include "wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "graph_build.hpp"
#include "lane_read.hpp"

using namespace mgx;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

struct World {
    int32_t k, L, nk;
    int strand, shift, front;
    std::vector<uint64_t> offsets, node_begin, pk[2];
    std::vector<uint32_t> nodes[2], iv[2], stream, work_key;
    std::vector<SeedHdr> hdr;
    std::vector<DevSeed> seeds;
    std::vector<ReadResult> results;
    std::string codes[2];
    unsigned long long cursor = 0;
    LaneParams LP;
};

// read 1 of two (read 0 is a 7-character dummy that owns the first words of the node arrays: the read's nodes begin behind them,
// `shift` words past a 16-byte boundary, and end with the array)
static void make(World &w, int32_t k, int32_t L, int strand, int shift, std::mt19937 &rng) {
    w.k = k; w.L = L; w.strand = strand; w.shift = shift;
    const uint64_t off0 = 7;
    w.offsets = { 0, off0, off0 + (uint64_t)L };
    const int32_t nk = L - k + 1;
    w.nk = nk;
    // the words in front of the read's nodes: as many as put the first node `shift` words behind a 16-byte boundary, wherever
    // the allocator put the array of the strand under test
    int front = shift;
    for (; front < shift + 4; ++front) {
        w.nodes[strand].assign(front + nk, 0);
        if ((((uintptr_t)w.nodes[strand].data() >> 2) + (uintptr_t)front) % 4 == (uintptr_t)shift) break;
    }
    if (front == shift + 4) { printf("FAILED: no placement of the node array at shift %d\n", shift); ++g_fail; front = shift; }
    w.front = front;
    w.node_begin = { 0, (uint64_t)front, (uint64_t)(front + nk) };
    const uint64_t wb = packed_word_begin(off0, 1), nw = ((uint64_t)L + 31) >> 5;
    for (int s = 0; s < 2; ++s) {
        w.codes[s].resize(L);
        w.pk[s].assign(wb + nw, 0);
        w.iv[s].assign(wb + nw, 0);
        for (int32_t i = 0; i < L; ++i) {
            const uint32_t c = rng() & 3u;
            w.codes[s][i] = "ACGT"[c];
            w.pk[s][wb + (i >> 5)] |= (uint64_t)c << (2 * (i & 31));
        }
        // the other strand's array is all zeros: a scan of the wrong strand refuses every read
        w.nodes[s].assign(front + nk, 0);
        if (s == strand)
            for (int32_t i = 0; i < nk; ++i) w.nodes[s][front + i] = 1000u * (s + 1) + (uint32_t)i;
    }
    // the first seed: from the query's first character, short of its end; a second one behind it, as behind a fork
    const int32_t len0 = (L - 5 >= k) ? L - 5 : L - 1;
    w.hdr.assign(2, SeedHdr{});
    SeedHdr &h = w.hdr[1];
    h.off = 3;
    w.seeds.assign(3, DevSeed{ 9, 9, 9, 9, 9 });
    const DevSeed head = { 0, (uint16_t)len0, 0, (uint16_t)(len0 >= k ? len0 - k + 1 : 0), 0 };
    const DevSeed later = { 2, (uint16_t)(L - 2), 0, 1, 0 };
    if (strand == 0) { w.seeds.push_back(head); w.seeds.push_back(later); h.n_seeds[0] = 2; h.n_seeds[1] = 0; h.num_matching[0] = (uint32_t)L; h.num_matching[1] = 0; }
    else { w.seeds.push_back(DevSeed{ 3, 2, 9, 1, 77 }); w.seeds.push_back(head); w.seeds.push_back(later); h.n_seeds[0] = 1; h.n_seeds[1] = 2; h.num_matching[0] = 2; h.num_matching[1] = (uint32_t)L; }
    h.status = ST_OK;
    w.results.assign(2, ReadResult{});
    w.work_key.assign(2, 0);
    memset(&w.LP, 0, sizeof(w.LP));
    AlignParams &P = w.LP.P;
    P.g.k = (uint32_t)k;
    P.cfg.fwd_and_rc = 1; P.cfg.rel_score_cutoff = 0.95; P.cfg.left_end_bonus = 5; P.cfg.right_end_bonus = 4;
    P.cfg.min_path_score = 0; P.cfg.min_cell_score = NINF;
    P.lim.Lmax = 256; P.lim.max_seeds = 4;
    P.offsets = w.offsets.data(); P.node_begin = w.node_begin.data();
    P.nodes_fwd = w.nodes[0].data(); P.nodes_rc = w.nodes[1].data();
    P.n_reads = 2;
    P.seed_hdr = w.hdr.data(); P.seed_stream = w.seeds.data();
    P.results = w.results.data();
    P.out_cursor = &w.cursor;
    P.work_key = w.work_key.data();
    w.LP.pk[0] = w.pk[0].data(); w.LP.pk[1] = w.pk[1].data(); w.LP.iv[0] = w.iv[0].data(); w.LP.iv[1] = w.iv[1].data();
    w.LP.self_score = 2;
    w.LP.exact = 2;
}

static const uint32_t GUARD = 0xDEADBEEFu;

// capacity `cap` words, the read's words handed out at `so`
static void emit(World &w, LaneResult &R, uint64_t so, uint64_t cap) {
    w.stream.assign(cap, GUARD);
    w.LP.P.out_stream = w.stream.data();
    w.LP.P.out_capacity = cap;
    LaneChip chip = { 0, nullptr, 0, nullptr, 0 };
    lane_emit(w.LP, 1, nullptr, chip, R, so);
}

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    std::mt19937 rng(20240733);
    long n_cases = 0, n_refused = 0;
    const int32_t k = 11;
    for (int32_t L : { 11, 12, 13, 14, 15, 18, 19, 31, 32, 33, 64, 150, 256 })
        for (int strand = 0; strand < 2; ++strand)
            for (int shift = 0; shift < 4; ++shift) {
                World w;
                make(w, k, L, strand, shift, rng);
                CHECK((((uintptr_t)(w.nodes[strand].data() + w.front) >> 2) & 3u) == (uintptr_t)shift);
                LaneResult R;
                memset(&R, 0, sizeof(R));
                CHECK(lane_exact(w.LP, 1, R) == LANE_EXACT_PATH);
                if (g_fail) return 1;
                const uint32_t nk = (uint32_t)w.nk, want_words = nk + 1 + ((uint32_t)L + 3) / 4;
                CHECK(R.words == want_words && R.mode == LANE_EMIT_EXACT && R.have_aln == 1 && R.strand == strand);
                CHECK(R.rr.n_extensions == 0 && R.rr.n_columns == 0 && R.score == 2 * L + 9);
                // the stream: exactly enough room, behind 5 words of another read
                const uint64_t so = 5;
                LaneResult R1 = R;
                emit(w, R1, so, so + want_words);
                const ReadResult &rr = w.results[1];
                CHECK(rr.status == ST_OK && rr.n_alignments == 1 && rr.score == 2 * L + 9 && rr.offset == 0);
                CHECK(rr.n_nodes == nk && rr.n_cigar == 1 && rr.seq_len == (uint32_t)L && rr.orientation == (uint32_t)strand && rr.stream_off == so);
                CHECK(rr.n_seeds_fwd == (strand ? 1u : 2u) && rr.n_seeds_rc == (strand ? 2u : 0u) && rr.n_extensions == 0 && rr.n_columns == 0);
                for (uint64_t x = 0; x < so; ++x) CHECK(w.stream[x] == GUARD);
                for (uint32_t x = 0; x < nk; ++x) CHECK(w.stream[so + x] == w.nodes[strand][w.front + x]);
                CHECK(w.stream[so + nk] == (((uint32_t)L << 3) | OP_MATCH));
                std::vector<uint8_t> want_seq(((size_t)L + 3) / 4 * 4, 0);
                memcpy(want_seq.data(), w.codes[strand].data(), (size_t)L);
                CHECK(!memcmp(&w.stream[so + nk + 1], want_seq.data(), want_seq.size()));
                // one word too small: the capacity status, nothing written
                LaneResult R2 = R;
                emit(w, R2, so, so + want_words - 1);
                CHECK(w.results[1].status == ST_CAPACITY && w.results[1].n_alignments == 0);
                for (uint64_t x = 0; x < w.stream.size(); ++x) CHECK(w.stream[x] == GUARD);
                // through lane_read(), the wrapper the host model calls
                {
                    LaneCounters ctr = { 0 };
                    LaneChip chip = { 0, nullptr, 0, nullptr, 0 };
                    LaneResult R3;
                    memset(&R3, 0, sizeof(R3));
                    CHECK(lane_read(w.LP, 1, 0, 0, nullptr, chip, ctr, R3) == LR_DONE && R3.words == want_words && R3.mode == LANE_EMIT_EXACT);
                }
                ++n_cases;
                auto refused = [&](const char *what, int at) {
                    LaneResult Rx;
                    memset(&Rx, 0, sizeof(Rx));
                    if (lane_exact(w.LP, 1, Rx) != LANE_EXACT_NONE) {
                        printf("FAILED: %s (%d) left through the exact exit (L %d, strand %d, shift %d)\n", what, at, L, strand, shift);
                        ++g_fail;
                    }
                    ++n_refused;
                };
                // level 1 leaves the read to the DP
                w.LP.exact = 1; refused("level 1", 0); w.LP.exact = 2;
                // one zero in the node array: at the first index, at the last, at every index in turn
                uint32_t *nd = w.nodes[strand].data() + w.front;
                { const uint32_t keep = nd[0]; nd[0] = 0; refused("a zero at the first index", 0); nd[0] = keep; }
                { const uint32_t keep = nd[nk - 1]; nd[nk - 1] = 0; refused("a zero at the last index", (int)nk - 1); nd[nk - 1] = keep; }
                for (uint32_t x = 0; x < nk; ++x) { const uint32_t keep = nd[x]; nd[x] = 0; refused("a zero", (int)x); nd[x] = keep; }
                // the words in front of the read's nodes are another read's: zeros there do not matter
                for (int x = 0; x < w.front; ++x) w.nodes[strand][x] = 0;
                { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx) == LANE_EXACT_PATH); }
                // the first seed must start at the query's first character
                DevSeed &sd = w.seeds[3 + strand];
                const DevSeed keep = sd;
                sd.clipping = 1; refused("a clipped first seed", 0); sd = keep;
                sd.offset = 1; refused("a first seed with an offset", 0); sd = keep;
                w.hdr[1].status = ST_CAPACITY; refused("a header with a capacity status", 0); w.hdr[1].status = ST_OK;
                w.LP.P.cfg.min_path_score = 2 * L + 10; refused("min_path_score above the full score", 0); w.LP.P.cfg.min_path_score = 0;
                w.LP.P.labeled = 1; refused("a label-aware batch", 0); w.LP.P.labeled = 0;
                // a first seed that spans the query is the first class, at either level
                sd.length = (uint16_t)L;
                { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx) == LANE_EXACT_SPAN); }
                sd = keep;
                { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx) == LANE_EXACT_PATH); }       // (everything restored)
            }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok %ld cases, %ld refusals\n", n_cases, n_refused);
    return 0;
}
