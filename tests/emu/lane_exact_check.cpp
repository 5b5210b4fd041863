// tests/emu/lane_exact_check.cpp — TEST ONLY: the exact exit of the lane-per-read extender (metagraph_amd/csrc/lane_read.hpp:
// lane_exact(), the LANE_EMIT_EXACT branch of lane_emit()) under the host wave model, on hand-made seed headers — what the host
// model's driver cannot vary: the capacity of the output stream.  Per read length L (packed-word and output-word boundaries) and
// strand: a header whose first seed spans the query; the stream exactly large enough (every word checked, the guard words behind
// it untouched), one word too small (capacity status, no word written), and the headers that must NOT leave through the exit
// (clipping, offset, a shorter seed, a header status, a second strand to align, min_path_score above the full score, a
// label-aware batch).  tests/test_lane_exact.py builds this program with -fsanitize=address,undefined; every buffer is sized
// exactly, so a word read or written past its array stops the run.
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
    int32_t k, L;
    int strand;
    std::vector<uint64_t> offsets, node_begin, pk[2];
    std::vector<uint32_t> nodes[2], iv[2], stream, work_key;
    std::vector<SeedHdr> hdr;
    std::vector<DevSeed> seeds;
    std::vector<ReadResult> results;
    std::string codes[2];
    unsigned long long cursor = 0;
    LaneParams LP;
};

// read 1 of two (read 0 is a 7-character dummy, so that offsets and packed words do not start at 0)
static void make(World &w, int32_t k, int32_t L, int strand, std::mt19937 &rng) {
    w.k = k; w.L = L; w.strand = strand;
    const uint64_t off0 = 7;
    w.offsets = { 0, off0, off0 + (uint64_t)L };
    const int32_t nk = L >= k ? L - k + 1 : 0;
    w.node_begin = { 0, 0, (uint64_t)nk };
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
        w.nodes[s].resize(nk);
        for (int32_t i = 0; i < nk; ++i) w.nodes[s][i] = 1000u * (s + 1) + (uint32_t)i;
    }
    // strand 0's seeds first: one sub-k tail seed on the other strand's side keeps the stream offsets honest
    w.seeds.clear();
    w.hdr.assign(2, SeedHdr{});
    SeedHdr &h = w.hdr[1];
    h.off = 3;
    w.seeds.assign(3, DevSeed{ 9, 9, 9, 9, 9 });
    const DevSeed full = { 0, (uint16_t)L, 0, (uint16_t)nk, 0 };
    if (strand == 0) { w.seeds.push_back(full); h.n_seeds[0] = 1; h.n_seeds[1] = 0; h.num_matching[0] = (uint32_t)L; h.num_matching[1] = 0; }
    else { w.seeds.push_back(DevSeed{ 3, 2, 9, 1, 77 }); w.seeds.push_back(full); h.n_seeds[0] = 1; h.n_seeds[1] = 1; h.num_matching[0] = 2; h.num_matching[1] = (uint32_t)L; }
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
    w.LP.exact = 1;
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
    std::mt19937 rng(20240611);
    long n_cases = 0, n_refused = 0;
    const int32_t k = 11;
    for (int32_t L : { 11, 12, 13, 14, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 255, 256 })
        for (int strand = 0; strand < 2; ++strand) {
            World w;
            make(w, k, L, strand, rng);
            LaneResult R;
            memset(&R, 0, sizeof(R));
            CHECK(lane_exact(w.LP, 1, R));
            if (g_fail) return 1;
            const uint32_t nk = (uint32_t)(L - k + 1), want_words = nk + 1 + ((uint32_t)L + 3) / 4;
            CHECK(R.words == want_words && R.mode == LANE_EMIT_EXACT && R.have_aln == 1 && R.strand == strand);
            CHECK(R.rr.n_extensions == 0 && R.rr.n_columns == 0);
            // exactly enough room, behind 5 words of another read
            const uint64_t so = 5;
            LaneResult R1 = R;
            emit(w, R1, so, so + want_words);
            const ReadResult &rr = w.results[1];
            CHECK(rr.status == ST_OK && rr.n_alignments == 1 && rr.score == 2 * L + 9 && rr.offset == 0);
            CHECK(rr.n_nodes == nk && rr.n_cigar == 1 && rr.seq_len == (uint32_t)L && rr.orientation == (uint32_t)strand && rr.stream_off == so);
            CHECK(rr.n_seeds_fwd == 1 && rr.n_seeds_rc == (uint32_t)strand && rr.n_extensions == 0 && rr.n_columns == 0);
            for (uint64_t x = 0; x < so; ++x) CHECK(w.stream[x] == GUARD);
            for (uint32_t x = 0; x < nk; ++x) CHECK(w.stream[so + x] == w.nodes[strand][x]);
            CHECK(w.stream[so + nk] == (((uint32_t)L << 3) | OP_MATCH));
            std::vector<uint8_t> want_seq(((size_t)L + 3) / 4 * 4, 0);
            memcpy(want_seq.data(), w.codes[strand].data(), (size_t)L);
            CHECK(!memcmp(&w.stream[so + nk + 1], want_seq.data(), want_seq.size()));
            // one word too small: the capacity status, nothing written
            LaneResult R2 = R;
            emit(w, R2, so, so + want_words - 1);
            CHECK(w.results[1].status == ST_CAPACITY && w.results[1].n_alignments == 0);
            for (uint64_t x = 0; x < w.stream.size(); ++x) CHECK(w.stream[x] == GUARD);
            // ... and the same through lane_read(), the wrapper the host model calls
            {
                LaneCounters ctr = { 0 };
                LaneChip chip = { 0, nullptr, 0, nullptr, 0 };
                LaneResult R3;
                memset(&R3, 0, sizeof(R3));
                CHECK(lane_read(w.LP, 1, 0, 0, nullptr, chip, ctr, R3) == LR_DONE && R3.words == want_words && R3.mode == LANE_EMIT_EXACT);
            }
            ++n_cases;
            // headers that stay with the DP
            auto refused = [&](const char *what) {
                LaneResult Rx;
                memset(&Rx, 0, sizeof(Rx));
                const bool r = lane_exact(w.LP, 1, Rx);
                if (r) { printf("FAILED: %s left through the exact exit (L %d, strand %d)\n", what, L, strand); ++g_fail; }
                ++n_refused;
            };
            DevSeed &sd = w.seeds[3 + strand];
            const DevSeed keep = sd;
            sd.clipping = 1; sd.length = (uint16_t)(L - 1); refused("a clipped seed"); sd = keep;
            sd.offset = 1; refused("a seed with an offset"); sd = keep;
            sd.length = (uint16_t)(L - 1); refused("a seed short of the query's end"); sd = keep;
            w.hdr[1].status = ST_CAPACITY; refused("a header with a capacity status"); w.hdr[1].status = ST_OK;
            { SeedHdr &h = w.hdr[1]; const SeedHdr hk = h; const int o = 1 - strand;
              if (h.n_seeds[o] == 0) h.n_seeds[o] = 1;       // (strand 0's run then takes the full seed's place: the other strand's header only)
              h.num_matching[o] = (uint32_t)((L * 96 + 99) / 100);
              if (strand == 1) refused("a second strand within rel_score_cutoff");
              h = hk; }
            w.LP.P.cfg.min_path_score = 2 * L + 10; refused("min_path_score above the full score");
            w.LP.P.cfg.min_path_score = 2 * L + 9; { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx)); }
            w.LP.P.cfg.min_path_score = 0;
            w.LP.P.cfg.min_cell_score = 2 * L + 10; refused("min_cell_score above the full score"); w.LP.P.cfg.min_cell_score = NINF;
            w.LP.P.labeled = 1; refused("a label-aware batch"); w.LP.P.labeled = 0;
            w.LP.P.lim.Lmax = (uint32_t)L - 1; refused("a read longer than the batch's limit"); w.LP.P.lim.Lmax = 256;
            { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx)); }       // (everything restored)
        }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok %ld cases, %ld refusals\n", n_cases, n_refused);
    return 0;
}
