// tests/emu/lane_exact_label_check.cpp — TEST ONLY: the lane extender's exact exit on a label-aware batch (metagraph_amd/csrc/
// lane_read.hpp: lane_exact_class(), lane_exact_label_filter(), lane_all_rows(), the LANE_EMIT_EXACT branch of lane_emit() with
// the two label words) under the host wave model, on hand-made seed headers, node arrays and annotation rows.  Per read length L
// (L = k: the span class; the 16-byte groups of the scan, packed-word and output-word boundaries), strand and alignment of the
// read's node array: k-mer seeds — as the label-aware seeder makes them — every fourth node and at the last, so that most nodes
// are seen by the row scan alone; every row { 7 } -> the class; a wrong row (another label, two labels with 7 among them, none)
// at the first node, the last, every node in turn -> refused; a node above g.n or behind the annotation's rows -> refused; a
// strand below min_exact_match -> refused; seeds of two labels -> refused; AlignParams::labeled == 1 -> refused with no
// annotation behind it; the stream exactly large enough (every word checked, guard words untouched) and one word too small
// (capacity status, nothing written).  tests/test_lane_exact_labels.py builds this program with -fsanitize=address,undefined;
// every buffer is sized exactly — the annotation's head words too — so a word read or written past its array stops the run.
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

static const uint32_t LABEL = 7, OTHER = 9;
static uint64_t head_one(uint32_t label) { return ((uint64_t)label << 16) | 1u; }
static const uint64_t HEAD_TWO = ((uint64_t)12 << 16) | 2u;       // two labels (an offset into the label lists behind it)
static const uint64_t HEAD_NONE = 0;

struct World {
    int32_t k, L, nk;
    int strand, shift, front, n_mine;
    std::vector<uint64_t> offsets, node_begin, pk[2], head;
    std::vector<uint32_t> nodes[2], iv[2], stream, work_key;
    std::vector<SeedHdr> hdr;
    std::vector<DevSeed> seeds;
    std::vector<ReadResult> results;
    std::string codes[2];
    unsigned long long cursor = 0;
    LaneParams LP;
};

// read 1 of two (read 0 owns the first words of the node arrays: the read's nodes begin `shift` words past a 16-byte boundary and
// end with the array).  Node x of the strand is node 1 + x of the graph, row x of the annotation; strand 1's world has one sub-k
// seed on strand 0 whose node is the graph's last (row nk), which the filter drops with its strand.
static void make(World &w, int32_t k, int32_t L, int strand, int shift, std::mt19937 &rng) {
    w.k = k; w.L = L; w.strand = strand; w.shift = shift;
    const uint64_t off0 = 7;
    w.offsets = { 0, off0, off0 + (uint64_t)L };
    const int32_t nk = L - k + 1;
    w.nk = nk;
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
        w.nodes[s].assign(front + nk, 0);
        if (s == strand)
            for (int32_t i = 0; i < nk; ++i) w.nodes[s][front + i] = 1u + (uint32_t)i;
    }
    const uint32_t n_rows = (uint32_t)nk + (strand ? 1u : 0u);
    w.head.assign(n_rows, head_one(LABEL));
    // the strand's seeds: one k-mer each, at every fourth node and at the last
    std::vector<DevSeed> mine;
    for (int32_t i = 0; i < nk; i += 4) mine.push_back(DevSeed{ (uint16_t)i, (uint16_t)k, 0, 1, 0 });
    if ((nk - 1) % 4) mine.push_back(DevSeed{ (uint16_t)(nk - 1), (uint16_t)k, 0, 1, 0 });
    w.n_mine = (int)mine.size();
    w.hdr.assign(2, SeedHdr{});
    SeedHdr &h = w.hdr[1];
    h.off = 3;
    w.seeds.assign(3, DevSeed{ 9, 9, 9, 9, 9 });
    if (strand) { w.seeds.push_back(DevSeed{ 3, 2, 9, 1, (uint32_t)nk + 1u }); h.n_seeds[0] = 1; h.num_matching[0] = 2; }
    w.seeds.insert(w.seeds.end(), mine.begin(), mine.end());
    h.n_seeds[strand] = (uint16_t)mine.size();
    h.num_matching[strand] = (uint32_t)L;
    h.status = ST_OK;
    w.results.assign(2, ReadResult{});
    w.work_key.assign(2, 0);
    memset(&w.LP, 0, sizeof(w.LP));
    AlignParams &P = w.LP.P;
    P.g.k = (uint32_t)k; P.g.n = n_rows;
    P.cfg.fwd_and_rc = 1; P.cfg.rel_score_cutoff = 0.95; P.cfg.left_end_bonus = 5; P.cfg.right_end_bonus = 4;
    P.cfg.min_path_score = 0; P.cfg.min_cell_score = NINF; P.cfg.min_exact_match = 0.7;
    P.lim.Lmax = 256; P.lim.max_seeds = (uint32_t)mine.size() + 1;
    P.offsets = w.offsets.data(); P.node_begin = w.node_begin.data();
    P.nodes_fwd = w.nodes[0].data(); P.nodes_rc = w.nodes[1].data();
    P.n_reads = 2;
    P.seed_hdr = w.hdr.data(); P.seed_stream = w.seeds.data();
    P.results = w.results.data();
    P.out_cursor = &w.cursor;
    P.work_key = w.work_key.data();
    P.labeled = 3; P.anno_rows = n_rows; P.anno_head = w.head.data();
    w.LP.pk[0] = w.pk[0].data(); w.LP.pk[1] = w.pk[1].data(); w.LP.iv[0] = w.iv[0].data(); w.LP.iv[1] = w.iv[1].data();
    w.LP.self_score = 2;
    w.LP.exact = 2;
}

static const uint32_t GUARD = 0xDEADBEEFu;

static void emit(World &w, LaneResult &R, uint64_t so, uint64_t cap) {
    w.stream.assign(cap, GUARD);
    w.LP.P.out_stream = w.stream.data();
    w.LP.P.out_capacity = cap;
    LaneChip chip = { 0, nullptr, 0, nullptr, 0 };
    lane_emit(w.LP, 1, nullptr, chip, R, so);
}

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    std::mt19937 rng(20240934);
    long n_cases = 0, n_refused = 0;
    const int32_t k = 11;
    for (int32_t L : { 11, 12, 13, 14, 15, 18, 19, 31, 32, 33, 64, 150, 256 })
        for (int strand = 0; strand < 2; ++strand)
            for (int shift = 0; shift < 4; ++shift) {
                World w;
                make(w, k, L, strand, shift, rng);
                const int want_cls = L == k ? LANE_EXACT_SPAN : LANE_EXACT_PATH;
                LaneResult R;
                memset(&R, 0, sizeof(R));
                CHECK(lane_exact(w.LP, 1, R) == want_cls);
                if (g_fail) return 1;
                const uint32_t nk = (uint32_t)w.nk, seq_words = ((uint32_t)L + 3) / 4, want_words = nk + 1 + seq_words + 2;
                CHECK(R.words == want_words && R.mode == LANE_EMIT_EXACT && R.have_aln == 1 && R.strand == strand && R.label == LABEL);
                CHECK(R.rr.n_extensions == 0 && R.rr.n_columns == 0 && R.score == 2 * L + 9);
                // the record: what the filter left — the other strand's sub-k seed is gone, num_matching recounted
                CHECK(R.rr.n_seeds_fwd == (strand ? 0u : (uint32_t)w.n_mine) && R.rr.n_seeds_rc == (strand ? (uint32_t)w.n_mine : 0u));
                CHECK(R.rr.num_matches_fwd == (strand ? 0u : (uint32_t)L) && R.rr.num_matches_rc == (strand ? (uint32_t)L : 0u));
                const uint64_t so = 5;
                LaneResult R1 = R;
                emit(w, R1, so, so + want_words);
                const ReadResult &rr = w.results[1];
                CHECK(rr.status == ST_OK && rr.n_alignments == 1 && rr.score == 2 * L + 9 && rr.offset == 0);
                CHECK(rr.n_nodes == nk && rr.n_cigar == 1 && rr.seq_len == (uint32_t)L && rr.orientation == (uint32_t)strand && rr.stream_off == so);
                for (uint64_t x = 0; x < so; ++x) CHECK(w.stream[x] == GUARD);
                for (uint32_t x = 0; x < nk; ++x) CHECK(w.stream[so + x] == 1u + x);
                CHECK(w.stream[so + nk] == (((uint32_t)L << 3) | OP_MATCH));
                std::vector<uint8_t> want_seq((size_t)seq_words * 4, 0);
                memcpy(want_seq.data(), w.codes[strand].data(), (size_t)L);
                CHECK(!memcmp(&w.stream[so + nk + 1], want_seq.data(), want_seq.size()));
                CHECK(w.stream[so + nk + 1 + seq_words] == 1u && w.stream[so + nk + 2 + seq_words] == LABEL);
                // one word too small: the capacity status, nothing written
                LaneResult R2 = R;
                emit(w, R2, so, so + want_words - 1);
                CHECK(w.results[1].status == ST_CAPACITY && w.results[1].n_alignments == 0);
                for (uint64_t x = 0; x < w.stream.size(); ++x) CHECK(w.stream[x] == GUARD);
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
                auto accepted = [&]() { LaneResult Rx; memset(&Rx, 0, sizeof(Rx)); CHECK(lane_exact(w.LP, 1, Rx) == want_cls); };
                if (L != k) { w.LP.exact = 1; refused("level 1", 0); w.LP.exact = 2; }
                // a wrong row: at the first node, the last, every node in turn
                for (const uint64_t wrong : { head_one(OTHER), HEAD_TWO, HEAD_NONE }) {
                    if (nk == 1 && wrong == head_one(OTHER)) {
                        // (the read's one node with another label: that is the read's label then — unless the other strand's seed,
                        // dropped or not, carries LABEL: seeds of two labels)
                        w.head[0] = wrong;
                        LaneResult Rx; memset(&Rx, 0, sizeof(Rx));
                        if (strand) refused("seeds of two labels, one on either strand", 0);
                        else CHECK(lane_exact(w.LP, 1, Rx) == want_cls && Rx.label == OTHER);
                        w.head[0] = head_one(LABEL);
                        continue;
                    }
                    { w.head[0] = wrong; refused("a wrong row at the first node", 0); w.head[0] = head_one(LABEL); }
                    { w.head[nk - 1] = wrong; refused("a wrong row at the last node", (int)nk - 1); w.head[nk - 1] = head_one(LABEL); }
                    for (uint32_t x = 0; x < nk; ++x) { w.head[x] = wrong; refused("a wrong row", (int)x); w.head[x] = head_one(LABEL); }
                }
                accepted();
                // seeds of two labels: the first node of the second seed (where there is one)
                if (w.n_mine > 1) { w.head[4 < nk ? 4 : nk - 1] = head_one(OTHER); refused("seeds of two labels", 4); w.head[4 < nk ? 4 : nk - 1] = head_one(LABEL); }
                // a node that is no k-mer of the graph, a node above g.n, a node behind the annotation's rows (the head words end there)
                uint32_t *nd = w.nodes[strand].data() + w.front;
                for (uint32_t x = 0; x < nk; ++x) { const uint32_t keep = nd[x]; nd[x] = 0; refused("a zero", (int)x); nd[x] = keep; }
                for (uint32_t x = 0; x < nk; ++x) { const uint32_t keep = nd[x]; nd[x] = (uint32_t)w.LP.P.g.n + 1u; refused("a node above g.n", (int)x); nd[x] = keep; }
                { const uint64_t keep = w.LP.P.g.n; w.LP.P.g.n = nk - 1; refused("the last node above g.n", (int)nk - 1); w.LP.P.g.n = keep; }
                {
                    // (the rows end one short of the last node's: a copy of exactly that size)
                    std::vector<uint64_t> fewer(w.head.begin(), w.head.begin() + (nk - 1));
                    w.LP.P.anno_head = fewer.data(); w.LP.P.anno_rows = nk - 1;
                    refused("a node behind the annotation's rows", (int)nk - 1);
                    w.LP.P.anno_head = w.head.data(); w.LP.P.anno_rows = w.head.size();
                }
                accepted();
                // the strand's label below min_exact_match: its seeds are dropped
                w.LP.P.cfg.min_exact_match = 1.5; refused("min_exact_match above 1", 0); w.LP.P.cfg.min_exact_match = 0.7;
                if ((double)(k + 4) < 0.7 * (double)L) {
                    const uint16_t keep = w.hdr[1].n_seeds[strand];
                    w.hdr[1].n_seeds[strand] = 2; refused("two seeds that cover too little", 0); w.hdr[1].n_seeds[strand] = keep;
                }
                // AlignParams::labeled without bit 1: no annotation pointer is touched
                w.LP.P.labeled = 1; w.LP.P.anno_head = nullptr; refused("rows of dummy nodes may hold labels", 0);
                w.LP.P.labeled = 3; w.LP.P.anno_head = w.head.data();
                // the tests of the unlabeled exit
                DevSeed &sd = w.seeds[3 + strand];
                const DevSeed keep = sd;
                sd.offset = 1; sd.node = 1; refused("a first seed with an offset", 0); sd = keep;
                w.hdr[1].status = ST_CAPACITY; refused("a header with a capacity status", 0); w.hdr[1].status = ST_OK;
                w.LP.P.cfg.min_path_score = 2 * L + 10; refused("min_path_score above the full score", 0); w.LP.P.cfg.min_path_score = 0;
                accepted();
                // through lane_read(), the wrapper the host model calls
                {
                    LaneCounters ctr = { 0 };
                    LaneChip chip = { 0, nullptr, 0, nullptr, 0 };
                    LaneResult R3;
                    memset(&R3, 0, sizeof(R3));
                    CHECK(lane_read(w.LP, 1, 0, 0, nullptr, chip, ctr, R3) == LR_DONE && R3.words == want_words && R3.mode == LANE_EMIT_EXACT);
                }
            }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok %ld cases, %ld refusals\n", n_cases, n_refused);
    return 0;
}
