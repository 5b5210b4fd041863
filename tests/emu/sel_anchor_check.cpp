// tests/emu/sel_anchor_check.cpp — TEST ONLY: the select anchors of the device index (graph_build.hpp: sel_anchor_shift,
// build_sel_anchor; dev_graph.hpp: sel_predict, select_last_scan) and the per-index primitives next to them (select_last_blk,
// select_W, rank_W, rank_last, pred_last, succ_last, succ_W_code) under the host wave model, against plain loops over the same W / last
// arrays.  The tables are random and need not be graphs: only `last`, the blocks and the hints are read.  Every 16-byte load
// of a block goes through the gld overload below, which counts it and refuses an index outside [0, n_blocks); the vectors are
// sized exactly as mgx_graph_create sizes the device buffers, and tests/test_sel_anchor_check.py builds this program with
// -fsanitize=address,undefined, so that a hint or anchor read past its table stops the run as well.
#include "wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace mgx {
static const uint4 *g_blocks_begin = nullptr, *g_blocks_end = nullptr;
static uint64_t g_block_loads = 0, g_block_loads_outside = 0;
// (a non-template overload: load_block's four gld calls resolve to it)
inline uint4 gld(const uint4 *p) {
    ++g_block_loads;
    if (p < g_blocks_begin || p >= g_blocks_end) { ++g_block_loads_outside; return uint4{ 0, 0, 0, 0 }; }
    return *p;
}
}
#include "../../metagraph_amd/csrc/graph_build.hpp"

using namespace mgx;

struct Table {
    uint64_t n = 0;
    std::vector<uint8_t> W, last;
    std::vector<Block> blocks;
    std::vector<uint32_t> last_hint, w_hint[4], sel_anchor;
    uint64_t tot[6] = { 0, 0, 0, 0, 0, 0 };
    DevGraph g;
};

// as mgx_graph_create: pass 1, the exclusive prefix sums on the host, pass 2, the anchors
static void build(Table &t, uint32_t max_entries) {
    const uint64_t n = t.n;
    const uint32_t n_blocks = (uint32_t)((n + 1 + 63) / 64);
    t.blocks.assign(n_blocks, Block());
    std::vector<uint32_t> counts((size_t)n_blocks * 6);
    for (uint32_t b = 0; b < n_blocks; ++b) build_block_pass1(b, t.W.data(), t.last.data(), n, t.blocks.data(), counts.data());
    for (int c = 0; c < 6; ++c) t.tot[c] = 0;
    for (uint32_t b = 0; b < n_blocks; ++b)
        for (int c = 0; c < 6; ++c) { const uint32_t v = counts[(size_t)b * 6 + c]; counts[(size_t)b * 6 + c] = (uint32_t)t.tot[c]; t.tot[c] += v; }
    t.last_hint.assign(t.tot[5] / 64 + 2, 0);
    uint32_t *wh[4];
    for (int c = 0; c < 4; ++c) { t.w_hint[c].assign(t.tot[c + 1] / 64 + 2, 0); wh[c] = t.w_hint[c].data(); }
    for (uint32_t b = 0; b < n_blocks; ++b) build_block_pass2(b, t.blocks.data(), counts.data(), t.last_hint.data(), wh);
    DevGraph &g = t.g;
    memset(&g, 0, sizeof(g));
    g.blocks = t.blocks.data();
    g.last_hint = t.last_hint.data();
    for (int c = 0; c < 4; ++c) g.w_hint[c] = t.w_hint[c].data();
    g.n = n; g.n_blocks = n_blocks; g.k = 31;
    g_blocks_begin = reinterpret_cast<const uint4 *>(t.blocks.data());
    g_blocks_end = reinterpret_cast<const uint4 *>(t.blocks.data() + n_blocks);
    g.sel_shift = sel_anchor_shift(t.tot[5], max_entries);
    g.sel_n = (uint32_t)(t.tot[5] >> g.sel_shift) + 2;
    t.sel_anchor.assign(g.sel_n, 0);
    for (uint32_t j = 0; j < g.sel_n; ++j) build_sel_anchor(g, j, g.sel_shift, g.sel_n, (uint32_t)t.tot[5], t.sel_anchor.data());
    g.sel_anchor = t.sel_anchor.data();
}

static uint64_t n_pairs = 0, n_scan_steps = 0, max_scan_steps = 0, n_hint_steps = 0, n_index_checks = 0, n_tables = 0, n_span0 = 0;
static uint64_t pairs_of_shift[32];

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return false; } } while (0)

// every rank r = 1 .. total_last: the prediction is a block of the table, the scan from it and the hinted select both give
// the plain answer (and its block)
static bool check_select(const Table &t) {
    const DevGraph &g = t.g;
    std::vector<uint64_t> pos(1, 0);
    for (uint64_t i = 1; i <= t.n; ++i) if (t.last[i]) pos.push_back(i);
    const uint64_t total = pos.size() - 1;
    CHECK(total == t.tot[5], "total_last %llu, the build counted %llu", (unsigned long long)total, (unsigned long long)t.tot[5]);
    CHECK(t.sel_anchor[0] == 0, "anchor 0");
    for (uint32_t j = 1; j < g.sel_n; ++j) {
        CHECK(t.sel_anchor[j] >= t.sel_anchor[j - 1], "anchors not ascending at %u", j);
        if (((uint64_t)j << g.sel_shift) <= total) CHECK(t.sel_anchor[j] == pos[(uint64_t)j << g.sel_shift], "anchor %u", j);
    }
    if ((total & ((1ull << g.sel_shift) - 1)) == 0) ++n_span0;
    for (uint64_t r = 1; r <= total; ++r) {
        const uint32_t p = sel_predict(g.sel_anchor, g.sel_shift, (uint32_t)r);
        CHECK(p < g.n_blocks, "r %llu shift %u: predicted block %u of %u", (unsigned long long)r, g.sel_shift, p, g.n_blocks);
        LineCtr ctr = { 0, 0, 0 };
        Block b;
        const uint64_t got = select_last_scan(g, (uint32_t)r, p, b, ctr);
        CHECK(got == pos[r], "select_last_scan r %llu shift %u from block %u: %llu, plain %llu", (unsigned long long)r, g.sel_shift, p,
              (unsigned long long)got, (unsigned long long)pos[r]);
        CHECK(memcmp(&b, &t.blocks[pos[r] >> 6], sizeof(Block)) == 0, "select_last_scan r %llu: not the block of the answer", (unsigned long long)r);
        n_scan_steps += ctr.select_lines;
        if (ctr.select_lines > max_scan_steps) max_scan_steps = ctr.select_lines;
        LineCtr c2 = { 0, 0, 0 };
        Block b2;
        const uint64_t got2 = select_last_blk(g, (uint32_t)r, b2, c2);
        CHECK(got2 == pos[r], "select_last_blk r %llu: %llu, plain %llu", (unsigned long long)r, (unsigned long long)got2, (unsigned long long)pos[r]);
        CHECK(memcmp(&b2, &t.blocks[pos[r] >> 6], sizeof(Block)) == 0, "select_last_blk r %llu: not the block of the answer", (unsigned long long)r);
        n_hint_steps += c2.select_lines;
        ++n_pairs;
        ++pairs_of_shift[g.sel_shift];
    }
    LineCtr ctr = { 0, 0, 0 };
    CHECK(select_last(g, 0, ctr) == 0, "select_last(0)");
    CHECK(g_block_loads_outside == 0, "%llu block loads outside [0, %u)", (unsigned long long)g_block_loads_outside, g.n_blocks);
    return true;
}

// every index i = 0 .. n: the ranks, pred_last, succ_last; every rank of every label: select_W
static bool check_index(const Table &t) {
    const DevGraph &g = t.g;
    const uint64_t n = t.n;
    uint32_t rw[5] = { 0, 0, 0, 0, 0 }, rl = 0;
    uint64_t pred = 0;
    std::vector<uint64_t> succ(n + 2, n + 1);
    for (uint64_t i = n; i >= 1; --i) succ[i] = t.last[i] ? i : succ[i + 1];
    std::vector<uint64_t> occ[5];
    std::vector<uint64_t> next_code[SIGMA];          // first position >= i whose label code is d, flagged or not; n + 1 if none
    for (uint32_t d = 0; d < SIGMA; ++d) {
        next_code[d].assign(n + 2, n + 1);
        for (uint64_t i = n; i >= 1; --i) next_code[d][i] = t.W[i] % SIGMA == d ? i : next_code[d][i + 1];
    }
    for (uint64_t i = 0; i <= n; ++i) {
        if (i >= 1) {
            if (t.W[i] < SIGMA) { ++rw[t.W[i]]; occ[t.W[i]].push_back(i); }
            if (t.last[i]) { ++rl; pred = i; }
        }
        LineCtr ctr = { 0, 0, 0 };
        for (uint32_t c = 0; c < SIGMA; ++c)
            CHECK(rank_W(g, i, c, ctr) == rw[c], "rank_W(%llu, %u) = %u, plain %u", (unsigned long long)i, c, rank_W(g, i, c, ctr), rw[c]);
        CHECK(rank_last(g, i, ctr) == rl, "rank_last(%llu)", (unsigned long long)i);
        CHECK(pred_last(g, i, ctr) == pred, "pred_last(%llu) = %llu, plain %llu", (unsigned long long)i, (unsigned long long)pred_last(g, i, ctr), (unsigned long long)pred);
        if (i >= 1) {
            CHECK(succ_last(g, i, ctr) == succ[i], "succ_last(%llu) = %llu, plain %llu", (unsigned long long)i, (unsigned long long)succ_last(g, i, ctr), (unsigned long long)succ[i]);
            CHECK(get_W(g, i, ctr) == t.W[i], "get_W(%llu)", (unsigned long long)i);
            for (uint32_t d = 0; d < SIGMA; ++d) {
                bool flagged = true;
                const uint64_t at = succ_W_code(g, i, d, &flagged, ctr), want = next_code[d][i];
                CHECK(at == want && flagged == (want <= n && t.W[want] >= SIGMA), "succ_W_code(%llu, %u) = %llu, plain %llu", (unsigned long long)i, d,
                      (unsigned long long)at, (unsigned long long)want);
            }
        }
        ++n_index_checks;
    }
    for (uint32_t c = 1; c < SIGMA; ++c) {
        CHECK(occ[c].size() == t.tot[c], "label %u: the build counted %llu", c, (unsigned long long)t.tot[c]);
        for (uint64_t r = 1; r <= occ[c].size(); ++r) {
            LineCtr ctr = { 0, 0, 0 };
            CHECK(select_W(g, c, (uint32_t)r, ctr) == occ[c][r - 1], "select_W(%u, %llu)", c, (unsigned long long)r);
        }
    }
    CHECK(g_block_loads_outside == 0, "%llu block loads outside [0, %u)", (unsigned long long)g_block_loads_outside, g.n_blocks);
    return true;
}

// a table of n edges with exactly `total` set last bits (total <= n), spread with the given density pattern
static void fill(Table &t, std::mt19937_64 &rng, uint64_t n, uint64_t total, int pattern) {
    t.n = n;
    t.W.assign(n + 1, 0);
    t.last.assign(n + 1, 0);
    for (uint64_t i = 1; i <= n; ++i) t.W[i] = (uint8_t)(rng() % 10);
    // pattern 0: uniform; 1: the first half twice as dense as the second (a slope the interpolation must follow);
    // 2: runs of 300 edges without a bit (blocks the scan has to cross)
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i + 1;
    for (uint64_t i = n; i > 1; --i) std::swap(order[i - 1], order[rng() % i]);
    auto weight = [&](uint64_t i) -> int {
        if (pattern == 1) return i <= n / 2 ? 2 : 1;
        if (pattern == 2) return (i / 300) % 3 == 1 ? 0 : 2;
        return 1;
    };
    uint64_t have = 0;
    for (int pass = 2; pass >= 0 && have < total; --pass)
        for (uint64_t x = 0; x < n && have < total; ++x) {
            const uint64_t i = order[x];
            if (t.last[i] || weight(i) < pass) continue;
            if (pass == 2 && (rng() & 1)) continue;           // (the dense class first, half of it)
            t.last[i] = 1; ++have;
        }
}

static bool run(std::mt19937_64 &rng, uint64_t n, uint64_t total, int pattern, uint32_t max_entries, uint32_t want_shift, bool index_too) {
    Table t;
    fill(t, rng, n, total, pattern);
    build(t, max_entries);
    CHECK(t.g.sel_shift == want_shift, "n %llu total %llu entries %u: shift %u, wanted %u", (unsigned long long)n, (unsigned long long)total,
          max_entries, t.g.sel_shift, want_shift);
    CHECK(t.g.sel_n <= max_entries, "sel_n %u above %u", t.g.sel_n, max_entries);
    ++n_tables;
    if (!check_select(t)) { printf("  (n %llu total %llu pattern %d entries %u shift %u)\n", (unsigned long long)n, (unsigned long long)total, pattern, max_entries, t.g.sel_shift); return false; }
    if (index_too && !check_index(t)) { printf("  (n %llu total %llu pattern %d)\n", (unsigned long long)n, (unsigned long long)total, pattern); return false; }
    return true;
}

int main() {
    std::mt19937_64 rng(20240917);
    const uint32_t entries[] = { 4, 5, 7, 12, 33, 64 };
    const int density_pct[] = { 20, 35, 60, 90, 100 };            // one bit in 5 ... all ones
    const uint64_t residues[] = { 0, 1, 2, 63, 29 };              // (n + 1) mod 64: 0 = the final block exactly full
    uint64_t variant = 0;
    for (uint32_t E : entries)
        for (uint32_t shift = 6; shift <= 12; ++shift) {
            // sel_anchor_shift returns `shift` for totals with (total >> shift) + 2 <= E < (total >> (shift - 1)) + 2
            const uint32_t m_hi = E - 2, m_lo = shift == 6 ? 1 : (E - 2) / 2 + 1;
            for (uint32_t m : { m_lo, m_hi }) {
                if (m < 1 || ((uint64_t)m << shift) > 70000) continue;
                for (int d = -1; d <= 1; ++d) {
                    const uint64_t total = ((uint64_t)m << shift) + d;
                    if (sel_anchor_shift(total, E) != shift) continue;      // (m << shift) - 1 of the lowest m belongs to shift - 1: covered there
                    const int dens = density_pct[variant % 5];
                    uint64_t n = dens == 100 ? total : total * 100 / dens + 1;
                    if (dens != 100) { const uint64_t want = residues[(variant / 5) % 5]; while ((n + 1) % 64 != want) ++n; }
                    const int pattern = dens == 100 ? 0 : (int)(variant % 3);
                    ++variant;
                    if (!run(rng, n, total, pattern, E, shift, n <= 20000)) return 1;
                }
            }
        }
    // small tables: one block, two blocks, every residue of the edge count; all ones and one bit in 5
    for (uint64_t n = 1; n <= 200; ++n)
        for (int dens : { 20, 100 }) {
            const uint64_t total = dens == 100 ? n : (n + 4) / 5;
            if (!run(rng, n, total, 0, 4, sel_anchor_shift(total, 4), true)) return 1;
        }
    for (uint32_t s = 6; s <= 12; ++s)
        if (!pairs_of_shift[s]) { printf("FAIL no table with shift %u\n", s); return 1; }
    if (!n_span0) { printf("FAIL no table whose total is a multiple of 2^shift\n"); return 1; }
    printf("ok %llu (r, shift) pairs on %llu tables, shifts 6..12:", (unsigned long long)n_pairs, (unsigned long long)n_tables);
    for (uint32_t s = 6; s <= 12; ++s) printf(" %llu", (unsigned long long)pairs_of_shift[s]);
    printf("; %llu tables with total a multiple of 2^shift; scan steps per select: mean %.3f max %llu (hinted select: mean %.3f); "
           "%llu indices checked; %llu block loads, %llu outside the table\n",
           (unsigned long long)n_span0, (double)n_scan_steps / (double)n_pairs, (unsigned long long)max_scan_steps,
           (double)n_hint_steps / (double)n_pairs, (unsigned long long)n_index_checks, (unsigned long long)g_block_loads,
           (unsigned long long)g_block_loads_outside);
    return 0;
}
