// tests/emu/dbg_decode_check.cpp — TEST ONLY: metagraph_amd/csrc/dbg_decode.hpp (the kernel bodies behind mgx_graph_load_dbg_device)
// run on the host, one call per item in the order of the launches of mgx_dbgload.hip, over the plan of dbg_plan.hpp.  Built with
// -fsanitize=address,undefined by tests/test_dbg_decode_model.py; every array has exactly the size the driver gives its device
// buffer, so that an access the kernels would make outside a buffer stops the program.
// usage: dbg_decode_check IN.dbg OUT.bin [IN.dbg OUT.bin ...]; one line per file:
//   "ok <n_edges>" (OUT.bin: k, sigma, mode, state, n_edges as u64, F, W, last), "invalid <message>" or "unsupported <message>"
#include "wave.hpp"
#include "../../metagraph_amd/csrc/dbg_decode.hpp"
#include "../../metagraph_amd/csrc/dbg_plan.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace mgx;
using namespace mgx::files;

typedef std::vector<uint64_t> Words;

static Words payload(const RawVec &v) {                     // upload(): the file's words and two zero words
    Words w(dd_words(v.bits), 0);
    if (v.words()) memcpy(w.data(), v.src, v.words() * 8);
    return w;
}
static void scan(Words &d) {
    uint64_t s = 0;
    for (uint64_t &x : d) { const uint64_t c = x; x = s; s += c; }
}

struct Tables { std::vector<uint8_t> wtab; Words binom; };
static Tables tables() {
    Tables t;
    const auto &C = binomial63().c;
    t.wtab.resize(64);
    t.binom.resize(DD_BINOM_ENTRIES);
    for (unsigned k = 0; k < 64; ++k) t.wtab[k] = (k == 0 || k == 63) ? 0 : (uint8_t)(64 - __builtin_clzll(C[63][k]));
    for (unsigned n = 0; n < 63; ++n) for (unsigned j = 0; j < 32; ++j) t.binom[n * 32 + j] = C[n][j];
    return t;
}

static Words decode_rrr(const RrrPlan &r, const Tables &t, uint64_t *err, uint32_t check_early) {
    const Words bt = payload(r.bt), btnr = payload(r.btnr);
    Words off(r.n_blocks + 1), blocks(r.n_blocks);
    for (uint64_t b = 0; b <= r.n_blocks; ++b) off[b] = dd_rrr_width(bt.data(), t.wtab.data(), b, r.n_blocks);
    scan(off);
    for (uint64_t b = 0; b < r.n_blocks; ++b)
        blocks[b] = dd_rrr_block(bt.data(), btnr.data(), r.btnr.bits, off.data(), t.wtab.data(), t.binom.data(), b, err, check_early);
    Words out(dd_words(r.bits));
    for (uint64_t wi = 0; wi < out.size(); ++wi) out[wi] = dd_rrr_pack(blocks.data(), r.n_blocks, r.bits, wi);
    return out;
}
static Words rank_directory(const Words &w, uint64_t bits) {
    Words dir(dd_words(bits));
    for (uint64_t wi = 0; wi < dir.size(); ++wi) dir[wi] = dd_popcount_word(w.data(), wi, bits);
    scan(dir);
    return dir;
}
static std::vector<uint8_t> expand_bits(const Words &w, uint64_t bits) {
    Words out8(dd_byte_alloc(bits) / 8);
    for (uint64_t t = 0; t < (bits + 7) / 8; ++t) out8[t] = dd_expand8(w.data(), bits, t);
    std::vector<uint8_t> out(bits);
    if (bits) memcpy(out.data(), out8.data(), bits);
    return out;
}

static std::vector<uint8_t> decode_W(const DbgPlan &p, const Tables &t, uint64_t *err) {
    const uint32_t alphabet2 = 2 * p.head.sigma;
    std::vector<uint8_t> W(p.w_size);
    if (p.w_kind == W_INT_VECTOR) {
        const Words iv = payload(p.w_bv);
        for (uint64_t i = 0; i < p.w_size; ++i) W[i] = dd_unpack_int(iv.data(), p.w_bv.width, alphabet2, i, err);
        return W;
    }
    const Words bv = p.w_kind == W_TREE_RRR ? decode_rrr(p.w_rrr, t, err, DD_W_RRR_EARLY) : payload(p.w_bv);
    const uint64_t bits = p.level_bits();
    const Words dir = rank_directory(bv, bits);
    if (p.w_kind == W_TREE_PLAIN && dir[(bits + 63) / 64] != p.w_ones) dd_fail(err, DD_W_SELECT, dir[(bits + 63) / 64]);
    std::vector<DdNode> nodes(p.nodes.size());
    for (size_t x = 0; x < nodes.size(); ++x) {
        const DdRawNode raw = { p.nodes[x].bv_pos, p.nodes[x].bv_pos_rank, { p.nodes[x].child[0], p.nodes[x].child[1] }, 0 };
        nodes[x] = dd_wt_node(raw, bv.data(), dir.data(), bits);
    }
    for (uint64_t i = 0; i < p.w_size; ++i) W[i] = dd_wt_decode(bv.data(), dir.data(), bits, nodes.data(), (uint32_t)nodes.size(), alphabet2, i, err);
    return W;
}

static std::vector<uint8_t> decode_last(const DbgPlan &p, const Tables &t, uint64_t *err) {
    if (p.last_code == CODE_RRR) return expand_bits(decode_rrr(p.l_rrr, t, err, DD_L_RRR_EARLY), p.l_rrr.bits);
    if (p.last_code == CODE_STAT) {
        const Words v = payload(p.l_stat.v);
        const Words dir = rank_directory(v, p.l_stat.v.bits);
        if (dir[p.l_stat.v.words()] != p.l_stat.ones) dd_fail(err, DD_L_ONES, dir[p.l_stat.v.words()]);
        return expand_bits(v, p.l_stat.v.bits);
    }
    const SdPlan &s = p.l_sd;
    const Words low = payload(s.low), high = payload(s.high);
    const Words rank = rank_directory(high, s.high.bits);
    const uint64_t m = rank[s.high.words()];
    std::vector<uint8_t> out;
    if (m != s.ones || s.zeros != s.high.bits - m || s.low.size() < m) { dd_fail(err, DD_L_SD_SELECT, m); return out; }
    out.assign(s.size, s.inverted ? 1 : 0);
    Words pos(m);
    for (uint64_t wi = 0; wi < s.high.words(); ++wi)
        dd_sd_word(high.data(), s.high.bits, rank.data(), low.data(), s.low.size(), s.wl, wi, pos.data(), m, err, DD_L_SD_SELECT);
    for (uint64_t i = 0; i < m; ++i) dd_sd_scatter(pos.data(), i, s.size, out.data(), s.inverted, err, DD_L_SD_ORDER);
    return out;
}

static void one(const std::string &in, const std::string &out_path) {
    try {
        const std::vector<uint8_t> image = read_whole_file(in);
        // the image at its exact size on the heap: the plan's spans are checked against it
        const DbgPlan p = plan_dbg(image.data(), image.size());
        std::vector<uint8_t> W, last;
        if (p.host_decode) {
            BossFile g = parse_dbg(image.data(), image.size());
            W = g.W; last = g.last;
        } else {
            const Tables t = tables();
            uint64_t err = DD_NO_ERROR;
            W = decode_W(p, t, &err);
            last = decode_last(p, t, &err);
            if (err != DD_NO_ERROR) { printf("invalid %s (at %llu)\n", dd_check_message((uint32_t)(err >> 48)), (unsigned long long)(err & ((1ull << 48) - 1))); return; }
        }
        FILE *f = fopen(out_path.c_str(), "wb");
        if (!f) { printf("invalid cannot write %s\n", out_path.c_str()); return; }
        const uint64_t hdr[5] = { p.head.k, p.head.sigma, p.head.mode, p.head.state, p.head.n_edges };
        fwrite(hdr, 8, 5, f);
        fwrite(p.head.F.data(), 8, p.head.F.size(), f);
        fwrite(W.data(), 1, W.size(), f);
        fwrite(last.data(), 1, last.size(), f);
        fclose(f);
        printf("ok %llu\n", (unsigned long long)p.head.n_edges);
    } catch (const Unsupported &e) {
        printf("unsupported %s\n", e.what());
    } catch (const ParseError &e) {
        printf("invalid %s\n", e.what());
    }
}

int main(int argc, char **argv) {
    if (argc < 3 || (argc & 1) == 0) { fprintf(stderr, "usage: %s IN.dbg OUT.bin [IN.dbg OUT.bin ...]\n", argv[0]); return 2; }
    for (int a = 1; a + 1 < argc; a += 2) one(argv[a], argv[a + 1]);
    return 0;
}
