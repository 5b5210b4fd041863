// dbg_plan.hpp — the host half of mgx_graph_load_dbg_device: the walk over the container headers of a `.dbg` file that parse_dbg
// (boss_files.hpp) makes, with the same Cursor, the same skip functions and the same header-level checks and messages, but
// without decoding a payload: every payload is noted as a span of the file image (RawVec), to be copied into a device buffer of its
// own and decoded by the kernels of dbg_decode.hpp.  Host code; used by mgx_dbgload.hip and by tests/emu/dbg_decode_check.cpp.
// The per-element checks of parse_dbg are the kernels' (DdCheck); dd_check_message gives each the host decoder's words.
#pragma once
#include "boss_files.hpp"

namespace mgx { namespace files {

struct RawVec {                                  // ceil(bits / 64) words at src (any alignment, inside the file image)
    const uint8_t *src = nullptr;
    uint64_t bits = 0;
    uint8_t width = 1;
    uint64_t words() const { return (bits + 63) / 64; }
    uint64_t size() const { return width ? bits / width : 0; }
};
// the vector a read_*_vector(c, ..., keep = false) call has just stepped over
inline RawVec raw_behind(const Cursor &c, const uint8_t *base, const Bits &b) {
    RawVec r;
    r.bits = b.bits; r.width = b.width;
    r.src = base + c.at() - r.words() * 8;
    return r;
}

struct RrrPlan { uint64_t bits = 0, n_blocks = 0; RawVec bt, btnr; };
inline RrrPlan plan_rrr63(Cursor &c, const uint8_t *base, const char *what) {       // the header part of read_rrr63
    RrrPlan r;
    r.bits = c.le(what);
    r.bt = raw_behind(c, base, read_int_vector(c, what, false));
    r.btnr = raw_behind(c, base, read_fixed_vector(c, 1, what, false));
    read_int_vector(c, what, false);
    read_int_vector(c, what, false);
    if (r.bt.width != 6 && r.bt.size()) throw ParseError(std::string(what) + ": block types are not 6 bits wide (not an rrr_vector<63>)");
    if (r.bits > r.bt.size() * 63) throw ParseError(std::string(what) + ": fewer block types than blocks");
    r.n_blocks = (r.bits + 62) / 63;
    return r;
}

struct StatPlan { RawVec v; uint64_t ones = 0; };
inline StatPlan plan_bit_vector_stat(Cursor &c, const uint8_t *base, const char *what) {       // read_bit_vector_stat
    StatPlan s;
    s.v = raw_behind(c, base, read_fixed_vector(c, 1, what, false));
    s.ones = c.be(what);
    skip_rank_support(c, s.v.bits, 11, what);
    if (skip_select_mcl(c, what) != s.ones) throw ParseError(std::string(what) + ": stored number of set bits differs from the vector's");
    return s;
}

struct SdPlan { uint64_t size = 0, ones = 0, zeros = 0; uint8_t wl = 0; RawVec low, high; bool inverted = false; };
inline SdPlan plan_sd_vector(Cursor &c, const uint8_t *base, const char *what, uint64_t expect) {      // the header part of read_sd_vector
    SdPlan s;
    s.size = c.le(what);
    if (s.size != expect) throw ParseError(std::string(what) + ": " + std::to_string(s.size) + " bits, expected " + std::to_string(expect));
    s.wl = c.u8(what);
    s.low = raw_behind(c, base, read_int_vector(c, what, false));
    s.high = raw_behind(c, base, read_fixed_vector(c, 1, what, false));
    s.ones = skip_select_mcl(c, what);
    s.zeros = skip_select_mcl(c, what);
    if (s.wl > 63 || (s.low.size() && s.low.width != s.wl)) throw ParseError(std::string(what) + ": low part width differs from wl");
    return s;
}

enum { W_TREE_RRR = 0, W_TREE_PLAIN, W_INT_VECTOR };
struct DbgPlan {
    BossFile head;                               // k, mode, state, sigma, F; n_edges; no arrays
    unsigned logsigma = 0;
    bool host_decode = false;                    // the node table is not a tree: parse_dbg decodes this file (see plan_dbg)
    int w_kind = W_TREE_RRR;
    uint64_t w_size = 0;                         // elements of W
    RrrPlan w_rrr;                               // W_TREE_RRR: the level bits
    RawVec w_bv;                                 // W_TREE_PLAIN: the level bits; W_INT_VECTOR: the sequence
    uint64_t w_ones = 0;                         // W_TREE_PLAIN: arguments of select_1
    std::vector<WtNode> nodes;
    uint64_t last_code = CODE_STAT;
    RrrPlan l_rrr;
    StatPlan l_stat;
    SdPlan l_sd;
    uint64_t level_bits() const { return w_kind == W_TREE_RRR ? w_rrr.bits : w_bv.bits; }
};

inline DbgPlan plan_dbg(const uint8_t *data, size_t n) {
    Cursor c(data, n);
    DbgPlan p;
    BossFile &g = p.head;
    const uint64_t nf = c.be("F");
    if (nf < 2 || nf > 64) throw ParseError("F has " + std::to_string(nf) + " entries");
    g.sigma = (uint32_t)nf;
    for (uint64_t i = 0; i < nf; ++i) g.F.push_back(c.be("F"));
    unsigned logsigma = 1;
    while ((1u << (logsigma - 1)) < nf) ++logsigma;
    p.logsigma = logsigma;
    const uint64_t boss_k = c.be("k");
    if (boss_k < 1 || boss_k > 255) throw ParseError("k out of range");
    g.k = (uint32_t)boss_k + 1;
    g.state = (uint32_t)c.be("state");
    uint64_t last_bits = 0;
    auto wt = [&](bool rrr) {
        p.w_size = c.le("W");
        const uint64_t sigma = c.le("W");
        if (rrr) { p.w_kind = W_TREE_RRR; p.w_rrr = plan_rrr63(c, data, "W (rrr levels)"); }
        else {
            p.w_kind = W_TREE_PLAIN;
            p.w_bv = raw_behind(c, data, read_fixed_vector(c, 1, "W (levels)", false));
            skip_rank_support(c, p.w_bv.bits, 9, "W (rank_support_v)");
            p.w_ones = skip_select_mcl(c, "W (select_1)");
            const uint64_t zeros = skip_select_mcl(c, "W (select_0)");
            if (p.w_ones > p.w_bv.bits || zeros != p.w_bv.bits - p.w_ones) throw ParseError("W: select supports disagree with the level bits");
        }
        const char *what = "W (tree)";                          // the header part of decode_wt
        const uint64_t n_nodes = c.le(what);
        if (n_nodes > 511 || (sigma && n_nodes != 2 * sigma - 1)) throw ParseError(std::string(what) + ": tree size does not fit sigma");
        p.nodes.resize(n_nodes);
        for (auto &v : p.nodes) { v.bv_pos = c.le(what); v.bv_pos_rank = c.le(what); v.parent = c.u16(what); v.child[0] = c.u16(what); v.child[1] = c.u16(what); }
        c.take(256 * 2 + 256 * 8, what);
        if (p.w_size && (n_nodes < 3 || p.w_size > p.level_bits()))
            throw ParseError(std::string(what) + ": " + std::to_string(p.w_size) + " elements over " + std::to_string(p.level_bits()) + " level bits");
        if (c.be("W (logsigma)") != logsigma) throw ParseError("W: logsigma does not fit the alphabet");
        // The kernels' walk takes an element's place below a node from the rank of its bit inside the node's stretch, which is
        // the host's per-node counter only while every node is entered from one place.  A table in which a node is
        // the child of two links, or the root a child, or a stretch begins beyond 2^63 (the host's position would wrap), is
        // left to the host decoder, whatever it makes of it.
        std::vector<uint8_t> entered(n_nodes, 0);
        for (const WtNode &v : p.nodes) {
            if (v.child[0] == 0xFFFF) continue;
            if (v.bv_pos >> 63) p.host_decode = true;
            for (uint16_t ch : v.child) if (ch < n_nodes && (ch == 0 || entered[ch]++)) p.host_decode = true;
        }
    };
    auto stat_last = [&]() { p.last_code = CODE_STAT; p.l_stat = plan_bit_vector_stat(c, data, "last"); last_bits = p.l_stat.v.bits; };
    switch (g.state) {
        case STATE_STAT: wt(false); stat_last(); break;
        case STATE_SMALL: {
            wt(true);
            p.last_code = c.be("last");                         // read_adaptive
            if (p.last_code == CODE_RRR) { p.l_rrr = plan_rrr63(c, data, "last"); last_bits = p.l_rrr.bits; }
            else if (p.last_code == CODE_STAT) { p.l_stat = plan_bit_vector_stat(c, data, "last"); last_bits = p.l_stat.v.bits; }
            else if (p.last_code == CODE_SD) {
                p.l_sd = plan_sd_vector(c, data, "last", p.w_size);
                p.l_sd.inverted = c.u8("last") != 0;
                last_bits = p.l_sd.size;
            } else if (p.last_code == CODE_IL4096) throw Unsupported("last: bit_vector_il<4096> is not read");
            else throw ParseError("last: unknown bit vector representation " + std::to_string(p.last_code));
            break;
        }
        case STATE_FAST: {
            p.w_kind = W_INT_VECTOR;
            p.w_bv = raw_behind(c, data, read_int_vector(c, "W (int_vector)", false));
            if (p.w_bv.width != logsigma) throw ParseError("W: int_vector width does not fit the alphabet");
            p.w_size = p.w_bv.size();
            for (unsigned j = 0; j < (1u << logsigma); ++j) read_bit_vector_stat(c, "W (bitmap)");      // (as parse_dbg: read, checked, dropped)
            stat_last();
            break;
        }
        case STATE_DYN: throw Unsupported("DYN-state graphs are not read: `metagraph transform --state small|stat|fast` first");
        default: throw ParseError("unknown BOSS state " + std::to_string(g.state));
    }
    if (!p.w_size || last_bits != p.w_size) throw ParseError("W and last differ in length");
    g.n_edges = p.w_size - 1;
    for (uint64_t i = 0; i < nf; ++i) if (g.F[i] > g.n_edges || (i && g.F[i] < g.F[i - 1])) throw ParseError("F is not ascending below the number of edges");
    const uint64_t mode = c.be("mode");
    if (mode > 2) throw ParseError("unknown graph mode " + std::to_string(mode));
    g.mode = (uint32_t)mode;
    return p;
}

// the words parse_dbg has for a check of the kernels (DdCheck, dbg_decode.hpp)
inline const char *dd_check_message(uint32_t check) {
    static const char *const text[] = {
        "", "W (rrr levels): block numbers end early", "W (rrr levels): block number outside its class",
        "W: select supports disagree with the level bits", "W (tree): walk leaves the level bit vector",
        "W (tree): child index outside the tree", "W (tree): symbol above 255", "last: block numbers end early",
        "last: block number outside its class", "last: stored number of set bits differs from the vector's",
        "last: select supports disagree with the high part", "last: positions not ascending below size",
        "W symbol outside the alphabet" };
    return check < sizeof(text) / sizeof(text[0]) ? text[check] : "unknown check";
}

}}  // namespace mgx::files
