// dbg_decode.hpp — the payloads of a `.dbg` file (boss_files.hpp: rrr_vector<63>, the Huffman-shaped wavelet tree of W, the
// int_vector of FAST-state graphs, the three forms of `last`) decoded into the W / last byte arrays of mgx_boss_view, one lane per
// item.  What parse_dbg (boss_files.hpp) does per edge on one host thread; the host still walks the container headers
// (dbg_plan.hpp).  The kernels are in mgx_dbgload.hip; every body here is an MGX_HD function over plain pointers, so that
// tests/emu/dbg_decode_check.cpp compiles this very file for the host, under the address sanitizer, with every array at the size
// dd_*_words / dd_byte_alloc give it.
//
// What every function relies on (the driver and the model provide it):
//   * every bit payload lies in an 8-byte-aligned array of its own of dd_words(bits) = ceil(bits / 64) + 2 words, the last two
//     zero: a field of up to 64 bits that BEGINS at a bit position <= bits is read with two word loads that stay inside;
//   * an index computed from file content (an offset into btnr, a position in the level bits, a child, an index into low, an sd
//     position) is compared with its array's length before it is used; on a failed check the lane records the check and its
//     position (dd_fail) and writes a zero;
//   * no loop's trip count depends on file content: un-ranking takes at most 63 steps, a walk at most DD_MAX_DEPTH, a word 64 bits.
// The error record is one 64-bit word, DD_NO_ERROR or (check << 48) | position, kept at its minimum: the checks are numbered in
// the order parse_dbg makes them, so the record names the check the host decoder would have failed first.
#pragma once
#include <stdint.h>
#include "wave.hpp"

namespace mgx {

enum DdCheck : uint32_t {
    DD_W_RRR_EARLY = 1,      // W (rrr levels): block numbers end early
    DD_W_RRR_CLASS,          // W (rrr levels): block number outside its class
    DD_W_SELECT,             // W: select supports disagree with the level bits (stored ones != popcount)
    DD_W_WALK,               // W (tree): walk leaves the level bit vector
    DD_W_CHILD,              // W (tree): child index outside the tree
    DD_W_SYMBOL,             // W (tree): symbol above 255
    DD_L_RRR_EARLY,          // last: block numbers end early
    DD_L_RRR_CLASS,          // last: block number outside its class
    DD_L_ONES,               // last: stored number of set bits differs from the vector's
    DD_L_SD_SELECT,          // last: select supports disagree with the high part
    DD_L_SD_ORDER,           // last: positions not ascending below size
    DD_W_ALPHABET,           // W symbol outside the alphabet (>= 2 * sigma)
    DD_CHECKS
};
constexpr uint64_t DD_NO_ERROR = ~0ull;
constexpr unsigned DD_MAX_DEPTH = 256;       // parse_dbg: depth > 255 is "walk leaves the level bit vector"
constexpr unsigned DD_MAX_NODES = 511;       // decode_wt: n_nodes > 511 is refused
constexpr unsigned DD_BINOM_ENTRIES = 63 * 32;     // C(n, j), n <= 62, j <= 31, at [n * 32 + j]

MGX_HD uint64_t dd_words(uint64_t bits) { return (bits + 63) / 64 + 2; }
MGX_HD uint64_t dd_byte_alloc(uint64_t n) { return (n + 7) & ~7ull; }      // byte arrays are written eight bytes per lane

MGX_HD void dd_fail(uint64_t *err, uint32_t check, uint64_t pos) {
    const uint64_t key = ((uint64_t)check << 48) | (pos < (1ull << 48) ? pos : (1ull << 48) - 1);
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(reinterpret_cast<unsigned long long *>(err), (unsigned long long)key);
#else
    if (key < *err) *err = key;
#endif
}

// int_vector::get_int(pos, len), len <= 64, pos <= the payload's bits (see above: both words are inside the array)
MGX_HD uint64_t dd_get(const uint64_t *w, uint64_t pos, unsigned len) {
    if (!len) return 0;
    const unsigned sh = (unsigned)(pos & 63);
    uint64_t v = w[pos >> 6] >> sh;
    if (sh) v |= w[(pos >> 6) + 1] << (64 - sh);
    return len == 64 ? v : v & ((1ull << len) - 1);
}

// the set bits of word wi of a vector of `bits` bits (bits behind the vector's end are not counted); wi < dd_words(bits)
MGX_HD uint64_t dd_word_masked(const uint64_t *w, uint64_t wi, uint64_t bits) {
    const uint64_t begin = wi * 64;
    if (begin >= bits) return 0;
    const uint64_t x = w[wi];
    return bits - begin >= 64 ? x : x & ((1ull << (bits - begin)) - 1);
}
MGX_HD uint64_t dd_popcount_word(const uint64_t *w, uint64_t wi, uint64_t bits) {
    return (uint64_t)__builtin_popcountll(dd_word_masked(w, wi, bits));
}

// ---- rrr_vector<63> -------------------------------------------------------------------------------------------------------------
// width[b] of block b's number in btnr: 0 for classes 0 and 63, else hi(C(63, bt[b])) + 1 (wtab, 64 entries);
// b == n_blocks: the zero that closes the scan.  b * 6 + 6 <= bt's bits for b < n_blocks (the plan checks it).
MGX_HD uint64_t dd_rrr_width(const uint64_t *bt, const uint8_t *wtab, uint64_t b, uint64_t n_blocks) {
    return b < n_blocks ? wtab[dd_get(bt, b * 6, 6)] : 0;
}

// block b (63 bits): its number, `len` bits at bit `pos` of btnr, un-ranked as read_rrr63 does.  C: DD_BINOM_ENTRIES binomials.
// *status: 0, or 1 (block numbers end early) / 2 (block number outside its class) with a zero block.
MGX_HD uint64_t dd_rrr_unrank(const uint64_t *bt, const uint64_t *btnr, uint64_t btnr_bits, uint64_t pos, const uint8_t *wtab,
                              const uint64_t *C, uint64_t b, unsigned *status) {
    *status = 0;
    const unsigned k = (unsigned)dd_get(bt, b * 6, 6);
    if (k == 63) return ~0ull >> 1;
    if (!k) return 0;
    const unsigned len = wtab[k];
    if (pos > btnr_bits || len > btnr_bits - pos) { *status = 1; return 0; }
    uint64_t nr = dd_get(btnr, pos, len);
    const bool inv = 2 * k > 63;
    unsigned j = inv ? 63 - k : k;                          // 1 .. 31
    uint64_t block = 0;
    for (unsigned p = 0; p < 63; ++p) {
        const uint64_t c = C[(62 - p) * 32 + (j & 31)];
        if (j && nr >= c) { nr -= c; --j; block |= 1ull << p; }
    }
    if (j || nr) { *status = 2; return 0; }
    return inv ? ~block & (~0ull >> 1) : block;
}
// off[b]: the scanned widths
MGX_HD uint64_t dd_rrr_block(const uint64_t *bt, const uint64_t *btnr, uint64_t btnr_bits, const uint64_t *off, const uint8_t *wtab,
                             const uint64_t *C, uint64_t b, uint64_t *err, uint32_t check_early) {
    unsigned status;
    const uint64_t block = dd_rrr_unrank(bt, btnr, btnr_bits, off[b], wtab, C, b, &status);
    if (status) dd_fail(err, check_early + status - 1, b);
    return block;
}

// word wi of the decoded vector from the at most two blocks that overlap it; wi < dd_words(bits): the pad words come out zero
MGX_HD uint64_t dd_rrr_pack(const uint64_t *blocks, uint64_t n_blocks, uint64_t bits, uint64_t wi) {
    const uint64_t begin = wi * 64;
    if (begin >= bits) return 0;
    const uint64_t b0 = begin / 63;
    const unsigned r = (unsigned)(begin - b0 * 63);         // 0 .. 62
    uint64_t x = b0 < n_blocks ? blocks[b0] >> r : 0;
    if (b0 + 1 < n_blocks) x |= blocks[b0 + 1] << (63 - r);
    return bits - begin >= 64 ? x : x & ((1ull << (bits - begin)) - 1);
}

// ---- wavelet tree ---------------------------------------------------------------------------------------------------------------
// a node as the walk reads it (LDS): r0 = rank1(bv_pos) — dd_wt_node; sym = min(bv_pos_rank, 256) of a leaf
struct DdNode { uint64_t bv_pos, r0; uint16_t child[2], sym, pad; };
static_assert(sizeof(DdNode) == 24, "DdNode");
// a node as the host plan uploads it (WtNode of boss_files.hpp in fixed-width fields)
struct DdRawNode { uint64_t bv_pos, bv_pos_rank; uint16_t child[2]; uint32_t pad; };
static_assert(sizeof(DdRawNode) == 24, "DdRawNode");

// rank1 of [0, at) over level bits bv with directory dir (dir[w] = set bits of words [0, w)); at <= bits
MGX_HD uint64_t dd_rank1(const uint64_t *bv, const uint64_t *dir, uint64_t at) {
    const unsigned sh = (unsigned)(at & 63);
    return dir[at >> 6] + (sh ? (uint64_t)__builtin_popcountll(bv[at >> 6] & ((1ull << sh) - 1)) : 0);
}
MGX_HD DdNode dd_wt_node(const DdRawNode &n, const uint64_t *bv, const uint64_t *dir, uint64_t bits) {
    DdNode d;
    d.bv_pos = n.bv_pos;
    d.r0 = n.bv_pos <= bits ? dd_rank1(bv, dir, n.bv_pos) : 0;      // (a node beyond the vector fails the walk before r0 is used)
    d.child[0] = n.child[0]; d.child[1] = n.child[1];
    d.sym = (uint16_t)(n.bv_pos_rank > 255 ? 256 : n.bv_pos_rank);
    d.pad = 0;
    return d;
}
// element i of the sequence.  pos = the element's place inside the node's stretch: i at the root; below, the number of earlier
// elements routed to the same child = the rank of its bit value inside the stretch (the host's cur[v]++).
MGX_HD uint8_t dd_wt_decode(const uint64_t *bv, const uint64_t *dir, uint64_t bits, const DdNode *nodes, uint32_t n_nodes,
                            uint32_t alphabet2, uint64_t i, uint64_t *err) {
    uint32_t v = 0;
    uint64_t pos = i;
    for (unsigned depth = 0; depth <= DD_MAX_DEPTH; ++depth) {
        const DdNode nd = nodes[v];
        if (nd.child[0] == 0xFFFF) {
            if (nd.sym > 255) { dd_fail(err, DD_W_SYMBOL, i); return 0; }
            if (nd.sym >= alphabet2) { dd_fail(err, DD_W_ALPHABET, i); return 0; }
            return (uint8_t)nd.sym;
        }
        if (depth == DD_MAX_DEPTH || nd.bv_pos >= bits || pos >= bits - nd.bv_pos) { dd_fail(err, DD_W_WALK, i); return 0; }
        const uint64_t at = nd.bv_pos + pos;
        const unsigned bit = (unsigned)((bv[at >> 6] >> (at & 63)) & 1);
        const uint64_t ones = dd_rank1(bv, dir, at) - nd.r0;
        pos = bit ? ones : pos - ones;
        v = bit ? nd.child[1] : nd.child[0];                   // (no runtime index into the register copy)
        if (v >= n_nodes) { dd_fail(err, DD_W_CHILD, i); return 0; }
    }
    return 0;
}

// ---- FAST state: element i of an int_vector of `width` <= 8 bits; (i + 1) * width <= the payload's bits ------------------------
MGX_HD uint8_t dd_unpack_int(const uint64_t *w, unsigned width, uint32_t alphabet2, uint64_t i, uint64_t *err) {
    const uint64_t x = dd_get(w, i * width, width);
    if (x >= alphabet2) { dd_fail(err, DD_W_ALPHABET, i); return 0; }
    return (uint8_t)x;
}

// ---- last -----------------------------------------------------------------------------------------------------------------------
// bits [8 t, 8 t + 8) of a vector as eight bytes (one store); 8 t < bits; bits behind the vector's end give zero bytes
MGX_HD uint64_t dd_expand8(const uint64_t *w, uint64_t bits, uint64_t t) {
    const uint64_t b = (dd_word_masked(w, t >> 3, bits) >> ((t & 7) * 8)) & 0xFF;
    const uint64_t x = (b * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
}

// sd_vector: word wi of `high` (rank[wi] set bits before it): pos[i] = ((p - i) << wl) | low[i] for its set bits p, i their
// index among all set bits.  pos has m entries, low low_n of wl bits.
MGX_HD void dd_sd_word(const uint64_t *high, uint64_t high_bits, const uint64_t *rank, const uint64_t *low, uint64_t low_n, unsigned wl,
                       uint64_t wi, uint64_t *pos, uint64_t m, uint64_t *err, uint32_t check_select) {
    uint64_t x = dd_word_masked(high, wi, high_bits), i = rank[wi];
    for (unsigned t = 0; t < 64 && x; ++t, ++i, x &= x - 1) {
        if (i >= m || i >= low_n) { dd_fail(err, check_select, i); return; }
        const uint64_t p = wi * 64 + (uint64_t)__builtin_ctzll(x);
        pos[i] = ((p - i) << wl) | (wl ? dd_get(low, i * wl, wl) : 0);
    }
}
// one lane per set bit: the position's byte, after the checks of read_sd_vector.  out: `size` bytes, all inverted ? 1 : 0 before
MGX_HD void dd_sd_scatter(const uint64_t *pos, uint64_t i, uint64_t size, uint8_t *out, bool inverted, uint64_t *err, uint32_t check_order) {
    const uint64_t v = pos[i];
    if (v >= size || (i && v <= pos[i - 1])) { dd_fail(err, check_order, i); return; }
    out[v] = inverted ? 0 : 1;
}

} // namespace mgx
