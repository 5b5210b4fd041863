// bv_decode.hpp — a batch of sdsl bit vectors (sd, inverted sd, stat, rrr<63>) that lie side by side in one arena, turned into bit
// maps and a rank scan over them: the stage that the binary columns of a `.column.annodbg` load (col_decode.hpp) and the
// delimiter vectors of its tuple sections (coord_decode.hpp) share.  The kernels are in mgx_colload.hip, the layout of the arena
// and the tables in col_plan.hpp (BvBatch); every body is an MGX_HD function over plain pointers, so that tests/emu compiles this
// very file for the host, under the address sanitizer, with every array at the size the driver gives its device buffer
// (tests/emu/bv_stage.hpp).  DESIGN 3.17.
//
// One arena of 64-bit words holds every payload: the vectors' bt, btnr, low, high and plain-bit payloads as they stand in the
// file, each on a word boundary, each section closed by two zero words (the rule of dbg_decode.hpp: a field of up to 64 bits that
// begins inside a payload is read with two word loads that stay inside the arena), and behind them one bit map of ceil(bits / 64)
// words for every rrr vector (its packed blocks) and every sd vector that wants one (its stored positions); a stat vector's
// payload is its bit map.  A vector's length is its own, so an item (an rrr block, a word of the concatenated high parts, a word
// of the concatenated bit maps) finds its vector by a binary search of 32 fixed steps over a prefix table: rbprefix[t] = the
// first block of rrr vector t, hprefix[s] = the first high word of sd vector s, bmprefix[m] = the first word of bit map m.  Where
// all vectors of a batch have the same length (the binary columns) the blocks and the map words find theirs by a division (bv_find).
//
// As in dbg_decode.hpp: an index computed from file content is compared with its array's length before use, no trip count depends
// on file content, and a lane whose check fails records (label, check, position) in one 64-bit word kept at its minimum and
// writes nothing out of range.  Whatever the record says, the caller asks the host reader for the message (col_plan.hpp).
#pragma once
#include <stdint.h>
#include "dbg_decode.hpp"

namespace mgx {

enum CdCheck : uint32_t {
    CD_RRR_EARLY = 1,        // block numbers end early
    CD_RRR_CLASS,            // block number outside its class
    CD_STAT_ONES,            // stored number of set bits differs from the vector's
    CD_STAT_TAIL,            // a bit is set behind the vector's last position
    CD_SD_SELECT,            // select supports disagree with the high part (ones != popcount(high), or an index into low)
    CD_SD_SHIFT,             // the upper part of a position does not fit 64 bits when shifted by wl
    CD_SD_ORDER,             // positions not ascending below size
    CD_OUT_RANGE,            // an output index outside the column's range of rows[] (the counts and the write pass disagree)
    CD_CHECKS
};
enum CdKind : uint32_t { CD_KIND_SD = 0, CD_KIND_SD_INVERTED, CD_KIND_STAT, CD_KIND_RRR };
constexpr uint32_t BV_NO_MAP = ~0u;

// per rrr vector: word offsets into the arena of bt, btnr and of the vector's bit map (map `map` of the batch); its bits; its label
struct BvRrr { uint64_t bt_begin, btnr_begin, btnr_bits, bm_begin, bits; uint32_t label, map; };
static_assert(sizeof(BvRrr) == 48, "BvRrr");
// per sd vector; map: its bit map among the batch's (bm_begin: that map's words), BV_NO_MAP: a plain sd column, whose positions
// are its rows
struct CdSd { uint64_t low_begin, high_begin, high_bits, low_n, ones, bm_begin; uint32_t wl, inverted, label, map; };
static_assert(sizeof(CdSd) == 64, "CdSd");
// per bit map (stat: the payload itself; rrr, sd: the map behind the payloads), in label order
struct BvMap { uint64_t src_begin, bits, stat_ones; uint32_t kind, label; };
static_assert(sizeof(BvMap) == 32, "BvMap");

MGX_HD void cd_fail(uint64_t *err, uint32_t label, uint32_t check, uint64_t pos) {
    const uint64_t key = ((uint64_t)(label & 0xFFFFFFu) << 40) | ((uint64_t)check << 32) | (pos < 0xFFFFFFFFull ? pos : 0xFFFFFFFFull);
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(reinterpret_cast<unsigned long long *>(err), (unsigned long long)key);
#else
    if (key < *err) *err = key;
#endif
}

// the largest s < n with prefix[s] <= x (prefix ascending, prefix[0] = 0 <= x < prefix[n]); 32 fixed steps: n < 2^24 + 1
MGX_HD uint32_t cd_find(const uint64_t *prefix, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    for (unsigned t = 0; t < 32; ++t) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (hi - lo > 1) { if (prefix[mid] <= x) lo = mid; else hi = mid; }
    }
    return lo;
}

// the vector of item x of a concatenated buffer: the largest t < n with prefix[t] <= x < prefix[n].  stride != 0: every vector of
// the batch has that many items (prefix[t] = t * stride: the binary columns of a load, all of n_rows bits), and the search is a
// division
MGX_HD uint32_t bv_find(const uint64_t *prefix, uint32_t n, uint64_t stride, uint64_t x) {
    return stride ? (uint32_t)(x / stride) : cd_find(prefix, n, x);
}

// ---- rrr vectors: global block gb of the concatenated vectors (rb_stride: bv_find's stride over rbprefix) ---------------------
// width[gb], gb <= rbprefix[n_rrr] (the last: the zero that closes the scan).  b * 6 + 6 <= the vector's bt bits (the plan)
MGX_HD uint64_t bv_rrr_width(const uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride, const uint8_t *wtab,
                             uint64_t gb) {
    if (gb >= rbprefix[n_rrr]) return 0;
    const uint32_t t = bv_find(rbprefix, n_rrr, rb_stride, gb);
    return wtab[dd_get(arena + rd[t].bt_begin, (gb - rbprefix[t]) * 6, 6)];
}
// off: the scan of the widths over all blocks; the block's offset in its vector's btnr = off[gb] - off[the vector's first block]
MGX_HD uint64_t bv_rrr_block(const uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride, const uint64_t *off,
                             const uint8_t *wtab, const uint64_t *C, uint64_t gb, uint64_t *err) {
    const uint32_t t = bv_find(rbprefix, n_rrr, rb_stride, gb);
    const BvRrr d = rd[t];
    const uint64_t b = gb - rbprefix[t];
    unsigned status;
    const uint64_t block = dd_rrr_unrank(arena + d.bt_begin, arena + d.btnr_begin, d.btnr_bits, off[gb] - off[rbprefix[t]], wtab, C, b, &status);
    if (status) cd_fail(err, d.label, status == 1 ? CD_RRR_EARLY : CD_RRR_CLASS, b);
    return block;
}
// word w of the vector's bit map, by the lane of the vector's block w: ceil(bits / 63) blocks are no fewer than ceil(bits / 64) words
MGX_HD void bv_rrr_pack(uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride, const uint64_t *blocks,
                        uint64_t gb) {
    const uint32_t t = bv_find(rbprefix, n_rrr, rb_stride, gb);
    const BvRrr d = rd[t];
    const uint64_t w = gb - rbprefix[t];
    if (w * 64 < d.bits) arena[d.bm_begin + w] = dd_rrr_pack(blocks + rbprefix[t], rbprefix[t + 1] - rbprefix[t], d.bits, w);
}

// ---- sd vectors: global word gw of the concatenated high parts ----------------------------------------------------------------
MGX_HD uint64_t bv_high_popcount(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, uint64_t gw) {
    if (gw >= hprefix[n_sd]) return 0;
    const uint32_t s = cd_find(hprefix, n_sd, gw);
    return dd_popcount_word(arena + sd[s].high_begin, gw - hprefix[s], sd[s].high_bits);
}
// The set bits p of word lw of d's high part, the i-th of their vector: the position ((p - i) << wl) | low[i] after the checks of
// read_sd_vector; sink(i, v): the i-th position v, false to stop.
// Order: p rises with i, so the upper parts p - i never fall, and two positions can be out of order only where the upper parts
// are equal, which is where bit p - 1 of high is set as well: then, and only then, low[i] must exceed low[i - 1].
template <class Sink>
MGX_HD void cd_sd_each(const uint64_t *arena, const CdSd &d, uint64_t lw, uint64_t i, uint64_t size, uint64_t *err, Sink &&sink) {
    const uint64_t *high = arena + d.high_begin, *low = arena + d.low_begin;
    const uint64_t word = dd_word_masked(high, lw, d.high_bits);
    uint64_t x = word;
    const uint64_t before = lw ? high[lw - 1] >> 63 : 0;                // bit p - 1 of the word's first bit
    for (unsigned t = 0; t < 64 && x; ++t, ++i, x &= x - 1) {
        if (i >= d.ones || i >= d.low_n) { cd_fail(err, d.label, CD_SD_SELECT, i); return; }
        const unsigned b = (unsigned)__builtin_ctzll(x);
        const uint64_t up = lw * 64 + b - i;
        const uint64_t lo = d.wl ? dd_get(low, i * d.wl, d.wl) : 0;
        if (d.wl && (up >> (64 - d.wl))) { cd_fail(err, d.label, CD_SD_SHIFT, i); return; }
        const uint64_t v = (up << d.wl) | lo;
        const bool adjacent = b ? (word >> (b - 1)) & 1 : before != 0;
        if (v >= size || (i && adjacent && lo <= (d.wl ? dd_get(low, (i - 1) * d.wl, d.wl) : 0))) { cd_fail(err, d.label, CD_SD_ORDER, i); return; }
        if (!sink(i, v)) return;
    }
}
MGX_HD void cd_set_bit(uint64_t *word, unsigned bit) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(reinterpret_cast<unsigned long long *>(word), 1ull << bit);
#else
    *word |= 1ull << bit;
#endif
}
// every stored position of the sd vectors that have a bit map into that map, cleared before.  hrank: the scan of bv_high_popcount
MGX_HD void bv_sd_scatter(uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank, const BvMap *map, uint64_t gw,
                          uint64_t *err) {
    const uint32_t s = cd_find(hprefix, n_sd, gw);
    const CdSd d = sd[s];
    if (d.map == BV_NO_MAP) return;
    cd_sd_each(arena, d, gw - hprefix[s], hrank[gw] - hrank[hprefix[s]], map[d.map].bits, err, [&](uint64_t, uint64_t v) {
        cd_set_bit(arena + d.bm_begin + (v >> 6), (unsigned)(v & 63));
        return true;
    });
}

// ---- bit maps: global word g of the concatenated maps (bm_stride: bv_find's stride over bmprefix) -----------------------------
// word w of the vector behind map d: an inverted vector's map complemented, nothing behind the last bit
MGX_HD uint64_t bv_map_word(const uint64_t *arena, const BvMap &d, uint64_t w) {
    uint64_t x = arena[d.src_begin + w];
    if (d.kind == CD_KIND_SD_INVERTED) x = ~x;
    const uint64_t left = d.bits - w * 64;                                 // >= 1
    return left >= 64 ? x : x & ((1ull << left) - 1);
}
// cnt[g], g <= bmprefix[n_map] (the last: the zero that closes the scan)
MGX_HD uint64_t bv_map_popcount(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_map, uint64_t bm_stride, uint64_t g) {
    if (g >= bmprefix[n_map]) return 0;
    const uint32_t m = bv_find(bmprefix, n_map, bm_stride, g);
    return (uint64_t)__builtin_popcountll(bv_map_word(arena, map[m], g - bmprefix[m]));
}

} // namespace mgx
