// col_decode.hpp — the columns of `.column.annodbg` files (boss_files.hpp: parse_columns) decoded into the set rows that
// mgx_annotation_create_sparse takes, batched over ALL columns of a load: one lane per item of a concatenated buffer (an rrr block,
// a word of an sd_vector's high part, a word of a column's bit map), the item's column found from a small descriptor table.
// The kernels are in mgx_colload.hip, the layout of the buffers and tables in col_plan.hpp (ColBatch); every body here is an
// MGX_HD function over plain pointers, so that tests/emu/col_decode_check.cpp compiles this very file for the host, under the
// address sanitizer, with every array at the size ColBatch gives it.  DESIGN 3.17.
//
// One arena of 64-bit words holds every payload (ColBatch): the columns' bt, btnr, low, high and plain-bit payloads as they stand
// in the file, each on a word boundary, each section closed by two zero words (the rule of dbg_decode.hpp: a field of up to 64
// bits that begins inside a payload is read with two word loads that stay inside the arena), and behind them one bit map of
// W = ceil(n_rows / 64) words for every rrr column (its packed blocks) and every inverted sd column (its stored positions).
// Every column has n_rows bits (the plan refuses a file in which one does not), so an rrr block or a bit-map word finds its column
// by a division; a word of the concatenated high parts finds it by a binary search of 32 fixed steps over the word prefixes.
//
// As in dbg_decode.hpp: an index computed from file content is compared with its array's length before use, no trip count depends
// on file content, and a lane whose check fails records (column, check, position) in one 64-bit word kept at its minimum and
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

// per rrr column: word offsets into the arena of bt, btnr and of the column's bit map; the column's label
struct CdRrr { uint64_t bt_begin, btnr_begin, btnr_bits, bm_begin; uint32_t label, pad; };
static_assert(sizeof(CdRrr) == 40, "CdRrr");
// per sd column; bm_begin: the bit map of an inverted column.  (Its high part's place among all high words: the prefix table)
struct CdSd { uint64_t low_begin, high_begin, high_bits, low_n, ones, bm_begin; uint32_t wl, inverted, label, pad; };
static_assert(sizeof(CdSd) == 64, "CdSd");
// per bit-map column (stat: the payload itself; rrr, inverted sd: the map behind the payloads), in label order
struct CdBm { uint64_t src_begin, stat_ones; uint32_t kind, label; };
static_assert(sizeof(CdBm) == 24, "CdBm");
// per label: CD_KIND_*, its index among the sd columns (sd kinds) and among the bit-map columns (all but plain sd)
struct CdLabel { uint32_t kind, sd, bm, pad; };
static_assert(sizeof(CdLabel) == 16, "CdLabel");

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

// ---- rrr columns: global block gb = t * n_blocks + b of rrr column t ------------------------------------------------------------
// width[gb], gb <= n_rrr * n_blocks (the last: the zero that closes the scan).  b * 6 + 6 <= the column's bt bits (the plan)
MGX_HD uint64_t cd_rrr_width(const uint64_t *arena, const CdRrr *rd, const uint8_t *wtab, uint64_t gb, uint64_t n_blocks, uint64_t n_rrr) {
    if (gb >= n_rrr * n_blocks) return 0;
    const uint64_t t = gb / n_blocks;
    return wtab[dd_get(arena + rd[t].bt_begin, (gb - t * n_blocks) * 6, 6)];
}
// off: the scan of the widths over all blocks; the block's offset in its column's btnr = off[gb] - off[the column's first block]
MGX_HD uint64_t cd_rrr_block(const uint64_t *arena, const CdRrr *rd, const uint64_t *off, const uint8_t *wtab, const uint64_t *C, uint64_t gb,
                             uint64_t n_blocks, uint64_t *err) {
    const uint64_t t = gb / n_blocks, b = gb - t * n_blocks;
    const CdRrr d = rd[t];
    unsigned status;
    const uint64_t block = dd_rrr_unrank(arena + d.bt_begin, arena + d.btnr_begin, d.btnr_bits, off[gb] - off[t * n_blocks], wtab, C, b, &status);
    if (status) cd_fail(err, d.label, status == 1 ? CD_RRR_EARLY : CD_RRR_CLASS, b);
    return block;
}
// word w < W of rrr column t's bit map, g = t * W + w
MGX_HD void cd_rrr_pack(uint64_t *arena, const CdRrr *rd, const uint64_t *blocks, uint64_t g, uint64_t W, uint64_t n_blocks, uint64_t n_rows) {
    const uint64_t t = g / W, w = g - t * W;
    arena[rd[t].bm_begin + w] = dd_rrr_pack(blocks + t * n_blocks, n_blocks, n_rows, w);
}

// ---- sd columns: global word gw of the concatenated high parts; hprefix[s] = the first of column s, hprefix[n_sd] = all ---------
MGX_HD uint64_t cd_high_popcount(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, uint64_t gw) {
    if (gw >= hprefix[n_sd]) return 0;
    const uint32_t s = cd_find(hprefix, n_sd, gw);
    return dd_popcount_word(arena + sd[s].high_begin, gw - hprefix[s], sd[s].high_bits);
}
// The set bits p of the word, the i-th of their column: the position ((p - i) << wl) | low[i] after the checks of read_sd_vector.
// pass 0 (inverted columns only): the position's bit into the column's cleared bit map; pass 1 (the others): the position itself
// to rows[col_begin[label] + i].  hrank: the scan of cd_high_popcount.
// Order: p rises with i, so the upper parts p - i never fall, and two positions can be out of order only where the upper parts
// are equal, which is where bit p - 1 of high is set as well: then, and only then, low[i] must exceed low[i - 1].
// (cd_sd_each: the walk over one word's set bits with the checks, shared with the delimiter vectors of coord_decode.hpp, whose
// sizes differ per column; sink(i, v): the i-th position v of the column, false to stop)
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
MGX_HD void cd_sd_word(uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank, uint64_t gw,
                       uint64_t n_rows, int pass, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint32_t s = cd_find(hprefix, n_sd, gw);
    const CdSd d = sd[s];
    if ((d.inverted != 0) != (pass == 0)) return;
    cd_sd_each(arena, d, gw - hprefix[s], hrank[gw] - hrank[hprefix[s]], n_rows, err, [&](uint64_t i, uint64_t v) {
        if (pass == 0) cd_set_bit(arena + d.bm_begin + (v >> 6), (unsigned)(v & 63));
        else {
            const uint64_t o = col_begin[d.label] + i;
            if (o >= col_begin[d.label + 1]) { cd_fail(err, d.label, CD_OUT_RANGE, i); return false; }
            rows[o] = v;
        }
        return true;
    });
}

// ---- bit-map columns: word g = t * W + w of bit-map column t ----------------------------------------------------------------------
// the column's rows in [64 w, 64 w + 64): an inverted column's map complemented, nothing behind row n_rows - 1
// (*tail: a stat column has a bit set behind its last row)
MGX_HD uint64_t cd_bm_word(const uint64_t *arena, const CdBm *bm, uint64_t g, uint64_t W, uint64_t n_rows, bool *tail) {
    const uint64_t t = g / W, w = g - t * W;
    const CdBm d = bm[t];
    uint64_t x = arena[d.src_begin + w];
    if (d.kind == CD_KIND_SD_INVERTED) x = ~x;
    const uint64_t left = n_rows - w * 64;                                 // >= 1
    const uint64_t y = left >= 64 ? x : x & ((1ull << left) - 1);
    *tail = d.kind == CD_KIND_STAT && y != x;
    return y;
}
// cnt[g], g <= n_bm * W (the last: the zero that closes the scan)
MGX_HD uint64_t cd_bm_popcount(const uint64_t *arena, const CdBm *bm, uint64_t g, uint64_t n_bm, uint64_t W, uint64_t n_rows, uint64_t *err) {
    if (g >= n_bm * W) return 0;
    bool tail;
    const uint64_t x = cd_bm_word(arena, bm, g, W, n_rows, &tail);
    if (tail) cd_fail(err, bm[g / W].label, CD_STAT_TAIL, g % W);
    return (uint64_t)__builtin_popcountll(x);
}
// the set rows of label j, after the comparisons of the stored counts (stat: its count of ones; sd: ones against popcount(high))
MGX_HD uint64_t cd_count(const CdLabel *lab, const CdSd *sd, const CdBm *bm, const uint64_t *hprefix, const uint64_t *hrank, const uint64_t *bscan,
                         uint32_t j, uint64_t W, uint64_t n_rows, uint64_t *err) {
    const CdLabel l = lab[j];
    uint64_t n = 0;
    if (l.kind == CD_KIND_SD || l.kind == CD_KIND_SD_INVERTED) {
        const uint64_t m = hrank[hprefix[l.sd + 1]] - hrank[hprefix[l.sd]];
        if (m != sd[l.sd].ones) cd_fail(err, j, CD_SD_SELECT, m);
        n = m;
    }
    if (l.kind != CD_KIND_SD) {
        const uint64_t c = bscan[(l.bm + 1) * W] - bscan[l.bm * W];
        if (l.kind == CD_KIND_STAT && c != bm[l.bm].stat_ones) cd_fail(err, j, CD_STAT_ONES, c);
        if (l.kind == CD_KIND_SD_INVERTED && c != n_rows - n) cd_fail(err, j, CD_SD_ORDER, c);      // (a position stored twice)
        n = c;
    }
    return n;
}
// the write pass of a bit-map word: its set rows to rows[col_begin[label] + rank ..), ascending
MGX_HD void cd_bm_extract(const uint64_t *arena, const CdBm *bm, const uint64_t *bscan, uint64_t g, uint64_t W, uint64_t n_rows,
                          const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint64_t t = g / W, w = g - t * W;
    const uint32_t j = bm[t].label;
    bool tail;                                                              // (recorded by the count pass)
    uint64_t x = cd_bm_word(arena, bm, g, W, n_rows, &tail);
    uint64_t o = col_begin[j] + (bscan[g] - bscan[t * W]);
    const uint64_t end = col_begin[j + 1];
    for (unsigned k = 0; k < 64 && x; ++k, ++o, x &= x - 1) {
        if (o >= end) { cd_fail(err, j, CD_OUT_RANGE, w); return; }
        rows[o] = w * 64 + (uint64_t)__builtin_ctzll(x);
    }
}

} // namespace mgx
