// col_decode.hpp — the columns of `.column.annodbg` files (boss_files.hpp: parse_columns) decoded into the set rows that
// mgx_annotation_create_sparse takes, batched over ALL columns of a load.  The columns are one batch of bit vectors of n_rows bits
// each (the plan refuses a file in which one has another length), decoded into bit maps and ranked by the shared stage of
// bv_decode.hpp; a plain sd column has no map there, its stored positions are its rows.  Here: what the columns do on top of that
// stage — the per-label counts, and the write pass of every set row to rows[col_begin[label] + rank].  The kernels are in
// mgx_colload.hip, the layout of the buffers and tables in col_plan.hpp (ColBatch); bodies, checks and the error record follow
// the rules of bv_decode.hpp, and tests/emu/col_decode_check.cpp compiles this very file for the host.  DESIGN 3.17.
#pragma once
#include "bv_decode.hpp"

namespace mgx {

// per label: CD_KIND_*, its index among the sd vectors (sd kinds) and among the bit maps (all but plain sd)
struct CdLabel { uint32_t kind, sd, bm, pad; };
static_assert(sizeof(CdLabel) == 16, "CdLabel");

// the set rows of label j, after the comparisons of the stored counts (stat: its count of ones, no bit behind its last row; sd:
// ones against popcount(high)).  hrank, bscan: the scans of the shared stage
MGX_HD uint64_t cd_count(const uint64_t *arena, const CdLabel *lab, const CdSd *sd, const BvMap *map, const uint64_t *hprefix, const uint64_t *hrank,
                         const uint64_t *bmprefix, const uint64_t *bscan, uint32_t j, uint64_t n_rows, uint64_t *err) {
    const CdLabel l = lab[j];
    uint64_t n = 0;
    if (l.kind == CD_KIND_SD || l.kind == CD_KIND_SD_INVERTED) {
        const uint64_t m = hrank[hprefix[l.sd + 1]] - hrank[hprefix[l.sd]];
        if (m != sd[l.sd].ones) cd_fail(err, j, CD_SD_SELECT, m);
        n = m;
    }
    if (l.kind != CD_KIND_SD) {
        const uint64_t c = bscan[bmprefix[l.bm + 1]] - bscan[bmprefix[l.bm]];
        const uint64_t last = (n_rows - 1) >> 6;
        if (l.kind == CD_KIND_STAT && c != map[l.bm].stat_ones) cd_fail(err, j, CD_STAT_ONES, c);
        if (l.kind == CD_KIND_STAT && arena[map[l.bm].src_begin + last] != bv_map_word(arena, map[l.bm], last)) cd_fail(err, j, CD_STAT_TAIL, last);
        if (l.kind == CD_KIND_SD_INVERTED && c != n_rows - n) cd_fail(err, j, CD_SD_ORDER, c);      // (a position stored twice)
        n = c;
    }
    return n;
}
// the write pass of a word of the high parts: the positions of a plain sd column to rows[col_begin[label] + i]
MGX_HD void cd_sd_rows(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank, uint64_t gw,
                       uint64_t n_rows, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint32_t s = cd_find(hprefix, n_sd, gw);
    const CdSd d = sd[s];
    if (d.map != BV_NO_MAP) return;
    cd_sd_each(arena, d, gw - hprefix[s], hrank[gw] - hrank[hprefix[s]], n_rows, err, [&](uint64_t i, uint64_t v) {
        const uint64_t o = col_begin[d.label] + i;
        if (o >= col_begin[d.label + 1]) { cd_fail(err, d.label, CD_OUT_RANGE, i); return false; }
        rows[o] = v;
        return true;
    });
}
// the write pass of a bit-map word: its set rows to rows[col_begin[label] + rank ..), ascending
MGX_HD void cd_bm_extract(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_map, uint64_t bm_stride, const uint64_t *bscan,
                          uint64_t g, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint32_t t = bv_find(bmprefix, n_map, bm_stride, g);
    const uint64_t w = g - bmprefix[t];
    const uint32_t j = map[t].label;
    uint64_t x = bv_map_word(arena, map[t], w);
    uint64_t o = col_begin[j] + (bscan[g] - bscan[bmprefix[t]]);
    const uint64_t end = col_begin[j + 1];
    for (unsigned k = 0; k < 64 && x; ++k, ++o, x &= x - 1) {
        if (o >= end) { cd_fail(err, j, CD_OUT_RANGE, w); return; }
        rows[o] = w * 64 + (uint64_t)__builtin_ctzll(x);
    }
}

} // namespace mgx
