// coord_decode.hpp — k-mer coordinates on the device, the kernel bodies of two steps:
//   * cq_*: the tuple section of `.column.annodbg.coords` / `.column_coord.annodbg` files (boss_files.hpp: read_tuples) decoded
//     into the coord_begin / coords arrays of mgx_annotation_set_coordinates, batched over all columns of a load;
//   * ct_*: mgx_annotation_set_coordinates_device, the transposition of those arrays into the row-major row_entry / coord_off /
//     coords of the device annotation.
// The kernels are in mgx_colload.hip and mgx_annot.hip; every body is an MGX_HD function over plain pointers, so that
// tests/emu/coord_decode_check.cpp compiles this very file for the host, with every array at the size the driver gives it.
//
// The delimiter vectors of a load are a second batch for the shared stage of bv_decode.hpp, after the binary columns: each has a
// length of its own (values + set rows + 1 bits), each gets a bit map (map j is column j's), and the maps are ranked by one scan.
// Here: what follows that stage — the conditions of read_tuples on every vector, the rank pass (the one of rank r, 0-based, at
// position p begins the tuple of the column's set row r at value p - r) and the unpacking of the values.  Rules as in
// bv_decode.hpp: indices from file content are compared with their array's length before use, no trip count depends on file
// content, a failed check records (column, check, position) and writes nothing out of range; the caller then asks the host reader.
#pragma once
#include "col_decode.hpp"

namespace mgx {

enum CqCheck : uint32_t {
    CQ_ONES = CD_CHECKS,     // delimiters: set bits != set rows + 1, or a stat vector's stored count differs from its bits
    CQ_FIRST,                // delimiters: first bit clear
    CQ_LAST,                 // delimiters: last bit clear
    CQ_VALUE,                // values: a coordinate of 2^63 or more
    CQ_CHECKS
};

// per column (= label), next to its delimiter vector's BvMap: sub: the vector's index among the sd vectors (sd kinds);
// val_begin / width: the values' words in the arena and their width (value i of the column is coords[vprefix[label] + i])
struct CqCol { uint64_t val_begin; uint32_t width, sub; };
static_assert(sizeof(CqCol) == 16, "CqCol");
// per column, after the scan: the conditions of read_tuples on a delimiter vector (its length against the values: the plan)
MGX_HD void cq_check(const uint64_t *arena, const BvMap *map, const CqCol *col, const CdSd *sd, const uint64_t *hprefix, const uint64_t *hrank,
                     const uint64_t *bmprefix, const uint64_t *bscan, const uint64_t *col_begin, uint32_t j, uint64_t *err) {
    const BvMap d = map[j];
    const uint64_t ones = bscan[bmprefix[j + 1]] - bscan[bmprefix[j]];
    if (d.kind == CD_KIND_SD || d.kind == CD_KIND_SD_INVERTED) {           // read_sd_vector: ones against popcount(high); a position twice
        const uint64_t s = col[j].sub, m = hrank[hprefix[s + 1]] - hrank[hprefix[s]];
        if (m != sd[s].ones) cd_fail(err, j, CD_SD_SELECT, m);
        if (ones != (d.kind == CD_KIND_SD ? m : d.bits - m)) cd_fail(err, j, CD_SD_ORDER, ones);
    }
    if (d.kind == CD_KIND_STAT && ones != d.stat_ones) cd_fail(err, j, CD_STAT_ONES, ones);
    if (ones != col_begin[j + 1] - col_begin[j] + 1) cd_fail(err, j, CQ_ONES, ones);
    if (!(bv_map_word(arena, d, 0) & 1)) cd_fail(err, j, CQ_FIRST, 0);
    if (!((bv_map_word(arena, d, (d.bits - 1) >> 6) >> ((d.bits - 1) & 63)) & 1)) cd_fail(err, j, CQ_LAST, d.bits - 1);
}
// the rank pass: the one of rank i of column j at position p begins the tuple of entry col_begin[j] + i at value vprefix[j] + p - i;
// the column's last one (i = its set rows) closes the last tuple: written by the last column only, as coord_begin[n_entries]
MGX_HD void cq_rank(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_cols, const uint64_t *bscan,
                    const uint64_t *col_begin, const uint64_t *vprefix, uint64_t g, uint64_t *coord_begin, uint64_t *err) {
    const uint32_t j = cd_find(bmprefix, n_cols, g);
    const uint64_t w = g - bmprefix[j], n_set = col_begin[j + 1] - col_begin[j];
    uint64_t x = bv_map_word(arena, map[j], w), i = bscan[g] - bscan[bmprefix[j]];
    for (unsigned t = 0; t < 64 && x; ++t, ++i, x &= x - 1) {
        if (i > n_set) { cd_fail(err, j, CD_OUT_RANGE, w); return; }
        const uint64_t p = w * 64 + (uint64_t)__builtin_ctzll(x);
        if (i < n_set || j + 1 == n_cols) coord_begin[col_begin[j] + i] = vprefix[j] + (p - i);
    }
}
// the unpack pass: value o of the load (o < vprefix[n_cols]) as an int64; widths 1 to 64, values that straddle a word (dd_get)
MGX_HD void cq_unpack(const uint64_t *arena, const CqCol *col, const uint64_t *vprefix, uint32_t n_cols, uint64_t o, int64_t *coords, uint64_t *err) {
    const uint32_t j = cd_find(vprefix, n_cols, o);
    const CqCol d = col[j];
    const uint64_t x = dd_get(arena + d.val_begin, (o - vprefix[j]) * d.width, d.width);
    if (x >> 63) { cd_fail(err, j, CQ_VALUE, o - vprefix[j]); coords[o] = 0; return; }
    coords[o] = (int64_t)x;
}

// ---- the transposition (mgx_annotation_set_coordinates_device) ------------------------------------------------------------------
// Entry x of the column-major input (row rows[x], label = the column whose range of col_begin holds x) -> the sort key of
// mgx_annotation_create_sparse, row << 24 | label; perm[x] = x rides along as the sort's value.
constexpr uint64_t CT_NO_ERROR = ~0ull;
enum CtCheck : uint64_t { CT_ROW = 0, CT_ORDER = 1 };        // the record: check << 62 | entry or coordinate, kept at its minimum:
                                                              // a row outside the matrix is reported before a descending tuple,
                                                              // as mgx_annotation_set_coordinates finds them
MGX_HD void ct_fail(uint64_t *err, uint64_t check, uint64_t at) {
    const uint64_t key = (check << 62) | (at & ((1ull << 62) - 1));
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(reinterpret_cast<unsigned long long *>(err), (unsigned long long)key);
#else
    if (key < *err) *err = key;
#endif
}
MGX_HD void ct_key(const uint64_t *col_begin, uint32_t n_labels, const uint64_t *rows, uint64_t n_rows, uint64_t x, uint64_t *keys, uint64_t *perm) {
    uint32_t lo = 0, hi = n_labels;                      // the last label with col_begin[label] <= x
    for (unsigned t = 0; t < 32; ++t) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (hi - lo > 1) { if (col_begin[mid] <= x) lo = mid; else hi = mid; }
    }
    keys[x] = rows[x] < n_rows ? (rows[x] << 24) | lo : 0;
    perm[x] = x;
}
// the largest e < n with prefix[e] <= x (prefix ascending, prefix[0] <= x < prefix[n]); 64 fixed steps
MGX_HD uint64_t ct_find(const uint64_t *prefix, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    for (unsigned t = 0; t < 64; ++t) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (hi - lo > 1) { if (prefix[mid] <= x) lo = mid; else hi = mid; }
    }
    return lo;
}
// item i < max(n_entries, n_coords): entry i's row inside the matrix; coordinate i not below its predecessor in the same tuple
// (looked up only where the values do fall: a tuple's first coordinate may be below the one before it)
MGX_HD void ct_check(const uint64_t *rows, uint64_t n_entries, uint64_t n_rows, const uint64_t *coord_begin, const int64_t *coords, uint64_t n_coords,
                     uint64_t i, uint64_t *err) {
    if (i < n_entries && rows[i] >= n_rows) ct_fail(err, CT_ROW, i);
    if (i && i < n_coords && coords[i] < coords[i - 1]) {
        // the last entry whose tuple begins at or before i (empty tuples share a begin: the last of them is the one that holds i)
        if (coord_begin[ct_find(coord_begin, n_entries, i)] != i) ct_fail(err, CT_ORDER, i);
    }
}
// sorted keys: the first entry of every row's run counts the run (rows without entries keep their zero)
MGX_HD void ct_row_count(const uint64_t *keys, uint64_t n_entries, uint64_t n_rows, uint64_t e, uint64_t *len) {
    const uint64_t row = keys[e] >> 24;
    if (row >= n_rows || (e && (keys[e - 1] >> 24) == row)) return;
    uint64_t end = e + 1;
    while (end < n_entries && (keys[end] >> 24) == row) ++end;      // (at most the labels of one row)
    len[row] = end - e;
}
// the tuple length of the entry that sorts to place e (tlen[n_entries]: the zero that closes the scan)
MGX_HD uint64_t ct_tuple_len(const uint64_t *perm, const uint64_t *coord_begin, uint64_t n_entries, uint64_t n_coords, uint64_t e) {
    if (e >= n_entries) return 0;
    const uint64_t x = perm[e];
    if (x >= n_entries) return 0;
    const uint64_t b = coord_begin[x], end = coord_begin[x + 1];
    return b <= end && end <= n_coords ? end - b : 0;
}
// coordinate o of the row-major array: one lane per coordinate, so a tuple of n coordinates is copied by n lanes
MGX_HD void ct_copy(const uint64_t *coord_off, const uint64_t *perm, const uint64_t *coord_begin, const int64_t *coords, uint64_t n_entries,
                    uint64_t n_coords, uint64_t o, int64_t *out) {
    const uint64_t e = ct_find(coord_off, n_entries, o);
    const uint64_t src = coord_begin[perm[e]] + (o - coord_off[e]);
    out[o] = src < n_coords ? coords[src] : 0;
}

} // namespace mgx
