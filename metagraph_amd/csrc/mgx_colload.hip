// mgx_colload.hip — `.column.annodbg` files decoded on the device: mgx_annotation_load_columns_device and the test hook
// mgx_column_file_decode_device (include/mgx.h, "files").  The host reads the files and walks their headers (col_plan.hpp); the
// payloads of ALL columns go into one arena with one copy, and the kernels below (bodies: col_decode.hpp) turn them into the
// columns' set rows in device memory, which mgx_annotation_create_sparse takes with on_device = 1.  DESIGN 3.17.
//
// Shapes: one lane per item of a concatenated buffer (an rrr block, a word of the sd high parts, a word of the bit maps); the
// number of launches and of device allocations depends on which of the four kinds of column occur (sd, inverted sd, stat, rrr),
// not on how many columns there are.  Two passes: counts per column (one copy of n_labels counts to the host, which forms
// col_begin), then every set row to rows[col_begin[j] + rank].  Scans: hipcub, 64-bit, on the null stream (the loader runs before
// any aligner exists).  The only atomics on data set the bits of an inverted column's stored positions in its cleared bit map.
//
// With coordinates (mgx_annotation_load_coord_columns_device): the tuple sections of the same load ride in the same
// arena (coord_plan.hpp: CoordBatch) and are decoded after the binary columns, whose counts the delimiter checks need, by the
// cq_* bodies of coord_decode.hpp into coord_begin / coords in device memory; mgx_annotation_set_coordinates_device takes them.
#include <memory>
#include <new>

#include "col_plan.hpp"
#include "coord_plan.hpp"
#include "column_file.hpp"
#include "dbg_kernels.hpp"

// =================================================================================================
// kernels (the shared ones: dbg_kernels.hpp)
// =================================================================================================
namespace {

__global__ void __launch_bounds__(256) k_col_rrr_width(const uint64_t *arena, const CdRrr *rd, const uint8_t *wtab, uint64_t *width, uint64_t n_blocks,
                                                       uint64_t n_rrr) {
    const uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb <= n_rrr * n_blocks) width[gb] = cd_rrr_width(arena, rd, wtab, gb, n_blocks, n_rrr);
}

__global__ void __launch_bounds__(256) k_col_rrr_block(const uint64_t *arena, const CdRrr *rd, const uint64_t *off, const uint8_t *wtab,
                                                       const uint64_t *binom, uint64_t *blocks, uint64_t n_blocks, uint64_t total, uint64_t *err) {
    __shared__ uint64_t C[DD_BINOM_ENTRIES];
    __shared__ uint8_t wt[64];
    for (uint32_t x = threadIdx.x; x < DD_BINOM_ENTRIES; x += blockDim.x) C[x] = binom[x];
    if (threadIdx.x < 64) wt[threadIdx.x] = wtab[threadIdx.x];
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; gb < total; gb += step)
        blocks[gb] = cd_rrr_block(arena, rd, off, wt, C, gb, n_blocks, err);
}

__global__ void __launch_bounds__(256) k_col_rrr_pack(uint64_t *arena, const CdRrr *rd, const uint64_t *blocks, uint64_t W, uint64_t n_blocks,
                                                      uint64_t n_rows, uint64_t total) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cd_rrr_pack(arena, rd, blocks, g, W, n_blocks, n_rows);
}

__global__ void __launch_bounds__(256) k_col_high_popcount(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, uint64_t *cnt,
                                                           uint64_t n_words) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw <= n_words) cnt[gw] = cd_high_popcount(arena, sd, hprefix, n_sd, gw);
}

__global__ void __launch_bounds__(256) k_col_sd_word(uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank,
                                                     uint64_t n_words, uint64_t n_rows, int pass, const uint64_t *col_begin, uint64_t *rows,
                                                     uint64_t *err) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw < n_words) cd_sd_word(arena, sd, hprefix, n_sd, hrank, gw, n_rows, pass, col_begin, rows, err);
}

__global__ void __launch_bounds__(256) k_col_bm_popcount(const uint64_t *arena, const CdBm *bm, uint64_t *cnt, uint64_t n_bm, uint64_t W,
                                                         uint64_t n_rows, uint64_t *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= n_bm * W) cnt[g] = cd_bm_popcount(arena, bm, g, n_bm, W, n_rows, err);
}

__global__ void __launch_bounds__(256) k_col_counts(const CdLabel *lab, const CdSd *sd, const CdBm *bm, const uint64_t *hprefix, const uint64_t *hrank,
                                                    const uint64_t *bscan, uint32_t n_labels, uint64_t W, uint64_t n_rows, uint64_t *counts,
                                                    uint64_t *err) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_labels) counts[j] = cd_count(lab, sd, bm, hprefix, hrank, bscan, j, W, n_rows, err);
}

__global__ void __launch_bounds__(256) k_col_bm_extract(const uint64_t *arena, const CdBm *bm, const uint64_t *bscan, uint64_t total, uint64_t W,
                                                        uint64_t n_rows, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cd_bm_extract(arena, bm, bscan, g, W, n_rows, col_begin, rows, err);
}

// ---- coordinates: the delimiter vectors and the values (bodies: coord_decode.hpp) ----
__global__ void __launch_bounds__(256) k_cq_rrr_width(const uint64_t *arena, const CqRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, const uint8_t *wtab,
                                                      uint64_t *width, uint64_t total) {
    const uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb <= total) width[gb] = cq_rrr_width(arena, rd, rbprefix, n_rrr, wtab, gb);
}
__global__ void __launch_bounds__(256) k_cq_rrr_block(const uint64_t *arena, const CqRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, const uint64_t *off,
                                                      const uint8_t *wtab, const uint64_t *binom, uint64_t *blocks, uint64_t total, uint64_t *err) {
    __shared__ uint64_t C[DD_BINOM_ENTRIES];
    __shared__ uint8_t wt[64];
    for (uint32_t x = threadIdx.x; x < DD_BINOM_ENTRIES; x += blockDim.x) C[x] = binom[x];
    if (threadIdx.x < 64) wt[threadIdx.x] = wtab[threadIdx.x];
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; gb < total; gb += step)
        blocks[gb] = cq_rrr_block(arena, rd, rbprefix, n_rrr, off, wt, C, gb, err);
}
__global__ void __launch_bounds__(256) k_cq_rrr_pack(uint64_t *arena, const CqCol *col, const uint64_t *bmprefix, uint32_t n_cols, const uint64_t *rbprefix,
                                                     const uint64_t *blocks, uint64_t total) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cq_rrr_pack(arena, col, bmprefix, n_cols, rbprefix, blocks, g);
}
__global__ void __launch_bounds__(256) k_cq_sd_word(uint64_t *arena, const CdSd *sd, const CqCol *col, const uint64_t *hprefix, uint32_t n_sd,
                                                    const uint64_t *hrank, uint64_t n_words, uint64_t *err) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw < n_words) cq_sd_word(arena, sd, col, hprefix, n_sd, hrank, gw, err);
}
__global__ void __launch_bounds__(256) k_cq_bm_popcount(const uint64_t *arena, const CqCol *col, const uint64_t *bmprefix, uint32_t n_cols, uint64_t *cnt,
                                                        uint64_t total) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= total) cnt[g] = cq_bm_popcount(arena, col, bmprefix, n_cols, g);
}
__global__ void __launch_bounds__(256) k_cq_check(const uint64_t *arena, const CqCol *col, const CdSd *sd, const uint64_t *hprefix, const uint64_t *hrank,
                                                  const uint64_t *bmprefix, const uint64_t *bscan, const uint64_t *col_begin, uint32_t n_cols, uint64_t *err) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cols) cq_check(arena, col, sd, hprefix, hrank, bmprefix, bscan, col_begin, j, err);
}
__global__ void __launch_bounds__(256) k_cq_rank(const uint64_t *arena, const CqCol *col, const uint64_t *bmprefix, uint32_t n_cols, const uint64_t *bscan,
                                                 const uint64_t *col_begin, const uint64_t *vprefix, uint64_t total, uint64_t *coord_begin, uint64_t *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cq_rank(arena, col, bmprefix, n_cols, bscan, col_begin, vprefix, g, coord_begin, err);
}
__global__ void __launch_bounds__(256) k_cq_unpack(const uint64_t *arena, const CqCol *col, const uint64_t *vprefix, uint32_t n_cols, uint64_t total,
                                                   int64_t *coords, uint64_t *err) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o < total) cq_unpack(arena, col, vprefix, n_cols, o, coords, err);
}

// =================================================================================================
// host
// =================================================================================================
template <class T>
int upload_table(DBuf &d, const std::vector<T> &v) {
    TRY_D(d.alloc(v.size() * sizeof(T)));
    return h2d(d.p, v.data(), v.size() * sizeof(T));
}

struct Loaded {
    ColBatch b;
    std::vector<uint64_t> col_begin;     // host; n_labels + 1
    DBuf rows;                           // col_begin.back() row indices on `device`
    bool host_only = false;              // nothing to decode (no rows or no labels, or more labels than a device matrix takes)
    // with coordinates: coord_begin (col_begin.back() + 1 entries) and coords (n_coords) on `device`
    CoordBatch cq;
    DBuf coord_begin, coords;
    uint64_t n_coords = 0;
};


// What the host reader says about these files when the plan or the device found fault with them: its code and message.  Never
// success: a file the host reader accepts and the device path does not is an internal error.
int host_answer(const char *const *paths, uint32_t n_paths, const char *why, bool coords = false) {
    mgx_column_file *cf = nullptr;
    const int rc = coords ? mgx_column_coord_file_read(paths, n_paths, &cf) : mgx_column_file_read(paths, n_paths, &cf);
    if (rc != MGX_OK) return rc;
    mgx_column_file_free(cf);
    return dfail(MGX_ERR_INVALID, "%s: internal error: the device decode refuses (%s) a file that the host reader accepts", paths[0], why);
}

const char *cd_check_name(uint32_t check) {
    static const char *const text[] = { "", "rrr block numbers end early", "rrr block number outside its class", "stat count of ones", "stat bits behind the end",
                                        "sd select supports", "sd shift", "sd positions not ascending below size", "output index",
                                        "delimiters: number of set bits", "delimiters: first bit", "delimiters: last bit", "values: 2^63 or more" };
    return check < sizeof(text) / sizeof(text[0]) ? text[check] : "unknown check";
}

// the files' columns as col_begin (host) and rows (device); coords: and their tuple sections (the side files of form (a), or one
// file of form (b)) as coord_begin and coords (device).  MGX_OK with out->host_only: the caller takes the host reader's table
int decode_files(const char *const *paths, uint32_t n_paths, int device, Loaded *out, bool coords = false) {
    std::vector<std::vector<uint8_t>> images(n_paths), sides(coords ? n_paths : 0);
    std::vector<ColumnsPlan> plans(n_paths);
    std::vector<std::vector<TuplePlan>> tuples(coords ? n_paths : 0);
    ColBatch &b = out->b;
    CoordBatch &cq = out->cq;
    try {
        for (uint32_t i = 0; i < n_paths; ++i) {
            if (coords && is_column_coord_path(paths[i])) {
                if (n_paths > 1) throw NeedsHost("a .column_coord.annodbg file next to others");
                images[i] = read_whole_file(paths[i]);
                plans[i] = plan_column_coord(images[i].data(), images[i].size(), tuples[i]);
                continue;
            }
            images[i] = read_whole_file(paths[i]);
            plans[i] = plan_columns(images[i].data(), images[i].size());
            if (coords) {
                sides[i] = read_whole_file(coord_side_path(paths[i]));
                Cursor c(sides[i].data(), sides[i].size());
                tuples[i] = plan_tuples(c, sides[i].data(), plans[i].labels.size(), plans[i].n_rows);
            }
        }
        check_merge(plans);
        uint64_t n_labels = 0;
        for (const ColumnsPlan &p : plans) n_labels += p.labels.size();
        if (!plans[0].n_rows || !n_labels || n_labels >= (1u << 24)) { out->host_only = true; return MGX_OK; }
        std::vector<const TuplePlan *> tp;
        for (const std::vector<TuplePlan> &v : tuples) for (const TuplePlan &t : v) tp.push_back(&t);
        if (coords) cq.layout(tp);
        b.build(plans, cq.upload_words);
        if (coords) cq.place(tp, b.extra_begin, b.arena_words, b.stage.data());
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "%s: out of host memory", paths[0]);
    } catch (const std::runtime_error &e) {                      // ParseError, Unsupported, NeedsHost
        return host_answer(paths, n_paths, e.what(), coords);
    }
    images.clear();                                              // (the payloads are in b.stage)
    sides.clear();
    if (mgx_device_count() <= device || device < 0) return dfail(MGX_ERR_NO_DEVICE, "HIP device %d not available", device);
    HIP_TRY_D(hipSetDevice(device));
    const uint32_t n_labels = (uint32_t)b.lab.size(), n_sd = (uint32_t)b.sd.size();
    const uint64_t HW = b.high_words(), BW = b.bm_words(), RB = b.rrr_blocks();

    DBuf err, arena, t_rrr, t_sd, t_bm, t_lab, t_hprefix, hrank, bscan, counts, d_cb;
    Tables tables;
    TRY_D(err.alloc(8));
    HIP_TRY_D(hipMemset(err.p, 0xFF, 8));
    uint64_t *e = err.as<uint64_t>();
    const uint64_t arena_words = b.arena_words + cq.tail_words;  // (the delimiter vectors' bit maps behind the columns')
    TRY_D(arena.alloc(arena_words * 8));
    TRY_D(h2d(arena.p, b.stage.data(), b.upload_words * 8));
    if (arena_words > b.upload_words) HIP_TRY_D(hipMemset(arena.as<uint64_t>() + b.upload_words, 0, (arena_words - b.upload_words) * 8));
    std::vector<uint64_t>().swap(b.stage);
    uint64_t *A = arena.as<uint64_t>();
    TRY_D(upload_table(t_rrr, b.rrr));
    TRY_D(upload_table(t_sd, b.sd));
    TRY_D(upload_table(t_bm, b.bm));
    TRY_D(upload_table(t_lab, b.lab));
    TRY_D(upload_table(t_hprefix, b.hprefix));
    TRY_D(hrank.alloc((HW + 1) * 8));
    TRY_D(bscan.alloc((BW + 1) * 8));
    TRY_D(counts.alloc((uint64_t)n_labels * 8));

    if (RB) {                                                    // rrr columns: widths, one scan over all blocks, un-rank, pack
        DBuf off, blocks;
        TRY_D(upload_tables(tables));
        TRY_D(off.alloc((RB + 1) * 8));
        TRY_D(blocks.alloc(RB * 8));
        k_col_rrr_width<<<grid_for(RB + 1), 256>>>(A, t_rrr.as<CdRrr>(), tables.wtab.as<uint8_t>(), off.as<uint64_t>(), b.n_blocks, b.rrr.size());
        LAUNCHED(0);
        TRY_D(scan_in_place(off.as<uint64_t>(), RB + 1));
        k_col_rrr_block<<<grid_for(RB, 2048), 256>>>(A, t_rrr.as<CdRrr>(), off.as<uint64_t>(), tables.wtab.as<uint8_t>(), tables.binom.as<uint64_t>(),
                                                      blocks.as<uint64_t>(), b.n_blocks, RB, e);
        LAUNCHED(0);
        const uint64_t words = (uint64_t)b.rrr.size() * b.W;
        k_col_rrr_pack<<<grid_for(words), 256>>>(A, t_rrr.as<CdRrr>(), blocks.as<uint64_t>(), b.W, b.n_blocks, b.n_rows, words);
        LAUNCHED(0);
    }
    if (n_sd) {                                                  // sd columns: the rank of every word of the high parts
        k_col_high_popcount<<<grid_for(HW + 1), 256>>>(A, t_sd.as<CdSd>(), t_hprefix.as<uint64_t>(), n_sd, hrank.as<uint64_t>(), HW);
        LAUNCHED(1);
        TRY_D(scan_in_place(hrank.as<uint64_t>(), HW + 1));
        if (b.kinds[CD_KIND_SD_INVERTED] && HW) {                // ... and the stored positions of the inverted ones into their bit maps
            k_col_sd_word<<<grid_for(HW), 256>>>(A, t_sd.as<CdSd>(), t_hprefix.as<uint64_t>(), n_sd, hrank.as<uint64_t>(), HW, b.n_rows, 0, nullptr, nullptr, e);
            LAUNCHED(1);
        }
    }
    if (BW) {                                                    // bit-map columns: the rank of every word
        k_col_bm_popcount<<<grid_for(BW + 1), 256>>>(A, t_bm.as<CdBm>(), bscan.as<uint64_t>(), b.bm.size(), b.W, b.n_rows, e);
        LAUNCHED(1);
        TRY_D(scan_in_place(bscan.as<uint64_t>(), BW + 1));
    }
    k_col_counts<<<grid_for(n_labels), 256>>>(t_lab.as<CdLabel>(), t_sd.as<CdSd>(), t_bm.as<CdBm>(), t_hprefix.as<uint64_t>(), hrank.as<uint64_t>(),
                                              bscan.as<uint64_t>(), n_labels, b.W, b.n_rows, counts.as<uint64_t>(), e);
    LAUNCHED(1);
    std::vector<uint64_t> n_set(n_labels);
    TRY_D(d2h(n_set.data(), counts.p, (uint64_t)n_labels * 8));  // (synchronises with the kernels)
    uint64_t key = DD_NO_ERROR;
    TRY_D(d2h(&key, e, 8));
    if (key == DD_NO_ERROR && !b.col_begin_from(n_set, out->col_begin)) return host_answer(paths, n_paths, "more than 2^33 expanded rows", coords);
    if (key == DD_NO_ERROR && coords && !cq.lengths_fit(out->col_begin)) return host_answer(paths, n_paths, "delimiters: length", coords);
    if (key == DD_NO_ERROR) {                                    // the write pass
        const uint64_t total = out->col_begin.back();
        TRY_D(upload_table(d_cb, out->col_begin));
        TRY_D(out->rows.alloc(total * 8));
        if (b.kinds[CD_KIND_SD] && HW) {
            k_col_sd_word<<<grid_for(HW), 256>>>(A, t_sd.as<CdSd>(), t_hprefix.as<uint64_t>(), n_sd, hrank.as<uint64_t>(), HW, b.n_rows, 1,
                                                 d_cb.as<uint64_t>(), out->rows.as<uint64_t>(), e);
            LAUNCHED(1);
        }
        if (BW) {
            k_col_bm_extract<<<grid_for(BW), 256>>>(A, t_bm.as<CdBm>(), bscan.as<uint64_t>(), BW, b.W, b.n_rows, d_cb.as<uint64_t>(),
                                                    out->rows.as<uint64_t>(), e);
            LAUNCHED(1);
        }
        if (coords) {                                            // the tuple sections: delimiters to bit maps, rank pass, unpack pass
            const uint32_t n_cols = (uint32_t)cq.col.size(), cq_sd = (uint32_t)cq.sd.size(), cq_rrr = (uint32_t)cq.rrr.size();
            const uint64_t CH = cq.high_words(), CB = cq.bm_words(), CR = cq.rrr_blocks(), NV = cq.n_values();
            DBuf q_col, q_rrr, q_sd, q_hprefix, q_rbprefix, q_bmprefix, q_vprefix, q_hrank, q_bscan;
            TRY_D(upload_table(q_col, cq.col));
            TRY_D(upload_table(q_rrr, cq.rrr));
            TRY_D(upload_table(q_sd, cq.sd));
            TRY_D(upload_table(q_hprefix, cq.hprefix));
            TRY_D(upload_table(q_rbprefix, cq.rbprefix));
            TRY_D(upload_table(q_bmprefix, cq.bmprefix));
            TRY_D(upload_table(q_vprefix, cq.vprefix));
            TRY_D(q_hrank.alloc((CH + 1) * 8));
            TRY_D(q_bscan.alloc((CB + 1) * 8));
            if (CR) {
                DBuf off, blocks;
                if (!tables.wtab.p) TRY_D(upload_tables(tables));
                TRY_D(off.alloc((CR + 1) * 8));
                TRY_D(blocks.alloc(CR * 8));
                k_cq_rrr_width<<<grid_for(CR + 1), 256>>>(A, q_rrr.as<CqRrr>(), q_rbprefix.as<uint64_t>(), cq_rrr, tables.wtab.as<uint8_t>(), off.as<uint64_t>(), CR);
                LAUNCHED(0);
                TRY_D(scan_in_place(off.as<uint64_t>(), CR + 1));
                k_cq_rrr_block<<<grid_for(CR, 2048), 256>>>(A, q_rrr.as<CqRrr>(), q_rbprefix.as<uint64_t>(), cq_rrr, off.as<uint64_t>(), tables.wtab.as<uint8_t>(),
                                                             tables.binom.as<uint64_t>(), blocks.as<uint64_t>(), CR, e);
                LAUNCHED(0);
                k_cq_rrr_pack<<<grid_for(CB), 256>>>(A, q_col.as<CqCol>(), q_bmprefix.as<uint64_t>(), n_cols, q_rbprefix.as<uint64_t>(), blocks.as<uint64_t>(), CB);
                LAUNCHED(0);
            }
            if (cq_sd) {
                k_col_high_popcount<<<grid_for(CH + 1), 256>>>(A, q_sd.as<CdSd>(), q_hprefix.as<uint64_t>(), cq_sd, q_hrank.as<uint64_t>(), CH);
                LAUNCHED(1);
                TRY_D(scan_in_place(q_hrank.as<uint64_t>(), CH + 1));
                if (CH) {
                    k_cq_sd_word<<<grid_for(CH), 256>>>(A, q_sd.as<CdSd>(), q_col.as<CqCol>(), q_hprefix.as<uint64_t>(), cq_sd, q_hrank.as<uint64_t>(), CH, e);
                    LAUNCHED(1);
                }
            }
            k_cq_bm_popcount<<<grid_for(CB + 1), 256>>>(A, q_col.as<CqCol>(), q_bmprefix.as<uint64_t>(), n_cols, q_bscan.as<uint64_t>(), CB);
            LAUNCHED(1);
            TRY_D(scan_in_place(q_bscan.as<uint64_t>(), CB + 1));
            k_cq_check<<<grid_for(n_cols), 256>>>(A, q_col.as<CqCol>(), q_sd.as<CdSd>(), q_hprefix.as<uint64_t>(), q_hrank.as<uint64_t>(), q_bmprefix.as<uint64_t>(),
                                                  q_bscan.as<uint64_t>(), d_cb.as<uint64_t>(), n_cols, e);
            LAUNCHED(1);
            TRY_D(out->coord_begin.alloc((total + 1) * 8));
            TRY_D(out->coords.alloc(NV * 8));
            out->n_coords = NV;
            k_cq_rank<<<grid_for(CB), 256>>>(A, q_col.as<CqCol>(), q_bmprefix.as<uint64_t>(), n_cols, q_bscan.as<uint64_t>(), d_cb.as<uint64_t>(),
                                             q_vprefix.as<uint64_t>(), CB, out->coord_begin.as<uint64_t>(), e);
            LAUNCHED(1);
            if (NV) {
                k_cq_unpack<<<grid_for(NV), 256>>>(A, q_col.as<CqCol>(), q_vprefix.as<uint64_t>(), n_cols, NV, out->coords.as<int64_t>(), e);
                LAUNCHED(1);
            }
        }
        TRY_D(d2h(&key, e, 8));
    }
    if (key != DD_NO_ERROR) {
        char why[128];
        snprintf(why, sizeof(why), "column %u: %s at %u", (unsigned)(key >> 40), cd_check_name((uint32_t)(key >> 32) & 0xFF), (unsigned)(key & 0xFFFFFFFFu));
        return host_answer(paths, n_paths, why, coords);
    }
    return MGX_OK;
}

int bad_paths(const char *who, const char *const *paths, uint32_t n_paths) {
    for (uint32_t i = 0; i < n_paths; ++i) if (!paths[i]) return dfail(MGX_ERR_INVALID, "%s: path %u is null", who, i);
    return MGX_OK;
}

}  // namespace

extern "C" {

void mgx_column_decode_kernel_launch_counts(uint64_t *out4) {
    out4[0] = g_counts[0].load() + g_counts[1].load();
    out4[1] = g_allocs.load();
    out4[2] = g_counts[2].load();
    out4[3] = g_counts[3].load();
}

int mgx_column_file_decode_device(const char *const *paths, uint32_t n_paths, int device, mgx_column_file **out) {
    if (!paths || !n_paths || !out) return dfail(MGX_ERR_INVALID, "mgx_column_file_decode_device: bad arguments");
    *out = nullptr;
    TRY_D(bad_paths("mgx_column_file_decode_device", paths, n_paths));
    Loaded l;
    TRY_D(decode_files(paths, n_paths, device, &l));
    if (l.host_only) return mgx_column_file_read(paths, n_paths, out);
    std::unique_ptr<mgx_column_file> m(new (std::nothrow) mgx_column_file());
    if (!m) return dfail(MGX_ERR_OOM, "mgx_column_file_decode_device: out of host memory");
    try {
        m->f.n_rows = l.b.n_rows;
        m->f.labels = l.b.labels;
        m->f.col_begin = l.col_begin;
        m->f.rows.resize(l.col_begin.back());
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "mgx_column_file_decode_device: out of host memory");
    }
    TRY_D(d2h(m->f.rows.data(), l.rows.p, m->f.rows.size() * 8));
    *out = m.release();
    return MGX_OK;
}

int mgx_column_coord_file_decode_device(const char *const *paths, uint32_t n_paths, int device, mgx_column_file **out) {
    if (!paths || !n_paths || !out) return dfail(MGX_ERR_INVALID, "mgx_column_coord_file_decode_device: bad arguments");
    *out = nullptr;
    TRY_D(bad_paths("mgx_column_coord_file_decode_device", paths, n_paths));
    Loaded l;
    TRY_D(decode_files(paths, n_paths, device, &l, true));
    if (l.host_only) return mgx_column_coord_file_read(paths, n_paths, out);
    std::unique_ptr<mgx_column_file> m(new (std::nothrow) mgx_column_file());
    if (!m) return dfail(MGX_ERR_OOM, "mgx_column_coord_file_decode_device: out of host memory");
    try {
        m->f.n_rows = l.b.n_rows;
        m->f.labels = l.b.labels;
        m->f.col_begin = l.col_begin;
        m->f.rows.resize(l.col_begin.back());
        m->f.coord_begin.resize(l.col_begin.back() + 1);
        m->f.coords.resize(l.n_coords);
        m->f.has_coords = true;
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "mgx_column_coord_file_decode_device: out of host memory");
    }
    TRY_D(d2h(m->f.rows.data(), l.rows.p, m->f.rows.size() * 8));
    TRY_D(d2h(m->f.coord_begin.data(), l.coord_begin.p, m->f.coord_begin.size() * 8));
    TRY_D(d2h(m->f.coords.data(), l.coords.p, m->f.coords.size() * 8));
    // a descending tuple is what the transposition's kernel finds in a load; the hook has no transposition: the host reader's word
    for (uint64_t x = 0; x + 1 < m->f.coord_begin.size(); ++x)
        for (uint64_t t = m->f.coord_begin[x] + 1; t < m->f.coord_begin[x + 1]; ++t)
            if (m->f.coords[t] < m->f.coords[t - 1]) return host_answer(paths, n_paths, "a tuple is not ascending", true);
    *out = m.release();
    return MGX_OK;
}

int mgx_annotation_load_coord_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out) {
    if (!paths || !n_paths || !out) return dfail(MGX_ERR_INVALID, "mgx_annotation_load_coord_columns_device: bad arguments");
    *out = nullptr;
    if (names_out) *names_out = nullptr;
    TRY_D(bad_paths("mgx_annotation_load_coord_columns_device", paths, n_paths));
    Loaded l;
    TRY_D(decode_files(paths, n_paths, device, &l, true));
    std::unique_ptr<mgx_column_file> m;
    if (l.host_only) {                                           // an empty matrix: the host reader's tables
        mgx_column_file *cf = nullptr;
        TRY_D(mgx_column_coord_file_read(paths, n_paths, &cf));
        m.reset(cf);
        TRY_D(mgx_annotation_create_from_file(cf, device, out));
        m->f.rows.clear(); m->f.coord_begin.clear(); m->f.coords.clear();
        m->f.has_coords = false;
    } else {
        m.reset(new (std::nothrow) mgx_column_file());
        if (!m) return dfail(MGX_ERR_OOM, "mgx_annotation_load_coord_columns_device: out of host memory");
        m->f.n_rows = l.b.n_rows;
        m->f.labels = l.b.labels;
        m->f.col_begin = l.col_begin;
        const uint32_t n_labels = (uint32_t)l.b.lab.size();
        TRY_D(mgx_annotation_create_sparse(l.b.n_rows, n_labels, l.col_begin.data(), l.rows.as<uint64_t>(), 1, device, out));
        const int rc = mgx_annotation_set_coordinates_device(*out, n_labels, l.col_begin.data(), l.rows.as<uint64_t>(), l.coord_begin.as<uint64_t>(),
                                                             l.coords.as<int64_t>());
        if (rc != MGX_OK) {
            mgx_annotation_destroy(*out);
            *out = nullptr;
            // (a descending tuple: the host reader names it; any other failure keeps its own code and message)
            return rc == MGX_ERR_INVALID ? host_answer(paths, n_paths, "a tuple is not ascending", true) : rc;
        }
    }
    m->rows_on_device = true;
    if (names_out) *names_out = m.release();
    return MGX_OK;
}

int mgx_annotation_load_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out) {
    if (!paths || !n_paths || !out) return dfail(MGX_ERR_INVALID, "mgx_annotation_load_columns_device: bad arguments");
    *out = nullptr;
    if (names_out) *names_out = nullptr;
    TRY_D(bad_paths("mgx_annotation_load_columns_device", paths, n_paths));
    Loaded l;
    TRY_D(decode_files(paths, n_paths, device, &l));
    std::unique_ptr<mgx_column_file> m;
    if (l.host_only) {                                           // an empty matrix: the host reader's table, nothing for a kernel to do
        mgx_column_file *cf = nullptr;
        TRY_D(mgx_column_file_read(paths, n_paths, &cf));
        m.reset(cf);
        TRY_D(mgx_annotation_create_from_file(cf, device, out));
        m->f.rows.clear();
    } else {
        m.reset(new (std::nothrow) mgx_column_file());
        if (!m) return dfail(MGX_ERR_OOM, "mgx_annotation_load_columns_device: out of host memory");
        m->f.n_rows = l.b.n_rows;
        m->f.labels = l.b.labels;
        m->f.col_begin = l.col_begin;
        TRY_D(mgx_annotation_create_sparse(l.b.n_rows, (uint32_t)l.b.lab.size(), l.col_begin.data(), l.rows.as<uint64_t>(), 1, device, out));
    }
    m->rows_on_device = true;
    if (names_out) *names_out = m.release();
    return MGX_OK;
}

}  // extern "C"
