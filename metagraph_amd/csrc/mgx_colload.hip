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
#include <memory>
#include <new>

#include "col_plan.hpp"
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
};

// What the host reader says about these files when the plan or the device found fault with them: its code and message.  Never
// success: a file the host reader accepts and the device path does not is an internal error.
int host_answer(const char *const *paths, uint32_t n_paths, const char *why) {
    mgx_column_file *cf = nullptr;
    const int rc = mgx_column_file_read(paths, n_paths, &cf);
    if (rc != MGX_OK) return rc;
    mgx_column_file_free(cf);
    return dfail(MGX_ERR_INVALID, "%s: internal error: the device decode refuses (%s) a file that the host reader accepts", paths[0], why);
}

const char *cd_check_name(uint32_t check) {
    static const char *const text[] = { "", "rrr block numbers end early", "rrr block number outside its class", "stat count of ones", "stat bits behind the end",
                                        "sd select supports", "sd shift", "sd positions not ascending below size", "output index" };
    return check < sizeof(text) / sizeof(text[0]) ? text[check] : "unknown check";
}

// the files' columns as col_begin (host) and rows (device).  MGX_OK with out->host_only: the caller takes the host reader's table
int decode_files(const char *const *paths, uint32_t n_paths, int device, Loaded *out) {
    std::vector<std::vector<uint8_t>> images(n_paths);
    std::vector<ColumnsPlan> plans(n_paths);
    ColBatch &b = out->b;
    try {
        for (uint32_t i = 0; i < n_paths; ++i) {
            images[i] = read_whole_file(paths[i]);
            plans[i] = plan_columns(images[i].data(), images[i].size());
        }
        check_merge(plans);
        uint64_t n_labels = 0;
        for (const ColumnsPlan &p : plans) n_labels += p.labels.size();
        if (!plans[0].n_rows || !n_labels || n_labels >= (1u << 24)) { out->host_only = true; return MGX_OK; }
        b.build(plans);
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "%s: out of host memory", paths[0]);
    } catch (const std::runtime_error &e) {                      // ParseError, Unsupported, NeedsHost
        return host_answer(paths, n_paths, e.what());
    }
    images.clear();                                              // (the payloads are in b.stage)
    if (mgx_device_count() <= device || device < 0) return dfail(MGX_ERR_NO_DEVICE, "HIP device %d not available", device);
    HIP_TRY_D(hipSetDevice(device));
    const uint32_t n_labels = (uint32_t)b.lab.size(), n_sd = (uint32_t)b.sd.size();
    const uint64_t HW = b.high_words(), BW = b.bm_words(), RB = b.rrr_blocks();

    DBuf err, arena, t_rrr, t_sd, t_bm, t_lab, t_hprefix, hrank, bscan, counts, d_cb;
    Tables tables;
    TRY_D(err.alloc(8));
    HIP_TRY_D(hipMemset(err.p, 0xFF, 8));
    uint64_t *e = err.as<uint64_t>();
    TRY_D(arena.alloc(b.arena_words * 8));
    TRY_D(h2d(arena.p, b.stage.data(), b.upload_words * 8));
    if (b.arena_words > b.upload_words) HIP_TRY_D(hipMemset(arena.as<uint64_t>() + b.upload_words, 0, (b.arena_words - b.upload_words) * 8));
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
    if (key == DD_NO_ERROR && !b.col_begin_from(n_set, out->col_begin)) return host_answer(paths, n_paths, "more than 2^33 expanded rows");
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
        TRY_D(d2h(&key, e, 8));
    }
    if (key != DD_NO_ERROR) {
        char why[128];
        snprintf(why, sizeof(why), "column %u: %s at %u", (unsigned)(key >> 40), cd_check_name((uint32_t)(key >> 32) & 0xFF), (unsigned)(key & 0xFFFFFFFFu));
        return host_answer(paths, n_paths, why);
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
