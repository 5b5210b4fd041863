// mgx_colload.hip — `.column.annodbg` files decoded on the device: mgx_annotation_load_columns_device and the test hook
// mgx_column_file_decode_device (include/mgx.h, "files").  The host reads the files and walks their headers (col_plan.hpp); the
// payloads of ALL columns go into one arena with one copy, and the kernels below turn them into the columns' set rows in device
// memory, which mgx_annotation_create_sparse takes with on_device = 1.  DESIGN 3.17.
//
// Shapes: one lane per item of a concatenated buffer (an rrr block, a word of the sd high parts, a word of the bit maps); the
// number of launches and of device allocations depends on which of the four kinds of vector occur (sd, inverted sd, stat, rrr),
// not on how many there are.  The columns are one batch of bit vectors for the shared stage (decode_vectors; bodies:
// bv_decode.hpp), which leaves their bit maps and rank scans; then two passes (bodies: col_decode.hpp): counts per column (one
// copy of n_labels counts to the host, which forms col_begin), then every set row to rows[col_begin[j] + rank].  Scans: hipcub,
// 64-bit, on the null stream (the loader runs before any aligner exists).  The only atomics on data set the bits of an sd
// vector's stored positions in its cleared bit map.
//
// With coordinates (mgx_annotation_load_coord_columns_device): the tuple sections of the same load ride in the same
// arena (coord_plan.hpp: CoordBatch); their delimiter vectors are a second batch for the same stage, decoded after the binary
// columns, whose counts the delimiter checks need, and the cq_* bodies of coord_decode.hpp make coord_begin / coords in device
// memory of them; mgx_annotation_set_coordinates_device takes those.
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

// ---- the shared stage: a batch of bit vectors into bit maps and rank scans (bodies: bv_decode.hpp) ----
__global__ void __launch_bounds__(256) k_bv_rrr_width(const uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride,
                                                      const uint8_t *wtab, uint64_t *width, uint64_t total) {
    const uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb <= total) width[gb] = bv_rrr_width(arena, rd, rbprefix, n_rrr, rb_stride, wtab, gb);
}

__global__ void __launch_bounds__(256) k_bv_rrr_block(const uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride,
                                                      const uint64_t *off, const uint8_t *wtab, const uint64_t *binom, uint64_t *blocks, uint64_t total,
                                                      uint64_t *err) {
    __shared__ uint64_t C[DD_BINOM_ENTRIES];
    __shared__ uint8_t wt[64];
    for (uint32_t x = threadIdx.x; x < DD_BINOM_ENTRIES; x += blockDim.x) C[x] = binom[x];
    if (threadIdx.x < 64) wt[threadIdx.x] = wtab[threadIdx.x];
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; gb < total; gb += step)
        blocks[gb] = bv_rrr_block(arena, rd, rbprefix, n_rrr, rb_stride, off, wt, C, gb, err);
}

__global__ void __launch_bounds__(256) k_bv_rrr_pack(uint64_t *arena, const BvRrr *rd, const uint64_t *rbprefix, uint32_t n_rrr, uint64_t rb_stride,
                                                     const uint64_t *blocks, uint64_t total) {
    const uint64_t gb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb < total) bv_rrr_pack(arena, rd, rbprefix, n_rrr, rb_stride, blocks, gb);
}

__global__ void __launch_bounds__(256) k_bv_high_popcount(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, uint64_t *cnt,
                                                          uint64_t n_words) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw <= n_words) cnt[gw] = bv_high_popcount(arena, sd, hprefix, n_sd, gw);
}

__global__ void __launch_bounds__(256) k_bv_sd_scatter(uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank,
                                                       const BvMap *map, uint64_t n_words, uint64_t *err) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw < n_words) bv_sd_scatter(arena, sd, hprefix, n_sd, hrank, map, gw, err);
}

__global__ void __launch_bounds__(256) k_bv_map_popcount(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_map, uint64_t bm_stride,
                                                         uint64_t *cnt, uint64_t total) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= total) cnt[g] = bv_map_popcount(arena, map, bmprefix, n_map, bm_stride, g);
}

// ---- the binary columns: counts and the write pass (bodies: col_decode.hpp) ----
__global__ void __launch_bounds__(256) k_col_counts(const uint64_t *arena, const CdLabel *lab, const CdSd *sd, const BvMap *map, const uint64_t *hprefix,
                                                    const uint64_t *hrank, const uint64_t *bmprefix, const uint64_t *bscan, uint32_t n_labels,
                                                    uint64_t n_rows, uint64_t *counts, uint64_t *err) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_labels) counts[j] = cd_count(arena, lab, sd, map, hprefix, hrank, bmprefix, bscan, j, n_rows, err);
}

__global__ void __launch_bounds__(256) k_col_sd_rows(const uint64_t *arena, const CdSd *sd, const uint64_t *hprefix, uint32_t n_sd, const uint64_t *hrank,
                                                     uint64_t n_words, uint64_t n_rows, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint64_t gw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw < n_words) cd_sd_rows(arena, sd, hprefix, n_sd, hrank, gw, n_rows, col_begin, rows, err);
}

__global__ void __launch_bounds__(256) k_col_bm_extract(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_map, uint64_t bm_stride,
                                                        const uint64_t *bscan, uint64_t total, const uint64_t *col_begin, uint64_t *rows, uint64_t *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cd_bm_extract(arena, map, bmprefix, n_map, bm_stride, bscan, g, col_begin, rows, err);
}

// ---- coordinates: the checks, the rank pass and the values (bodies: coord_decode.hpp) ----
__global__ void __launch_bounds__(256) k_cq_check(const uint64_t *arena, const BvMap *map, const CqCol *col, const CdSd *sd, const uint64_t *hprefix,
                                                  const uint64_t *hrank, const uint64_t *bmprefix, const uint64_t *bscan, const uint64_t *col_begin,
                                                  uint32_t n_cols, uint64_t *err) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cols) cq_check(arena, map, col, sd, hprefix, hrank, bmprefix, bscan, col_begin, j, err);
}
__global__ void __launch_bounds__(256) k_cq_rank(const uint64_t *arena, const BvMap *map, const uint64_t *bmprefix, uint32_t n_cols, const uint64_t *bscan,
                                                 const uint64_t *col_begin, const uint64_t *vprefix, uint64_t total, uint64_t *coord_begin, uint64_t *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) cq_rank(arena, map, bmprefix, n_cols, bscan, col_begin, vprefix, g, coord_begin, err);
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

// a BvBatch on the device: its tables (the three prefix tables in one buffer) and, after decode_vectors, its two rank scans
struct BvDev {
    DBuf rrr, sd, map, prefix, hrank, bscan;
    const uint64_t *rbprefix = nullptr, *hprefix = nullptr, *bmprefix = nullptr;
    uint32_t n_rrr = 0, n_sd = 0, n_map = 0;
    uint64_t HW = 0, BW = 0;             // words of the high parts, of the bit maps
};
// one load on the device: the arena, the error word, the binomials of the rrr vectors, and the columns' tables
struct Device {
    DBuf err, arena, lab, counts, col_begin;
    Tables tables;
    BvDev cols;
    uint64_t *A = nullptr, *e = nullptr;
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

// the files' plans and the staged arena of out->b / out->cq.  MGX_OK with out->host_only: the caller takes the host reader's table
int plan_and_stage(const char *const *paths, uint32_t n_paths, bool coords, Loaded *out) {
    std::vector<std::vector<uint8_t>> images(n_paths), sides(coords ? n_paths : 0);
    std::vector<ColumnsPlan> plans(n_paths);
    std::vector<std::vector<TuplePlan>> tuples(coords ? n_paths : 0);
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
        if (coords) out->cq.layout(tp);
        out->b.build(plans, out->cq.upload_words);
        if (coords) out->cq.place(tp, out->b.extra_begin, out->b.arena_words, out->b.stage.data());
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "%s: out of host memory", paths[0]);
    } catch (const std::runtime_error &e) {                      // ParseError, Unsupported, NeedsHost
        return host_answer(paths, n_paths, e.what(), coords);
    }
    return MGX_OK;
}

// the error word, and the arena: the staged words with one copy, the bit maps (the columns', then the delimiters') cleared
int upload_arena(Loaded *l, Device &d) {
    ColBatch &b = l->b;
    TRY_D(d.err.alloc(8));
    HIP_TRY_D(hipMemset(d.err.p, 0xFF, 8));
    d.e = d.err.as<uint64_t>();
    const uint64_t arena_words = b.arena_words + l->cq.v.tail_words;
    TRY_D(d.arena.alloc(arena_words * 8));
    TRY_D(h2d(d.arena.p, b.stage.data(), b.upload_words * 8));
    if (arena_words > b.upload_words) HIP_TRY_D(hipMemset(d.arena.as<uint64_t>() + b.upload_words, 0, (arena_words - b.upload_words) * 8));
    std::vector<uint64_t>().swap(b.stage);
    d.A = d.arena.as<uint64_t>();
    return MGX_OK;
}

// The shared stage over one batch: rrr vectors to their bit maps (widths, one scan over all blocks, un-rank, pack); the rank of
// every word of the sd high parts, and the stored positions of the sd vectors that have a map into it; the rank of every word of
// the bit maps.  Leaves v's tables and the two scans (hrank, bscan) in d.
int decode_vectors(const BvBatch &v, Device &dev, BvDev &d) {
    uint64_t *A = dev.A;
    d.n_rrr = (uint32_t)v.rrr.size(); d.n_sd = (uint32_t)v.sd.size(); d.n_map = (uint32_t)v.map.size();
    d.HW = v.high_words(); d.BW = v.bm_words();
    const uint64_t RB = v.rrr_blocks();
    std::vector<uint64_t> prefix(v.rbprefix);
    prefix.insert(prefix.end(), v.hprefix.begin(), v.hprefix.end());
    prefix.insert(prefix.end(), v.bmprefix.begin(), v.bmprefix.end());
    TRY_D(upload_table(d.rrr, v.rrr));
    TRY_D(upload_table(d.sd, v.sd));
    TRY_D(upload_table(d.map, v.map));
    TRY_D(upload_table(d.prefix, prefix));
    d.rbprefix = d.prefix.as<uint64_t>();
    d.hprefix = d.rbprefix + v.rbprefix.size();
    d.bmprefix = d.hprefix + v.hprefix.size();
    TRY_D(d.hrank.alloc((d.HW + 1) * 8));
    TRY_D(d.bscan.alloc((d.BW + 1) * 8));
    if (RB) {
        DBuf off, blocks;
        if (!dev.tables.wtab.p) TRY_D(upload_tables(dev.tables));
        TRY_D(off.alloc((RB + 1) * 8));
        TRY_D(blocks.alloc(RB * 8));
        k_bv_rrr_width<<<grid_for(RB + 1), 256>>>(A, d.rrr.as<BvRrr>(), d.rbprefix, d.n_rrr, v.rb_stride, dev.tables.wtab.as<uint8_t>(), off.as<uint64_t>(), RB);
        LAUNCHED(0);
        TRY_D(scan_in_place(off.as<uint64_t>(), RB + 1));
        k_bv_rrr_block<<<grid_for(RB, 2048), 256>>>(A, d.rrr.as<BvRrr>(), d.rbprefix, d.n_rrr, v.rb_stride, off.as<uint64_t>(), dev.tables.wtab.as<uint8_t>(),
                                                     dev.tables.binom.as<uint64_t>(), blocks.as<uint64_t>(), RB, dev.e);
        LAUNCHED(0);
        k_bv_rrr_pack<<<grid_for(RB), 256>>>(A, d.rrr.as<BvRrr>(), d.rbprefix, d.n_rrr, v.rb_stride, blocks.as<uint64_t>(), RB);
        LAUNCHED(0);
    }
    if (d.n_sd) {
        k_bv_high_popcount<<<grid_for(d.HW + 1), 256>>>(A, d.sd.as<CdSd>(), d.hprefix, d.n_sd, d.hrank.as<uint64_t>(), d.HW);
        LAUNCHED(1);
        TRY_D(scan_in_place(d.hrank.as<uint64_t>(), d.HW + 1));
        if (v.sd_maps && d.HW) {
            k_bv_sd_scatter<<<grid_for(d.HW), 256>>>(A, d.sd.as<CdSd>(), d.hprefix, d.n_sd, d.hrank.as<uint64_t>(), d.map.as<BvMap>(), d.HW, dev.e);
            LAUNCHED(1);
        }
    }
    if (d.BW) {
        k_bv_map_popcount<<<grid_for(d.BW + 1), 256>>>(A, d.map.as<BvMap>(), d.bmprefix, d.n_map, v.bm_stride, d.bscan.as<uint64_t>(), d.BW);
        LAUNCHED(1);
        TRY_D(scan_in_place(d.bscan.as<uint64_t>(), d.BW + 1));
    }
    return MGX_OK;
}

// the first round trip: the set rows of every label, and the error word so far
int count_columns(const ColBatch &b, Device &dev, std::vector<uint64_t> &n_set, uint64_t *key) {
    const BvDev &d = dev.cols;
    const uint32_t n_labels = (uint32_t)b.lab.size();
    TRY_D(upload_table(dev.lab, b.lab));
    TRY_D(dev.counts.alloc((uint64_t)n_labels * 8));
    k_col_counts<<<grid_for(n_labels), 256>>>(dev.A, dev.lab.as<CdLabel>(), d.sd.as<CdSd>(), d.map.as<BvMap>(), d.hprefix, d.hrank.as<uint64_t>(), d.bmprefix,
                                              d.bscan.as<uint64_t>(), n_labels, b.n_rows, dev.counts.as<uint64_t>(), dev.e);
    LAUNCHED(1);
    n_set.resize(n_labels);
    TRY_D(d2h(n_set.data(), dev.counts.p, (uint64_t)n_labels * 8));  // (synchronises with the kernels)
    return d2h(key, dev.e, 8);
}

// the write pass: col_begin to the device, every set row to out->rows
int write_rows(const ColBatch &b, Device &dev, Loaded *out) {
    const BvDev &d = dev.cols;
    TRY_D(upload_table(dev.col_begin, out->col_begin));
    TRY_D(out->rows.alloc(out->col_begin.back() * 8));
    if (b.kinds[CD_KIND_SD] && d.HW) {
        k_col_sd_rows<<<grid_for(d.HW), 256>>>(dev.A, d.sd.as<CdSd>(), d.hprefix, d.n_sd, d.hrank.as<uint64_t>(), d.HW, b.n_rows, dev.col_begin.as<uint64_t>(),
                                               out->rows.as<uint64_t>(), dev.e);
        LAUNCHED(1);
    }
    if (d.BW) {
        k_col_bm_extract<<<grid_for(d.BW), 256>>>(dev.A, d.map.as<BvMap>(), d.bmprefix, d.n_map, b.v.bm_stride, d.bscan.as<uint64_t>(), d.BW, dev.col_begin.as<uint64_t>(),
                                                  out->rows.as<uint64_t>(), dev.e);
        LAUNCHED(1);
    }
    return MGX_OK;
}

// the tuple sections: the delimiter vectors through the shared stage, their checks, the rank pass, the unpack pass
int decode_coords(const CoordBatch &cq, Device &dev, Loaded *out) {
    const uint32_t n_cols = (uint32_t)cq.col.size();
    const uint64_t NV = cq.n_values(), *cb = dev.col_begin.as<uint64_t>();
    BvDev d;
    DBuf col, vprefix;
    TRY_D(decode_vectors(cq.v, dev, d));
    TRY_D(upload_table(col, cq.col));
    TRY_D(upload_table(vprefix, cq.vprefix));
    k_cq_check<<<grid_for(n_cols), 256>>>(dev.A, d.map.as<BvMap>(), col.as<CqCol>(), d.sd.as<CdSd>(), d.hprefix, d.hrank.as<uint64_t>(), d.bmprefix,
                                          d.bscan.as<uint64_t>(), cb, n_cols, dev.e);
    LAUNCHED(1);
    TRY_D(out->coord_begin.alloc((out->col_begin.back() + 1) * 8));
    TRY_D(out->coords.alloc(NV * 8));
    out->n_coords = NV;
    k_cq_rank<<<grid_for(d.BW), 256>>>(dev.A, d.map.as<BvMap>(), d.bmprefix, n_cols, d.bscan.as<uint64_t>(), cb, vprefix.as<uint64_t>(), d.BW,
                                       out->coord_begin.as<uint64_t>(), dev.e);
    LAUNCHED(1);
    if (NV) {
        k_cq_unpack<<<grid_for(NV), 256>>>(dev.A, col.as<CqCol>(), vprefix.as<uint64_t>(), n_cols, NV, out->coords.as<int64_t>(), dev.e);
        LAUNCHED(1);
    }
    return MGX_OK;
}

// the files' columns as col_begin (host) and rows (device); coords: and their tuple sections (the side files of form (a), or one
// file of form (b)) as coord_begin and coords (device).  MGX_OK with out->host_only: the caller takes the host reader's table
int decode_files(const char *const *paths, uint32_t n_paths, int device, Loaded *out, bool coords) {
    TRY_D(plan_and_stage(paths, n_paths, coords, out));
    if (out->host_only) return MGX_OK;
    if (mgx_device_count() <= device || device < 0) return dfail(MGX_ERR_NO_DEVICE, "HIP device %d not available", device);
    HIP_TRY_D(hipSetDevice(device));
    const ColBatch &b = out->b;
    Device dev;
    TRY_D(upload_arena(out, dev));
    TRY_D(decode_vectors(b.v, dev, dev.cols));
    std::vector<uint64_t> n_set;
    uint64_t key = DD_NO_ERROR;
    TRY_D(count_columns(b, dev, n_set, &key));
    if (key == DD_NO_ERROR && !b.col_begin_from(n_set, out->col_begin)) return host_answer(paths, n_paths, "more than 2^33 expanded rows", coords);
    if (key == DD_NO_ERROR && coords && !out->cq.lengths_fit(out->col_begin)) return host_answer(paths, n_paths, "delimiters: length", coords);
    if (key == DD_NO_ERROR) {
        TRY_D(write_rows(b, dev, out));
        if (coords) TRY_D(decode_coords(out->cq, dev, out));
        TRY_D(d2h(&key, dev.e, 8));                              // the second round trip
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

// What the four entry points do (who: the entry point, for its messages).  The hooks copy the decoded tables back into *file;
// the loaders create *annot from them in device memory, and *file (optional) keeps the labels and col_begin.
int load(const char *who, const char *const *paths, uint32_t n_paths, int device, bool coords, mgx_annotation **annot, bool hook, mgx_column_file **file) {
    if (!paths || !n_paths || (hook ? !file : !annot)) return dfail(MGX_ERR_INVALID, "%s: bad arguments", who);
    if (annot) *annot = nullptr;
    if (file) *file = nullptr;
    TRY_D(bad_paths(who, paths, n_paths));
    Loaded l;
    TRY_D(decode_files(paths, n_paths, device, &l, coords));
    const auto host_read = coords ? mgx_column_coord_file_read : mgx_column_file_read;
    std::unique_ptr<mgx_column_file> m;
    if (l.host_only) {                                           // an empty matrix: the host reader's tables, nothing for a kernel to do
        if (hook) return host_read(paths, n_paths, file);
        mgx_column_file *cf = nullptr;
        TRY_D(host_read(paths, n_paths, &cf));
        m.reset(cf);
        TRY_D(mgx_annotation_create_from_file(cf, device, annot));
        m->f.rows.clear(); m->f.coord_begin.clear(); m->f.coords.clear();
        m->f.has_coords = false;
    } else {
        ColumnFile *f = nullptr;
        const uint64_t total = l.col_begin.back();
        try {
            m.reset(new mgx_column_file());
            f = &m->f;
            f->n_rows = l.b.n_rows;
            f->labels = l.b.labels;
            f->col_begin = l.col_begin;
            if (hook) f->rows.resize(total);
            if (hook && coords) { f->coord_begin.resize(total + 1); f->coords.resize(l.n_coords); f->has_coords = true; }
        } catch (const std::bad_alloc &) {
            return dfail(MGX_ERR_OOM, "%s: out of host memory", who);
        }
        const uint32_t n_labels = (uint32_t)l.b.lab.size();
        if (hook) {
            TRY_D(d2h(f->rows.data(), l.rows.p, total * 8));
            TRY_D(d2h(f->coord_begin.data(), l.coord_begin.p, f->coord_begin.size() * 8));
            TRY_D(d2h(f->coords.data(), l.coords.p, f->coords.size() * 8));
            // a descending tuple is what the transposition's kernel finds in a load; the hook has no transposition: the host reader's word
            for (uint64_t x = 0; x + 1 < f->coord_begin.size(); ++x)
                for (uint64_t t = f->coord_begin[x] + 1; t < f->coord_begin[x + 1]; ++t)
                    if (f->coords[t] < f->coords[t - 1]) return host_answer(paths, n_paths, "a tuple is not ascending", true);
        } else {
            TRY_D(mgx_annotation_create_sparse(l.b.n_rows, n_labels, l.col_begin.data(), l.rows.as<uint64_t>(), 1, device, annot));
            const int rc = !coords ? MGX_OK : mgx_annotation_set_coordinates_device(*annot, n_labels, l.col_begin.data(), l.rows.as<uint64_t>(),
                                                                                     l.coord_begin.as<uint64_t>(), l.coords.as<int64_t>());
            if (rc != MGX_OK) {
                mgx_annotation_destroy(*annot);
                *annot = nullptr;
                // (a descending tuple: the host reader names it; any other failure keeps its own code and message)
                return rc == MGX_ERR_INVALID ? host_answer(paths, n_paths, "a tuple is not ascending", true) : rc;
            }
        }
    }
    if (!hook) m->rows_on_device = true;
    if (file) *file = m.release();
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
    return load("mgx_column_file_decode_device", paths, n_paths, device, false, nullptr, true, out);
}

int mgx_column_coord_file_decode_device(const char *const *paths, uint32_t n_paths, int device, mgx_column_file **out) {
    return load("mgx_column_coord_file_decode_device", paths, n_paths, device, true, nullptr, true, out);
}

int mgx_annotation_load_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out) {
    return load("mgx_annotation_load_columns_device", paths, n_paths, device, false, out, false, names_out);
}

int mgx_annotation_load_coord_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out) {
    return load("mgx_annotation_load_coord_columns_device", paths, n_paths, device, true, out, false, names_out);
}

}  // extern "C"
