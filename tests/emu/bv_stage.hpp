// tests/emu/bv_stage.hpp — TEST ONLY: the host replay of the stages that mgx_colload.hip launches, one call per item in the order
// of the launches: the shared stage over a batch of bit vectors (decode_vectors; bodies: bv_decode.hpp) and the two passes of the
// binary columns on top of it (count_columns, write_rows; bodies: col_decode.hpp).  Used by col_decode_check.cpp and
// coord_decode_check.cpp.  Every array has exactly the size the driver gives its device buffer (the three prefix tables, which the
// driver uploads in one buffer, are arrays of their own here), so that under -fsanitize=address an access the kernels would make
// outside a buffer stops the program.
#pragma once
#include "../../metagraph_amd/csrc/col_plan.hpp"

#include <vector>

using namespace mgx;
using namespace mgx::files;

typedef std::vector<uint64_t> Words;

static void scan(Words &d) {
    uint64_t s = 0;
    for (uint64_t &x : d) { const uint64_t c = x; x = s; s += c; }
}

// a batch's tables (copies at their exact sizes: the data() of an empty table is not dereferenced by a correct body) and scans
struct BvHost {
    std::vector<BvRrr> rrr;
    std::vector<CdSd> sd;
    std::vector<BvMap> map;
    Words rbprefix, hprefix, bmprefix, hrank, bscan;
    uint32_t n_rrr, n_sd, n_map;
    uint64_t HW, BW;
    explicit BvHost(const BvBatch &v)
        : rrr(v.rrr), sd(v.sd), map(v.map), rbprefix(v.rbprefix), hprefix(v.hprefix), bmprefix(v.bmprefix), hrank(v.high_words() + 1),
          bscan(v.bm_words() + 1), n_rrr((uint32_t)v.rrr.size()), n_sd((uint32_t)v.sd.size()), n_map((uint32_t)v.map.size()), HW(v.high_words()),
          BW(v.bm_words()) {}
};

// decode_vectors
static void bv_stage(uint64_t *A, const BvBatch &v, BvHost &d, uint64_t *err) {
    const uint64_t RB = v.rrr_blocks();
    if (RB) {
        const auto &C = binomial63().c;
        std::vector<uint8_t> wtab(64);
        Words binom(DD_BINOM_ENTRIES), off(RB + 1), blocks(RB);
        for (unsigned k = 0; k < 64; ++k) wtab[k] = (k == 0 || k == 63) ? 0 : (uint8_t)(64 - __builtin_clzll(C[63][k]));
        for (unsigned n = 0; n < 63; ++n) for (unsigned j = 0; j < 32; ++j) binom[n * 32 + j] = C[n][j];
        for (uint64_t gb = 0; gb <= RB; ++gb) off[gb] = bv_rrr_width(A, d.rrr.data(), d.rbprefix.data(), d.n_rrr, v.rb_stride, wtab.data(), gb);
        scan(off);
        for (uint64_t gb = 0; gb < RB; ++gb)
            blocks[gb] = bv_rrr_block(A, d.rrr.data(), d.rbprefix.data(), d.n_rrr, v.rb_stride, off.data(), wtab.data(), binom.data(), gb, err);
        for (uint64_t gb = 0; gb < RB; ++gb) bv_rrr_pack(A, d.rrr.data(), d.rbprefix.data(), d.n_rrr, v.rb_stride, blocks.data(), gb);
    }
    if (d.n_sd) {
        for (uint64_t gw = 0; gw <= d.HW; ++gw) d.hrank[gw] = bv_high_popcount(A, d.sd.data(), d.hprefix.data(), d.n_sd, gw);
        scan(d.hrank);
        if (v.sd_maps)
            for (uint64_t gw = 0; gw < d.HW; ++gw) bv_sd_scatter(A, d.sd.data(), d.hprefix.data(), d.n_sd, d.hrank.data(), d.map.data(), gw, err);
    }
    if (d.BW) {
        for (uint64_t g = 0; g <= d.BW; ++g) d.bscan[g] = bv_map_popcount(A, d.map.data(), d.bmprefix.data(), d.n_map, v.bm_stride, g);
        scan(d.bscan);
    }
}

// count_columns
static Words col_counts(const uint64_t *A, const ColBatch &b, const BvHost &d, uint64_t *err) {
    const std::vector<CdLabel> lab(b.lab);
    Words counts(lab.size());
    for (uint32_t j = 0; j < lab.size(); ++j)
        counts[j] = cd_count(A, lab.data(), d.sd.data(), d.map.data(), d.hprefix.data(), d.hrank.data(), d.bmprefix.data(), d.bscan.data(), j, b.n_rows, err);
    return counts;
}

// write_rows; cb: col_begin at its size, rows: cb.back() entries
static void col_rows(const uint64_t *A, const ColBatch &b, const BvHost &d, const Words &cb, uint64_t *rows, uint64_t *err) {
    if (b.kinds[CD_KIND_SD])
        for (uint64_t gw = 0; gw < d.HW; ++gw) cd_sd_rows(A, d.sd.data(), d.hprefix.data(), d.n_sd, d.hrank.data(), gw, b.n_rows, cb.data(), rows, err);
    for (uint64_t g = 0; g < d.BW; ++g) cd_bm_extract(A, d.map.data(), d.bmprefix.data(), d.n_map, b.v.bm_stride, d.bscan.data(), g, cb.data(), rows, err);
}
