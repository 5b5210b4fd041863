// dbg_kernels.hpp — the kernels and launch helpers that the units decoding the reference's files on the device share
// (mgx_dbgload.hip: `.dbg`; mgx_colload.hip: `.column.annodbg`): the rrr_vector<63> kernels, the popcount / rank directory, the
// total and failure records (bodies: dbg_decode.hpp), the device buffer, the counted copies and the in-place scan.  Everything
// here has internal linkage: each including unit has kernels, counters and helpers of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/mgx.h"
#include "dbg_decode.hpp"
#include "dbg_plan.hpp"
#include "kernel_units.hpp"

namespace {

using namespace mgx;
using namespace mgx::files;

// =================================================================================================
// kernels
// =================================================================================================
__global__ void __launch_bounds__(256) k_rrr_width(const uint64_t *bt, const uint8_t *wtab, uint64_t *width, uint64_t n_blocks) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= n_blocks) width[b] = dd_rrr_width(bt, wtab, b, n_blocks);
}

__global__ void __launch_bounds__(256) k_rrr_block(const uint64_t *bt, const uint64_t *btnr, uint64_t btnr_bits, const uint64_t *off,
                                                   const uint8_t *wtab, const uint64_t *binom, uint64_t *blocks, uint64_t n_blocks,
                                                   uint64_t *err, uint32_t check_early) {
    __shared__ uint64_t C[DD_BINOM_ENTRIES];
    __shared__ uint8_t wt[64];
    for (uint32_t x = threadIdx.x; x < DD_BINOM_ENTRIES; x += blockDim.x) C[x] = binom[x];
    if (threadIdx.x < 64) wt[threadIdx.x] = wtab[threadIdx.x];
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += step)
        blocks[b] = dd_rrr_block(bt, btnr, btnr_bits, off, wt, C, b, err, check_early);
}

__global__ void __launch_bounds__(256) k_rrr_pack(const uint64_t *blocks, uint64_t n_blocks, uint64_t bits, uint64_t *out, uint64_t n_words) {
    const uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi < n_words) out[wi] = dd_rrr_pack(blocks, n_blocks, bits, wi);
}

// cnt[wi] = the set bits of word wi, wi < n_words = dd_words(bits) (the pad words: 0); scanned in place it is the rank directory
__global__ void __launch_bounds__(256) k_popcount(const uint64_t *w, uint64_t bits, uint64_t *cnt, uint64_t n_words) {
    const uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi < n_words) cnt[wi] = dd_popcount_word(w, wi, bits);
}

__global__ void k_check_total(const uint64_t *total, uint64_t expect, uint32_t check, uint64_t *err) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && *total != expect) dd_fail(err, check, *total);
}

__global__ void k_fail(uint64_t *err, uint32_t check, uint64_t pos) {
    if (threadIdx.x == 0 && blockIdx.x == 0) dd_fail(err, check, pos);
}

// =================================================================================================
// host
// =================================================================================================
std::atomic<uint64_t> g_counts[4];       // launches counted in slot 0 (the rrr kernels) and slot 1 (the others), bytes H2D, bytes D2H
std::atomic<uint64_t> g_allocs;          // device allocations (DBuf::alloc)

int dfail(int code, const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    mgx_set_last_error(buf);
    return code;
}
#define HIP_TRY_D(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) return dfail(MGX_ERR_NO_DEVICE, "%s: %s", #e, hipGetErrorString(r_)); } while (0)
#define TRY_D(e) do { if (int rc_ = (e)) return rc_; } while (0)

struct DBuf {
    void *p = nullptr;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    ~DBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    int alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        ++g_allocs;
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return dfail(MGX_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
        return MGX_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

uint32_t grid_for(uint64_t n, uint64_t cap = 0) {
    uint64_t b = (n + 255) / 256;
    if (cap && b > cap) b = cap;
    return (uint32_t)(b ? b : 1);
}
int h2d(void *dst, const void *src, size_t bytes) {
    if (bytes) { HIP_TRY_D(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); g_counts[2] += bytes; }
    return MGX_OK;
}
int d2h(void *dst, const void *src, size_t bytes) {
    if (bytes) { HIP_TRY_D(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); g_counts[3] += bytes; }
    return MGX_OK;
}
#define LAUNCHED(slot) do { HIP_TRY_D(hipGetLastError()); ++g_counts[slot]; } while (0)

// a payload as the kernels want it: an aligned buffer of its own, the words of the file and two zero words behind them
int upload(DBuf &d, const RawVec &v) {
    const uint64_t nw = v.words();
    TRY_D(d.alloc(dd_words(v.bits) * 8));
    TRY_D(h2d(d.p, v.src, nw * 8));
    HIP_TRY_D(hipMemset(d.as<uint64_t>() + nw, 0, 16));
    return MGX_OK;
}

// d[0 .. n) <- its exclusive sums
int scan_in_place(uint64_t *d, uint64_t n) {
    size_t tmp_bytes = 0;
    HIP_TRY_D(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d, d, (size_t)n));
    DBuf tmp;
    TRY_D(tmp.alloc(tmp_bytes));
    HIP_TRY_D(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, d, d, (size_t)n));
    return MGX_OK;
}

struct Tables { DBuf wtab, binom; };
int upload_tables(Tables &t) {
    const auto &C = binomial63().c;
    uint8_t wtab[64];
    std::vector<uint64_t> flat(DD_BINOM_ENTRIES);
    for (unsigned k = 0; k < 64; ++k) wtab[k] = (k == 0 || k == 63) ? 0 : (uint8_t)(64 - __builtin_clzll(C[63][k]));
    for (unsigned n = 0; n < 63; ++n) for (unsigned j = 0; j < 32; ++j) flat[n * 32 + j] = C[n][j];
    TRY_D(t.wtab.alloc(64));
    TRY_D(t.binom.alloc(flat.size() * 8));
    TRY_D(h2d(t.wtab.p, wtab, 64));
    return h2d(t.binom.p, flat.data(), flat.size() * 8);
}

// an rrr_vector<63> -> out: dd_words(bits) words (the pad words zero)
int decode_rrr(const RrrPlan &r, Tables &t, uint64_t *err, uint32_t check_early, DBuf &out) {
    if (!t.wtab.p) TRY_D(upload_tables(t));
    DBuf bt, btnr, off, blocks;
    TRY_D(upload(bt, r.bt));
    TRY_D(upload(btnr, r.btnr));
    TRY_D(off.alloc((r.n_blocks + 1) * 8));
    TRY_D(blocks.alloc(r.n_blocks * 8));
    k_rrr_width<<<grid_for(r.n_blocks + 1), 256>>>(bt.as<uint64_t>(), t.wtab.as<uint8_t>(), off.as<uint64_t>(), r.n_blocks);
    LAUNCHED(0);
    TRY_D(scan_in_place(off.as<uint64_t>(), r.n_blocks + 1));
    if (r.n_blocks) {
        k_rrr_block<<<grid_for(r.n_blocks, 2048), 256>>>(bt.as<uint64_t>(), btnr.as<uint64_t>(), r.btnr.bits, off.as<uint64_t>(), t.wtab.as<uint8_t>(),
                                                         t.binom.as<uint64_t>(), blocks.as<uint64_t>(), r.n_blocks, err, check_early);
        LAUNCHED(0);
    }
    const uint64_t nw = dd_words(r.bits);
    TRY_D(out.alloc(nw * 8));
    k_rrr_pack<<<grid_for(nw), 256>>>(blocks.as<uint64_t>(), r.n_blocks, r.bits, out.as<uint64_t>(), nw);
    LAUNCHED(0);
    return MGX_OK;
}

// dir[0 .. dd_words(bits)) = the set bits in front of every word of w (dir[ceil(bits / 64)] = all of them)
int rank_directory(const uint64_t *w, uint64_t bits, DBuf &dir) {
    const uint64_t nw = dd_words(bits);
    TRY_D(dir.alloc(nw * 8));
    k_popcount<<<grid_for(nw), 256>>>(w, bits, dir.as<uint64_t>(), nw);
    LAUNCHED(1);
    return scan_in_place(dir.as<uint64_t>(), nw);
}

}  // namespace
