// mgx.hip — libmgx.so: gfx950 kernels and the C-ABI of include/mgx.h.
// Host side is plain C++ around the HIP runtime; there is no CPU execution path for the aligner.
#include <hip/hip_runtime.h>
#include "pack_swar.hpp"
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/mgx.h"
#define MGX_NO_EXTEND 1      // this unit holds k_map and the seeding kernel; the extension lives in mgx_grp.hip
#include "graph_build.hpp"
#include "map_pipe.hpp"
#include "host_common.hpp"
#include "chain_host.hpp"
#include "lane_types.hpp"
#include "seed_lane.hpp"
#include "kernel_units.hpp"
#include "tsv_format.hpp"
#include "map_format.hpp"
#include "json_format.hpp"
#include "results_decode.hpp"

using namespace mgx;
static_assert(sizeof(AlignParams) == MGX_ALIGN_PARAMS_BYTES && sizeof(LaneParams) == MGX_LANE_PARAMS_BYTES
              && sizeof(SeedLaneParams) == MGX_SEED_LANE_PARAMS_BYTES, "a parameter block differs from what the kernel units take");
// the records the decode kernels write (results_decode.hpp) are the public ones, field by field
static_assert(sizeof(RdBatch) == MGX_DECODE_ARGS_BYTES, "RdBatch differs from what mgx_decode.hip takes");
static_assert(sizeof(RdCigarOp) == sizeof(mgx_cigar_op) && offsetof(RdCigarOp, len) == offsetof(mgx_cigar_op, len)
              && offsetof(RdCigarOp, op) == offsetof(mgx_cigar_op, op) && offsetof(RdCigarOp, pad) == offsetof(mgx_cigar_op, _pad),
              "RdCigarOp is not mgx_cigar_op");
static_assert(sizeof(RdAlignment) == sizeof(mgx_alignment) && offsetof(RdAlignment, score) == offsetof(mgx_alignment, score)
              && offsetof(RdAlignment, offset) == offsetof(mgx_alignment, offset) && offsetof(RdAlignment, clipping) == offsetof(mgx_alignment, clipping)
              && offsetof(RdAlignment, end_clipping) == offsetof(mgx_alignment, end_clipping)
              && offsetof(RdAlignment, num_matches) == offsetof(mgx_alignment, num_matches) && offsetof(RdAlignment, n_nodes) == offsetof(mgx_alignment, n_nodes)
              && offsetof(RdAlignment, n_cigar) == offsetof(mgx_alignment, n_cigar) && offsetof(RdAlignment, seq_len) == offsetof(mgx_alignment, seq_len)
              && offsetof(RdAlignment, nodes_begin) == offsetof(mgx_alignment, nodes_begin)
              && offsetof(RdAlignment, cigar_begin) == offsetof(mgx_alignment, cigar_begin) && offsetof(RdAlignment, seq_begin) == offsetof(mgx_alignment, seq_begin)
              && offsetof(RdAlignment, orientation) == offsetof(mgx_alignment, orientation) && offsetof(RdAlignment, pad) == offsetof(mgx_alignment, _pad)
              && offsetof(RdAlignment, n_labels) == offsetof(mgx_alignment, n_labels) && offsetof(RdAlignment, labels_begin) == offsetof(mgx_alignment, labels_begin),
              "RdAlignment is not mgx_alignment");
static_assert(sizeof(mgx_results_sizes) == RD_ARRAYS * 8, "mgx_results_sizes is the five totals in the order of RdArray");

// =================================================================================================
// kernels
// =================================================================================================
__global__ void k_build_pass1(const uint8_t *W, const uint8_t *last, uint64_t n, Block *blocks, uint32_t *counts, uint32_t n_blocks) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_blocks) build_block_pass1(b, W, last, n, blocks, counts);
}

struct HintPtrs { uint32_t *last_hint; uint32_t *w_hint[4]; };
__global__ void k_sel_anchor(DevGraph g, uint32_t shift, uint32_t n_entries, uint32_t total_last, uint32_t *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_entries) build_sel_anchor(g, j, shift, n_entries, total_last, out);
}

__global__ void k_build_pass2(Block *blocks, const uint32_t *cum, HintPtrs hp, uint32_t n_blocks) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_blocks) build_block_pass2(b, blocks, cum, hp.last_hint, hp.w_hint);
}

__global__ void k_parent(DevGraph g, uint32_t *P, uint8_t *D) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e <= g.n) { P[e] = build_parent(g, e); D[e] = (uint8_t)node_last_value(g, e); }
}

__global__ void k_gather(const uint32_t *P, const uint8_t *Din, uint8_t *Dout, uint64_t n) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e <= n) Dout[e] = Din[P[e]];
}

__global__ void k_key_step(const uint8_t *D, uint32_t *key, uint64_t n, uint32_t m, uint32_t r) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e <= n) key[e] = build_key_step(r ? key[e] : 0u, D[e], m, r);
}

__global__ void k_prefix_init(uint2 *tbl, uint64_t entries) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < entries) tbl[i] = make_uint2(1u, 0u);        // empty range (rl > ru)
}

__global__ void k_prefix_fill(const uint32_t *key, uint64_t n, uint2 *tbl) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 1 && e <= n) build_prefix_entry(key, e, n, tbl);
}

__global__ void k_pack_firstc(const uint8_t *D, uint32_t *firstc, uint64_t n) {
    uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi * 8 <= n) {
        uint32_t v = 0;
        for (int j = 0; j < 8; ++j) {
            uint64_t e = wi * 8 + j;
            if (e <= n) v |= (uint32_t)(D[e] & 0xF) << (4 * j);
        }
        firstc[wi] = v;
    }
}

__global__ void k_pack_valid(const uint8_t *valid, uint64_t *bits, uint64_t n) {
    uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi * 64 <= n) {
        uint64_t v = 0;
        for (int j = 0; j < 64; ++j) {
            uint64_t e = wi * 64 + j;
            if (e <= n && valid[e]) v |= 1ull << j;
        }
        bits[wi] = v;
    }
}

__global__ void k_terminus(DevGraph g, uint64_t *bits) {
    uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;       // blockDim multiple of 64
    bool t = v <= g.n && in_graph(g, v) && build_terminus(g, v);
    uint64_t m = __ballot(t);
    if ((threadIdx.x & 63) == 0 && (v >> 6) < ((g.n + 64) >> 6)) bits[v >> 6] = m;
}

// PRIMARY graphs: the wrapper's terminus bits of both ids of every base node (canon_graph.hpp)
__global__ void k_terminus_primary(DevGraph g, uint64_t *bits, uint64_t *bits_rc) {
    uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;       // blockDim multiple of 64
    const uint32_t t = (v <= g.n && in_graph(g, v)) ? build_terminus_primary(g, v) : 0u;
    const uint64_t m0 = __ballot(t & 1u), m1 = __ballot(t & 2u);
    if ((threadIdx.x & 63) == 0 && (v >> 6) < ((g.n + 64) >> 6)) { bits[v >> 6] = m0; bits_rc[v >> 6] = m1; }
}

// PRIMARY graphs (unless MGX_PRIMARY_TABLES=0): palindrome bit of every edge and, per BOSS node, the last edge of its
// reverse complement's node (canon_graph.hpp, canon_children_tables)
__global__ void k_primary_tables(DevGraph g, uint64_t *pal, uint32_t *rc_node) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;       // blockDim multiple of 64
    const bool live = e >= 1 && e <= g.n;
    const uint64_t m = __ballot(live && build_pal_bit(g, e));
    if ((threadIdx.x & 63) == 0 && (e >> 6) < ((g.n + 64) >> 6)) pal[e >> 6] = m;
    if (live) {
        const Block b = load_block(g, (uint32_t)(e >> 6));
        if ((b.last_bits >> (e & 63)) & 1)
            rc_node[b.last_cum + (uint32_t)popc64(b.last_bits & mask_upto((int)(e & 63)))] = build_rc_node(g, e);
    }
}

// PRIMARY graphs: base-graph mappings of both strands -> the wrapper's paths (canon_merge_pair), one wavefront per read
__global__ void k_canon_merge(DevGraph g, const char *seqs, const uint64_t *offsets, const uint64_t *node_begin,
                              uint32_t *nodes_fwd, uint32_t *nodes_rc, uint64_t n_reads) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = (int)(threadIdx.x & 63);
    for (uint64_t read = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; read < n_reads; read += n_waves) {
        const uint64_t off = offsets[read], nb = node_begin[read];
        const int32_t L = (int32_t)(offsets[read + 1] - off);
        const int32_t nk = (int32_t)(node_begin[read + 1] - nb);
        for (int32_t i = lane; i < nk; i += 64) canon_merge_pair(g, seqs + off, L, i, nodes_fwd + nb, nodes_rc + nb);
    }
}

__global__ void k_kmer_counts(const uint64_t *offsets, uint64_t n_reads, uint32_t k, uint64_t *counts, unsigned long long *lmax) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long L = 0;
    if (i < n_reads) {
        L = offsets[i + 1] - offsets[i];
        counts[i] = L >= k ? L - k + 1 : 0;
    }
    if (i == n_reads) counts[i] = 0;
    // the batch's longest read: one atomic per wavefront (10 M atomics on one address were most of this kernel's 1.6 ms)
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(L, d); L = o > L ? o : L; }
    if ((threadIdx.x & 63) == 0 && L) atomicMax(lmax, L);
}

#ifndef MGX_MAP_BLOCKS_PER_CU
#define MGX_MAP_BLOCKS_PER_CU 8          // 256-thread blocks resident per CU (8 = 32 waves: full occupancy if registers allow)
#endif
// persistent lanes, one (read, strand) chain at a time (map_lane_step); 6 waves/SIMD (80 VGPRs, 1 spill) measured best
// for this latency-bound gather kernel (5: +6 %, 8: +3 %)
__global__ void __launch_bounds__(256, 6) k_map(DevGraph g, const char *seqs, const uint64_t *offsets, const uint64_t *node_begin,
                                             uint32_t *nodes_fwd, uint32_t *nodes_rc, uint8_t *mlen_fwd, uint8_t *mlen_rc,
                                             uint2 *rng_fwd, uint2 *rng_rc, int min_rng_len,
                                             uint64_t n_reads, int do_rc, unsigned long long *cursor, KernelStats *stats) {
    LineCtr ctr = { 0, 0, 0 };
    MapLane m;
    m.state = 0;
    const uint64_t n_chains = do_rc ? 2 * n_reads : n_reads;
    auto fetch = [&](MapLane &ml) -> bool {
        uint64_t c = atomicAdd(cursor, 1ull);
        if (c >= n_chains) return false;
        uint64_t read = do_rc ? (c >> 1) : c;
        ml.strand = do_rc ? (int)(c & 1) : 0;
        uint64_t off = offsets[read];
        ml.L = (int32_t)(offsets[read + 1] - off);
        ml.seq = seqs + off;
        ml.out = (ml.strand ? nodes_rc : nodes_fwd) + node_begin[read];
        ml.out_len = (ml.strand ? mlen_rc : mlen_fwd) + node_begin[read];
        uint2 *rg = ml.strand ? rng_rc : rng_fwd;
        ml.out_rng = rg ? rg + node_begin[read] : nullptr;
        ml.min_rng_len = min_rng_len;
        ml.n_kmers = ml.L - (int32_t)g.k + 1;
        return true;
    };
    while (m.state != 3) map_lane_step(g, m, ctr, fetch);
    // per-wave reduction of the line counters
    uint32_t r = ctr.rank_lines, s = ctr.select_lines, b = ctr.bit_lines;
    for (int d = 32; d >= 1; d >>= 1) { r += __shfl_xor(r, d, 64); s += __shfl_xor(s, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0 && (r | s | b)) {
        atomicAdd(&stats->rank_lines, (unsigned long long)r);
        atomicAdd(&stats->select_lines, (unsigned long long)s);
        atomicAdd(&stats->bit_lines, (unsigned long long)b);
        atomicAdd(&stats->map_lines, (unsigned long long)r + s + b);
    }
}

// 2-bit packing pre-pass of the mapping kernel (graph_build.hpp, pack_read_word): one thread per (read, 32-base word)
__global__ void k_pack_reads(const char *seqs, const uint64_t *offsets, uint64_t n_reads, uint32_t words_per_read, int do_rc,
                             uint64_t *pk_fwd, uint64_t *pk_rc, uint32_t *iv_fwd, uint32_t *iv_rc) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t read = t / words_per_read;
    const int32_t j = (int32_t)(t % words_per_read);
    if (read >= n_reads) return;
    const uint64_t off = offsets[read];
    const int32_t L = (int32_t)(offsets[read + 1] - off);
    if (32 * j >= L) return;
    const uint64_t w = packed_word_begin(off, read) + (uint64_t)j;
    uint64_t c; uint32_t v;
    // 32 characters at a time (pack_swar.hpp) where the word's 32 bytes lie inside the batch; the byte loop at its two ends
    const uint64_t total = offsets[n_reads];
    auto load32 = [&](uint64_t at, uint64_t *b) {
        const char *p = seqs + at;
        for (int x = 0; x < 4; ++x) { uint64_t q; __builtin_memcpy(&q, p + 8 * x, 8); b[x] = q; }
    };
    const int32_t p0 = 32 * j, nf = L - p0 < 32 ? L - p0 : 32;
    if (off + (uint64_t)p0 + 32 <= total) {
        uint64_t b[4];
        load32(off + (uint64_t)p0, b);
        mgx_pack::pack32(b, nf, 0, &c, &v);
    } else pack_read_word(seqs + off, L, 0, j, &c, &v);
    pk_fwd[w] = c; iv_fwd[w] = v;
    if (do_rc) {
        // strand position 32 j + t of the reverse complement is read position L - 1 - 32 j - t: the 32 bytes from lo on, backwards
        const int64_t lo = (int64_t)L - 32 * (int64_t)j - 32;
        if ((int64_t)off + lo >= 0) {
            uint64_t b[4];
            load32((uint64_t)((int64_t)off + lo), b);
            mgx_pack::pack32(b, nf, 1, &c, &v);
        } else pack_read_word(seqs + off, L, 1, j, &c, &v);
        pk_rc[w] = c; iv_rc[w] = v;
    }
}

// k_map over the packed reads (k <= 32): same chains, same primitives, same outputs (map_lane_step_packed)
#ifndef MGX_MAP_PACKED_WAVES
#define MGX_MAP_PACKED_WAVES 6
#endif
__global__ void __launch_bounds__(256, MGX_MAP_PACKED_WAVES) k_map_packed(DevGraph g, const uint64_t *offsets, const uint64_t *node_begin,
                                             const uint64_t *pk_fwd, const uint64_t *pk_rc, const uint32_t *iv_fwd, const uint32_t *iv_rc,
                                             uint32_t *nodes_fwd, uint32_t *nodes_rc, uint8_t *mlen_fwd, uint8_t *mlen_rc,
                                             uint2 *rng_fwd, uint2 *rng_rc, int min_rng_len,
                                             uint64_t n_reads, int do_rc, unsigned long long *cursor, KernelStats *stats) {
    LineCtr ctr = { 0, 0, 0 };
    MapLanePacked m;
    m.state = 0;
    const uint64_t n_chains = do_rc ? 2 * n_reads : n_reads;
    auto fetch = [&](MapLanePacked &ml) -> bool {
        uint64_t c = atomicAdd(cursor, 1ull);
        if (c >= n_chains) return false;
        const uint64_t read = do_rc ? (c >> 1) : c;
        const int strand = do_rc ? (int)(c & 1) : 0;
        const uint64_t off = offsets[read];
        const int32_t L = (int32_t)(offsets[read + 1] - off);
        const uint64_t w = packed_word_begin(off, read);
        ml.pk = (strand ? pk_rc : pk_fwd) + w;
        ml.iv = (strand ? iv_rc : iv_fwd) + w;
        ml.n_words = (L + 31) >> 5;
        ml.out = (strand ? nodes_rc : nodes_fwd) + node_begin[read];
        ml.out_len = (strand ? mlen_rc : mlen_fwd) + node_begin[read];
        uint2 *rg = strand ? rng_rc : rng_fwd;
        ml.out_rng = rg ? rg + node_begin[read] : nullptr;
        ml.min_rng_len = min_rng_len;
        ml.n_kmers = L - (int32_t)g.k + 1;
        return true;
    };
    while (m.state != 3) map_lane_step_packed(g, m, ctr, fetch);
    uint32_t r = ctr.rank_lines, s = ctr.select_lines, b = ctr.bit_lines;
    for (int d = 32; d >= 1; d >>= 1) { r += __shfl_xor(r, d, 64); s += __shfl_xor(s, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0 && (r | s | b)) {
        atomicAdd(&stats->rank_lines, (unsigned long long)r);
        atomicAdd(&stats->select_lines, (unsigned long long)s);
        atomicAdd(&stats->bit_lines, (unsigned long long)b);
        atomicAdd(&stats->map_lines, (unsigned long long)r + s + b);
    }
}

// k_map as a request / response machine (map_pipe.hpp): one memory round trip per iteration for all lanes of a wavefront
#ifndef MGX_MAP_PIPE_WAVES
#define MGX_MAP_PIPE_WAVES 3
#endif
#ifndef MGX_SEL_ANCHOR_MAX
#define MGX_SEL_ANCHOR_MAX 8192      // entries of the select-anchor table (32 KB of LDS per workgroup of k_map_pipe)
#endif
__shared__ uint32_t s_sel_anchor[MGX_SEL_ANCHOR_MAX];       // DevGraph::sel_anchor, one copy per workgroup
struct SelPredictLds {
    uint32_t shift;
    __device__ __forceinline__ uint32_t operator()(uint32_t r) const { return sel_predict(s_sel_anchor, shift, r); }
};
__global__ void __launch_bounds__(256, MGX_MAP_PIPE_WAVES) k_map_pipe(DevGraph g, MapArgs a, KernelStats *stats) {
    for (uint32_t j = threadIdx.x; j < g.sel_n; j += blockDim.x) s_sel_anchor[j] = g.sel_anchor[j];
    __syncthreads();
    LineCtr ctr = { 0, 0, 0 };
    MapPipe m;
    map_pipe_init(m);
    ChainClaim claim(a.cursor);
    const SelPredictLds pred = { g.sel_shift };
    for (;;) {
        const bool live = map_pipe_step(g, a, m, ctr, claim, pred);
        if (!__ballot(live)) break;
    }
    uint32_t r = ctr.rank_lines, s = ctr.select_lines, b = ctr.bit_lines;
    for (int d = 32; d >= 1; d >>= 1) { r += __shfl_xor(r, d, 64); s += __shfl_xor(s, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0 && (r | s | b)) {
        atomicAdd(&stats->rank_lines, (unsigned long long)r);
        atomicAdd(&stats->select_lines, (unsigned long long)s);
        atomicAdd(&stats->bit_lines, (unsigned long long)b);
        atomicAdd(&stats->map_lines, (unsigned long long)r + s + b);
    }
}

#include "seed_kernel.hpp"

__global__ void k_iota(uint32_t *v, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// label-aware alignment: does any dummy node (W == 0: the reference's AnnotationBuffer gives those no labels whatever their row
// says, annotation_buffer.cpp:64-68) have a label in the matrix?  Checked once per aligner; if none does — annotations are built
// from real k-mers — the kernels skip the W look-up in front of every row access.
// label-aware alignment on a CANONICAL-mode graph: node -> the representative of its k-mer (canon_repr_node), whose row holds
// the node's labels
__global__ void k_canon_repr(DevGraph g, uint32_t *out) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > g.n) return;
    out[v] = v ? canon_repr_node(g, v) : 0u;
}
__global__ void k_anno_dummy_rows(DevGraph g, const uint64_t *head, uint64_t n_rows, uint32_t *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (v > g.n || v - 1 >= n_rows || head[v - 1] == 0) return;
    LineCtr lc = { 0, 0, 0 };
    if (get_W(g, v, lc) == 0) atomicOr(flag, 1u);
}

// =================================================================================================
// host side
// =================================================================================================
static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? MGX_ERR_OOM : MGX_ERR_NO_DEVICE, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

// Device blocks of destroyed aligners, kept for the next aligner on the same device.  The reference builds one aligner per
// thread-pool task (cli/align.cpp:440-475); with hipMalloc / hipFree per handle every task paid for fresh multi-GB arenas
// (first-touch of a new 20 - 40 GB block: seconds, `profiles/r06_workers_one_device.txt`) and every hipFree synchronised the
// whole device under the other workers.  A block returns here when its aligner is destroyed (its stream has been
// synchronised by then) and is handed out best-fit; the pool is emptied when an allocation fails and by mgx_device_trim().
struct DevPool {
    enum { MAX_DEV = 16 };
    std::mutex mu;
    std::multimap<size_t, void *> blocks[MAX_DEV];
    size_t held[MAX_DEV] = { 0 };
    static int dev() { int d = 0; (void)hipGetDevice(&d); return d >= 0 && d < MAX_DEV ? d : -1; }
    void *take(size_t want, size_t *got) {
        const int d = dev();
        if (d < 0) return nullptr;
        std::lock_guard<std::mutex> lock(mu);
        auto it = blocks[d].lower_bound(want);
        if (it == blocks[d].end() || it->first > want + want / 2 + (1u << 20)) return nullptr;       // (a much larger block stays for who needs it)
        void *p = it->second;
        *got = it->first;
        held[d] -= it->first;
        blocks[d].erase(it);
        return p;
    }
    void give(void *p, size_t bytes) {
        const int d = dev();
        if (d < 0) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> lock(mu);
        blocks[d].emplace(bytes, p);
        held[d] += bytes;
    }
    size_t held_bytes() {
        const int d = dev();
        if (d < 0) return 0;
        std::lock_guard<std::mutex> lock(mu);
        return held[d];
    }
    void flush() {
        const int d = dev();
        if (d < 0) return;
        std::lock_guard<std::mutex> lock(mu);
        for (auto &e : blocks[d]) (void)hipFree(e.second);
        blocks[d].clear();
        held[d] = 0;
    }
};
static DevPool g_pool;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pooled = false;              // an aligner's buffer: comes from / returns to g_pool (the graph's own tables do not)
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        if (pooled) g_pool.give(p, bytes); else (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
    // headroom: 1/8 on top for buffers that grow with the batch; none for the arena, which is sized from the free memory.
    // (A block from the pool holds whatever its last owner left: like a fresh hipMalloc block, its contents are undefined —
    // every owner initialises what it reads, keyed on `bytes` having changed.)
    int ensure(size_t n, bool exact = false) {
        if (n <= bytes) return MGX_OK;
        release();
        size_t want = exact ? n : n + n / 8 + 256;
        if (pooled) {
            size_t got = 0;
            if (void *q = g_pool.take(want, &got)) { p = q; bytes = got; return MGX_OK; }
        }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && g_pool.held_bytes()) {      // what the pool holds is free memory: give it back and try again
            (void)hipGetLastError();
            g_pool.flush();
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) { p = nullptr; return fail(MGX_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        bytes = want;
        return MGX_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct mgx_graph {
    int device = 0;
    DevGraph g;
    DevBuf blocks, last_hint, w_hint[4], sel_anchor, firstc, terminus, valid, prefix_tbl;
    uint64_t bytes = 0;
    uint32_t mode = MGX_MODE_BASIC;
    bool primary_tables = false;      // PRIMARY: reverse-complement tables built (default; MGX_PRIMARY_TABLES=0 turns them off)
    // What label-aware aligners derive from the whole graph, computed once per graph (and annotation) instead of once per
    // aligner — the host adapters build one aligner per batch and worker thread:
    mutable std::mutex label_mu;
    mutable DevBuf canon_repr;        // CANONICAL-mode graphs: node -> the representative of its k-mer (k_canon_repr, 4 B per node)
    mutable bool canon_repr_ready = false;
    mutable std::map<uint64_t, bool> dummy_clean;   // per annotation, by its process-unique id (mgx_annotation_uid: never reused, unlike the handle's address)
};

// The pipeline run_align launches ("split8", the only one): seeding — the lane-per-read seeder, then one wavefront per read
// (k_align<PH_SEED>) on what it left —, a radix sort of the reads by predicted extension work, extension — the lane-per-read
// kernel, then 8-lane groups (8 reads per wavefront, mgx_grp.hip) or one read per wavefront on what it left.

// launches of the counted extension kernels since the library was loaded (mgx_kernel_launch_counts; bit order of MGX_KERNEL_*)
enum LaunchCounter { CNT_NONE = -1, CNT_GRP8 = 0, CNT_GRP8_PRIM, CNT_GRP8_ALT, CNT_EXT64, CNT_LANE, CNT_N };
static std::atomic<uint64_t> g_kernel_launches[CNT_N];

// The builds of the extension kernel (kernel_units.hpp).  Slot sizing and the launch read the same row.
struct ExtBuild {
    int (*launch_grp)(const void *params, uint32_t n_groups, uint32_t lds_bytes, int phase, void *stream);     // 8 reads per wavefront ...
    int (*launch_64)(const void *params, uint32_t blocks, uint32_t lds_bytes, void *stream);                   // ... or one (the other is null)
    int (*waves_per_simd)(void);
    unsigned (*static_lds)(void);
    uint64_t kernel_bit;              // MGX_KERNEL_*
    LaunchCounter counter;            // its entry of g_kernel_launches (the label-aware builds are not counted)
};
enum ExtBuildId { EXT_GRP8, EXT_GRP8_PRIM, EXT_GRP8_ALT, EXT_GRP8_LAB, EXT_EXT64, EXT_LAB64 };
static const ExtBuild g_ext_builds[] = {
    { mgx_launch_align_grp8, nullptr, mgx_grp_waves_per_simd8, mgx_grp_static_lds8, MGX_KERNEL_GRP8, CNT_GRP8 },
    { mgx_launch_align_grp8_prim, nullptr, mgx_grp_waves_per_simd8_prim, mgx_grp_static_lds8_prim, MGX_KERNEL_GRP8_PRIM, CNT_GRP8_PRIM },
    { mgx_launch_align_grp8_alt, nullptr, mgx_grp_waves_per_simd8_alt, mgx_grp_static_lds8_alt, MGX_KERNEL_GRP8_ALT, CNT_GRP8_ALT },
    { mgx_launch_align_grp8_lab, nullptr, mgx_grp_waves_per_simd8_lab, mgx_grp_static_lds8_lab, MGX_KERNEL_GRP8_LAB, CNT_NONE },
    { nullptr, mgx_launch_ext64, mgx_ext64_waves_per_simd, mgx_ext64_static_lds, MGX_KERNEL_EXT64, CNT_EXT64 },
    { nullptr, mgx_launch_lab64, mgx_lab64_waves_per_simd, mgx_lab64_static_lds, MGX_KERNEL_LAB64, CNT_NONE },
};
static uint32_t waves_per_cu(const ExtBuild &b) { return 4u * (uint32_t)b.waves_per_simd(); }
// The 8-lane-group build a configuration extends on: the label-aware one; else the one with room for alternative paths
// (either kind of graph); else, on PRIMARY graphs, the product with the CanonicalDBG branches; else the product.
static const ExtBuild &group_build(bool labeled, bool primary, uint64_t agg_cap) {
    return g_ext_builds[labeled ? EXT_GRP8_LAB : agg_cap > 1 ? EXT_GRP8_ALT : primary ? EXT_GRP8_PRIM : EXT_GRP8];
}

// Latency-critical scalar arrays go to LDS when they fit next to the other resident wavefronts of the CU.  The budget: a
// wavefront's share of the CU's 160 KB minus the kernel's static LDS and a margin (overshooting by a few bytes costs a whole
// resident wavefront per CU); the dynamic LDS per read: what its arrays want (fast_lds_bytes) or its share of the budget.
static uint32_t lds_budget(uint32_t waves_cu, uint32_t static_lds, uint32_t margin) { return (160u * 1024u) / waves_cu - static_lds - margin; }
static uint32_t lds_per_read(uint32_t Lmax, uint32_t waves_cu, uint32_t static_lds, uint32_t margin, uint32_t reads_per_wave = 1) {
    return std::min<uint32_t>(fast_lds_bytes(Lmax), lds_budget(waves_cu, static_lds, margin) / reads_per_wave) & ~15u;
}

// Environment variables: every read of the environment in this unit goes through this block.
// (a) Measurement probes — occupancy scans, LDS caps, prints, ablations that give WRONG results — are read in -DMGX_PROBES builds
// (tools/build_variant.sh) only; the product library ignores them: MGX_MAP_BYTES, MGX_DEBUG_SLOTS, MGX_ABLATE,
// MGX_EXT_GROUPS_PCT, MGX_EXT_LDS_CAP, MGX_SEED_LDS_CAP, MGX_SEED_LDS_PRINT, MGX_SEED_WAVES_PCT, MGX_HOST_TIMERS.
#ifdef MGX_PROBES
static bool probe_env_set(const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; }
static uint32_t probe_env_u32(const char *name, uint32_t dflt) { const char *e = getenv(name); return e ? (uint32_t)atoi(e) : dflt; }
static uint32_t probe_env_pct(const char *name) { const char *e = getenv(name); return e ? (uint32_t)std::min(100, std::max(1, atoi(e))) : 100u; }
#else
static inline bool probe_env_set(const char *) { return false; }
static inline uint32_t probe_env_u32(const char *, uint32_t dflt) { return dflt; }
static inline uint32_t probe_env_pct(const char *) { return 100u; }
#endif
// (b) Read by the product library too (the tools/pmc_*.sh flows and the variant builds run against it); none changes a result:
//   MGX_PREFIX_LEN_MAX=m    graph load: the suffix-range table covers at most m characters (2 .. 15)
//   MGX_PRIMARY_TABLES=0    graph load: no reverse-complement tables for a PRIMARY graph
//   MGX_LANE_HASH_MULT=f    k_lane: f times the node-table slots per lane
//   MGX_LANE_BLOCKS_PCT=p   k_lane: p % of the resident wavefronts (is the kernel bound by the latency of its own dependent
//                           accesses, or by what the memory system serves per second?)
//   MGX_LANE_TIMERS / MGX_SL_TIMERS   print the section timers of a -DMGX_LANE_TIMERS / -DMGX_SL_TIMERS build of the lane kernels
static bool env_int(const char *name, int *v) {
    const char *e = getenv(name);
    if (e) *v = atoi(e);
    return e != nullptr;
}

// The words of mgx_aligner::cursors (16 x 8 B): what the kernels count, through the pointers the host hands them.
enum CursorSlot {
    CUR_OUT = 0,              // output-stream words handed out (keeps counting past the capacity: mgx_align_batch_device)
    CUR_READ = 1,             // next work item of a persistent kernel: rewound before every launch that takes items from it
    CUR_SEED = 2,             // seeds in the seed stream (keeps counting past the capacity)
    CUR_LMAX = CUR_SEED,      // ... and, while a batch is staged, the length of its longest read (k_kmer_counts)
    CUR_RETRY = 3,            // multi-pass extension: reads listed for the next pass (CUR_OUT .. CUR_RETRY: cleared when run_align starts)
    CUR_MAP = 4,              // next chain of the mapping kernels
    CUR_LANE_BAIL = 5,        // k_lane: reads passed on to the extension kernel ...
    CUR_LANE_DONE = 6,        // ... and reads finished (the host reads the two with one copy)
    CUR_SL_BAIL = 8,          // lane-per-read seeder, first pass: reads left, listed from the front ...
    CUR_SL_DONE = 9,          // (both passes: reads seeded)
    CUR_SL_BAIL2 = 10,        // second pass: reads left for the wave-per-read seeding kernel
    CUR_SL_BAIL_BACK = 11,    // ... first pass: reads left, listed from the back
    CUR_WORDS = 16
};

// mgx_aligner::ev: the stream positions mgx_stats' times are measured between (collect_stats)
enum AlignEvent {
    EV_MAP_BEGIN, EV_MAP_END,         // run_map
    EV_ALIGN_BEGIN, EV_ALIGN_END,     // run_align, from the first seeding launch
    EV_SEEDED,                        // both seeders are through
    EV_SORTED,                        // the work sort is through: the extension starts
    EV_LANE_END,                      // the lane-per-read kernel is through (= the extension's start when it does not run)
    EV_SEED_LANE_END,                 // the lane-per-read seeder is through
    EV_COUNT
};

struct mgx_aligner {
    const mgx_graph *graph = nullptr;
    const mgx_annotation *anno = nullptr;      // label-aware alignment (mgx_labeled_aligner_create)
    bool anno_dummy_clean = false;             // no row of a dummy node holds a label (k_anno_dummy_rows)
    mgx_config cfg;
    DevConfig dcfg;
    mgx_limits user_lim;
    bool have_user_lim = false;
    DevBuf mlen_fwd, mlen_rc;     // k_map's index() match lengths, one byte per k-mer position
    DevBuf pk_fwd, pk_rc, iv_fwd, iv_rc;      // 2-bit packed reads + invalid flags of the mapping kernel (k <= 32)
    DevBuf rng_fwd, rng_rc;       // and the (rl, ru) of matches >= min_seed_length (8 B per position; optional)
    bool have_rng = false;
    DevBuf score_matrix, seqs, offsets, counts, node_begin, nodes_fwd, nodes_rc, arena, results, stream, cursors, d_stats, d_stats_map, scan_tmp, dbg_seeds;
    DevBuf seed_hdr, seed_stream, work_key, work_key_sorted, order_in, order, sort_tmp, retry_list;    // seeds from the seeding to the extension kernels, the work sort
    DevBuf resume_pool[2], retry_list2, retry_key[2];      // multi-pass extension: resume records, retry lists and keys (ping-pong)
    DevBuf lane_scratch, lane_params, lane_bail, lane_hist;           // lane-per-read kernel: per-lane scratch, its parameter block, the reads it passes on
    bool packed_valid = false;    // pk_* / iv_* hold this batch's strands (k <= 32 and the batch was mapped)
    uint32_t lane_epoch = 0;
    uint64_t lane_done = 0;
    unsigned long long lane_hist_h[32] = { 0 };
    DevBuf seedlane_scratch, seedlane_params, seedlane_bail, seedlane_hist;   // lane-per-read seeder: seed buffers, parameter block, the reads it leaves, why
    uint64_t seedlane_launched = 0;    // the last batch ran it (its counters are read back by collect_stats)
    uint32_t n_passes = 0;
    DevLimits lim;
    uint64_t n_reads = 0, total_kmers = 0;
    uint32_t n_slots = 0;
    bool keep_seeds = false;
    // host copies
    std::vector<ReadResult> h_results;
    std::vector<uint32_t> h_stream;
    HostResults host;
    HostResults host_chained;          // post_chain_alignments: `host` after chain_host.hpp
    HostResults host_retried;          // mgx_align_batch: the results with the re-aligned capacity queries in place
    bool retry_capacity = true;        // (mgx_aligner_set_pipeline "retry_capacity=0": statuses are handed to the caller)
    uint32_t label_scale = 1;          // the label arenas' multiplier (derive_limits; doubled per attempt of the capacity retry)
    const char *last_d_seqs = nullptr;           // the batch mgx_align_batch_device ran last (device pointers)
    const uint64_t *last_d_offsets = nullptr;
    // Every launch, asynchronous copy and hipcub call of this aligner goes to this stream, and its blocking copies synchronise
    // this stream only (copy_sync).  0 = the legacy default stream (what rounds 1-5 used throughout): ordered with everything
    // else the process does on blocking streams.  mgx_aligner_set_stream() gives a handle its own stream, so that the handles
    // of several worker threads on one device (cli/align.cpp:440-475: one aligner per thread-pool task) overlap instead of
    // serialising on the default stream.
    hipStream_t hstream = nullptr;
    int device = 0;                    // the graph's device
    bool own_stream = false;           // mgx_aligner_create_stream: destroyed with the aligner
    uint64_t stage_generation = 0;               // counts stage_batch calls (mgx_map_batch re-stages the same buffers) ...
    uint64_t aligned_generation = 0;             // ... and which of them mgx_align_batch_device aligned: post-chaining and the
                                                 // capacity retry read the batch back only while it is still the staged one
    std::vector<uint64_t> m_node_begin, m_fwd, m_rc;
    DevBuf ms_counts, ms_nodes, ms_sorted;       // mgx_map_summary_batch: the 12-byte records, the merged node array, the long form's scratch
    std::vector<mgx_map_counts> h_ms_counts;
    std::vector<uint64_t> h_ms_nodes;
    // the batch mgx_map_summary_batch ran last, for mgx_format_map_batch: the stage_batch call it was (0: none, or the call failed —
    // every other batch call stages again and so ends it), its reads (device pointers), map_length, longest read, and whether
    // ms_nodes holds its node array
    uint64_t ms_generation = 0;
    const char *ms_d_seqs = nullptr;
    const uint64_t *ms_d_offsets = nullptr;
    uint32_t ms_map_length = 0, ms_lmax = 0;
    bool ms_have_nodes = false;
    DevBuf mf_threshold;                         // mgx_format_map_batch: the presence threshold per k-mer count
    std::vector<uint64_t> h_mf_threshold;        // ... its host copy (the handle's: an asynchronous upload may outlive the call that failed)
    // mgx_format_tsv_batch: headers, their offsets, label names (bytes, then the n + 1 begins), line lengths, line_begin (n + 1, then
    // the capacity counter), the text, the capacity list, the host-formatted lines' (query, length) pairs
    DevBuf tf_headers, tf_header_offsets, tf_names, tf_len, tf_begin, tf_text, tf_cap, tf_patch;
    char *h_text = nullptr;                      // the text on the host: pinned memory, grown as needed
    size_t h_text_bytes = 0;
    std::vector<uint64_t> h_line_begin;
    // decode_on_device (mgx_decode_results_device, the option decode_on_device): the five count arrays and their exclusive sums
    // (RD_ARRAYS x (n + 1) words each; the first of the sums is aln_begin), the five totals, and the other six output arrays
    DevBuf rd_counts, rd_begins, rd_totals, rd_alns, rd_nodes, rd_cigar, rd_seqs, rd_status, rd_labels;
    enum { RD_H_ALN_BEGIN = 0, RD_H_ALNS, RD_H_NODES, RD_H_CIGAR, RD_H_SEQS, RD_H_STATUS, RD_H_LABELS, RD_H_N };
    void *h_rd[RD_H_N] = {};                     // the seven arrays on the host: pinned memory, grown as needed (like h_text)
    size_t h_rd_bytes[RD_H_N] = {};
    bool aligned_empty = false;                  // the last mgx_align_batch_device call had no query (it stages nothing)
    mgx_stats hstats;
    hipEvent_t ev[EV_COUNT] = {};
    uint64_t kernels_ran = 0;     // MGX_KERNEL_* bits of the extension kernels the last batch launched
    uint64_t seed_scale = 1, seed_cap = 0;
    uint64_t arena_stride = 0;
    uint64_t out_words = 0;       // capacity of `stream` for the current batch shape
    uint64_t out_min_words = 0;   // raised when a batch overflowed the heuristic size
    bool no_fast = false;         // test hook: extension through the general path only
    // Result-preserving kernel-selection switches (mgx_aligner_set_pipeline "key=value"; INTEGRATION.md "run-time switches").
    // Every combination gives the same alignments; the parity suite runs the kernels the automatic choice would not pick for
    // its small batches through them.  -1 = automatic.
    struct Options {
        int ext64 = 1;            // 0: never the 64-lane one-read-per-wavefront kernel (small batches run the 8-lane groups)
        int groups_per_wave = -1; // 0 = all 8 groups of a wavefront take reads, 1 .. 8 = that many
        int multi_pass = -1;      // multi-pass extension on / off
        int no_compact = 0, no_alias = 0, no_bt_runs = 0, no_flat = 0;
        int lane = -1;            // the lane-per-read kernel in front of the extension kernel: -1 auto, 0 off, 1 forced
        int seed_lane = -1;       // the lane-per-read seeder in front of the seeding kernel (seed_lane.hpp): -1 auto, 0 off, 1 forced
        int seed_wps = 8;         // wavefronts per SIMD of the short-read seeding kernel: 8 (64 VGPRs, spills) or 4 (102 VGPRs, tables in LDS)
        int device_share = 1;     // handles expected to run on this device at the same time (worker threads, -p N): the per-slot
                                  // arenas of this handle are sized for 1 / device_share of the machine instead of all of it
        int decode_on_device = 0; // mgx_fetch_results: the mgx_results arrays written by kernels (decode_on_device below) instead of HostResults::decode
        int map_pipe = 1;         // k_map as the request / response machine (map_pipe.hpp): 1 = for batches of >= 65536 chains, 2 = always,
                                  // 0 = never (one chain step per lane and iteration: rounds 1-4)
    } opt;
};

static unsigned long long *cursor(const mgx_aligner *A, CursorSlot s) { return A->cursors.as<unsigned long long>() + s; }
// zero the slots first .. last
static hipError_t clear_cursors(mgx_aligner *A, CursorSlot first, CursorSlot last) {
    return hipMemsetAsync(cursor(A, first), 0, (size_t)(last - first + 1) * 8, A->hstream);
}

extern "C" {

int mgx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char *mgx_last_error(void) { return g_err.c_str(); }
// the other translation units of libmgx.so (mgx_annot.hip) report through the same thread-local message
extern "C" void mgx_set_last_error(const char *msg) { g_err = msg ? msg : ""; }
uint32_t mgx_abi_version(void) { return MGX_ABI_VERSION; }

void mgx_config_init_default(mgx_config *c) {
    memset(c, 0, sizeof(*c));
    c->num_alternative_paths = 1;
    c->max_num_seeds_per_locus = UINT64_MAX;
    c->min_cell_score = INT32_MIN + 100;
    c->min_path_score = 0;
    c->xdrop = INT32_MAX;
    c->max_nodes_per_seq_char = 1.7976931348623157e308;
    c->max_ram_per_alignment = 1.7976931348623157e308;
    c->gap_opening_penalty = -5;
    c->gap_extension_penalty = -2;
    c->forward_and_reverse_complement = 1;
    c->global_xdrop = 1;
    c->allow_left_trim = 1;
    c->seed_complexity_filter = 1;
}

void mgx_config_set_dna_matrix(mgx_config *c, int8_t match, int8_t mm_transition, int8_t mm_transversion) {
    for (int i = 0; i < 128; ++i)
        for (int j = 0; j < 128; ++j) c->score_matrix[i][j] = mm_transversion;
    c->score_matrix['A']['G'] = c->score_matrix['G']['A'] = mm_transition;
    c->score_matrix['C']['T'] = c->score_matrix['T']['C'] = mm_transition;
    c->score_matrix['A']['A'] = c->score_matrix['C']['C'] = c->score_matrix['G']['G'] = c->score_matrix['T']['T'] = match;
}

void mgx_config_set_unit_matrix(mgx_config *c, int8_t match) {
    for (int i = 0; i < 128; ++i)
        for (int j = 0; j < 128; ++j) c->score_matrix[i][j] = (int8_t)-match;
    c->score_matrix['A']['A'] = c->score_matrix['C']['C'] = c->score_matrix['G']['G'] = c->score_matrix['T']['T'] = match;
}

void mgx_config_set_scoring_matrix(mgx_config *c) {
    if (c->alignment_edit_distance) {
        mgx_config_set_unit_matrix(c, 1);
        c->left_end_bonus = 0;
        c->right_end_bonus = 0;
    } else {
        mgx_config_set_dna_matrix(c, c->alignment_match_score, (int8_t)-c->alignment_mm_transition_score,
                                  (int8_t)-c->alignment_mm_transversion_score);
    }
}

void mgx_config_init_cli(mgx_config *c, uint32_t k) {
    mgx_config_init_default(c);
    c->min_seed_length = std::min<uint64_t>(19, k);
    c->max_seed_length = UINT64_MAX;
    c->max_num_seeds_per_locus = 1000;
    c->xdrop = 27;
    c->min_exact_match = 0.7;
    c->max_nodes_per_seq_char = 5.0;
    c->max_ram_per_alignment = 200.0;
    c->rel_score_cutoff = 0.95;
    c->gap_opening_penalty = -6;
    c->gap_extension_penalty = -2;
    c->left_end_bonus = 5;
    c->right_end_bonus = 5;
    c->alignment_edit_distance = 0;            /* cli/config/config.hpp:117-120 */
    c->alignment_match_score = 2;
    c->alignment_mm_transition_score = 3;
    c->alignment_mm_transversion_score = 3;
    mgx_config_set_scoring_matrix(c);
}

void mgx_limits_init_default(mgx_limits *l, uint32_t max_query_length) {
    memset(l, 0, sizeof(*l));
    l->max_query_length = max_query_length;      // the rest: 0 = derive from the config at batch time
}

// ------------------------------------------------------------------------------------------------
// graph
// ------------------------------------------------------------------------------------------------
int mgx_graph_create(const mgx_boss_view *view, int device, mgx_graph **out) {
    if (!view || !out || !view->W || !view->last || !view->F) return fail(MGX_ERR_INVALID, "null BOSS view");
    if (view->sigma != SIGMA) return fail(MGX_ERR_UNSUPPORTED, "only the DNA alphabet $ACGT (sigma = 5) is implemented");
    // CANONICAL: a DBGSuccinct that stores both strands (same index, different aligner flow).  PRIMARY: one k-mer of every
    // pair is stored and the reference aligns through the CanonicalDBG wrapper (dbg_aligner.cpp:52-53) — canon_graph.hpp.
    if (view->mode != MGX_MODE_BASIC && view->mode != MGX_MODE_CANONICAL && view->mode != MGX_MODE_PRIMARY)
        return fail(MGX_ERR_INVALID, "unknown graph mode %u", view->mode);
    if (view->k < 2 || view->k > 255) return fail(MGX_ERR_INVALID, "k out of range");
    if (view->n_edges == 0 || view->n_edges >= 0xFFFFFFF0ull) return fail(MGX_ERR_UNSUPPORTED, "edge count must fit 32 bits");
    if (view->mode == MGX_MODE_PRIMARY) {
        if (view->k > 64) return fail(MGX_ERR_UNSUPPORTED, "PRIMARY-mode graphs need k <= 64 (the load-time kernels hold node spellings in registers)");
        if (view->n_edges * 2 >= 0xFFFFFFF0ull) return fail(MGX_ERR_UNSUPPORTED, "PRIMARY mode: ids of both strands must fit 32 bits");
    }
    if (mgx_device_count() <= device) return fail(MGX_ERR_NO_DEVICE, "HIP device %d not available", device);
    HIP_TRY(hipSetDevice(device));
    auto *G = new mgx_graph();
    std::unique_ptr<mgx_graph> guard(G);
    G->device = device;
    G->mode = view->mode;
    const uint64_t n = view->n_edges;
    const uint32_t n_blocks = (uint32_t)((n + 1 + 63) / 64);
    DevBuf dW, dLast, dValid, counts, cum;
    const uint8_t *W = view->W, *last = view->last;
    if (!view->on_device) {
        if (int rc = dW.ensure(n + 1)) return rc;
        if (int rc = dLast.ensure(n + 1)) return rc;
        HIP_TRY(hipMemcpy(dW.p, view->W, n + 1, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dLast.p, view->last, n + 1, hipMemcpyHostToDevice));
        W = dW.as<uint8_t>();
        last = dLast.as<uint8_t>();
    }
    if (int rc = G->blocks.ensure((size_t)n_blocks * sizeof(Block))) return rc;
    if (int rc = counts.ensure((size_t)n_blocks * 6 * 4)) return rc;
    k_build_pass1<<<(n_blocks + 255) / 256, 256>>>(W, last, n, G->blocks.as<Block>(), counts.as<uint32_t>(), n_blocks);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> hc((size_t)n_blocks * 6);
    HIP_TRY(hipMemcpy(hc.data(), counts.p, hc.size() * 4, hipMemcpyDeviceToHost));
    uint64_t tot[6] = { 0, 0, 0, 0, 0, 0 };
    for (uint32_t b = 0; b < n_blocks; ++b)
        for (int c = 0; c < 6; ++c) { uint32_t v = hc[(size_t)b * 6 + c]; hc[(size_t)b * 6 + c] = (uint32_t)tot[c]; tot[c] += v; }
    if (int rc = cum.ensure(hc.size() * 4)) return rc;
    HIP_TRY(hipMemcpy(cum.p, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
    HintPtrs hp;
    if (int rc = G->last_hint.ensure((tot[5] / 64 + 2) * 4)) return rc;
    hp.last_hint = G->last_hint.as<uint32_t>();
    for (int c = 0; c < 4; ++c) {
        if (int rc = G->w_hint[c].ensure((tot[c + 1] / 64 + 2) * 4)) return rc;
        hp.w_hint[c] = G->w_hint[c].as<uint32_t>();
    }
    k_build_pass2<<<(n_blocks + 255) / 256, 256>>>(G->blocks.as<Block>(), cum.as<uint32_t>(), hp, n_blocks);
    HIP_TRY(hipGetLastError());

    DevGraph &g = G->g;
    memset(&g, 0, sizeof(g));
    g.blocks = G->blocks.as<Block>();
    g.last_hint = hp.last_hint;
    for (int c = 0; c < 4; ++c) g.w_hint[c] = hp.w_hint[c];
    g.n = n;
    g.n_blocks = n_blocks;
    g.k = view->k;
    for (int c = 0; c < SIGMA; ++c) {
        if (view->F[c] > n) return fail(MGX_ERR_INVALID, "F[%d] out of range", c);
        g.F[c] = (uint32_t)view->F[c];
    }
    // NF[c] = rank_last(F[c]) (boss.cpp:1095-1101)
    {
        std::vector<Block> hb(1);
        for (int c = 0; c < SIGMA; ++c) {
            uint64_t i = g.F[c];
            if (i == 0) { g.NF[c] = 0; continue; }
            HIP_TRY(hipMemcpy(hb.data(), g.blocks + (i >> 6), sizeof(Block), hipMemcpyDeviceToHost));
            uint64_t m = hb[0].last_bits & ((i & 63) == 63 ? ~0ull : ((1ull << ((i & 63) + 1)) - 1));
            g.NF[c] = hb[0].last_cum + (uint32_t)__builtin_popcountll(m);
        }
    }
    {
        g.sel_shift = sel_anchor_shift(tot[5], MGX_SEL_ANCHOR_MAX);
        g.sel_n = (uint32_t)(tot[5] >> g.sel_shift) + 2;
        if (int rc = G->sel_anchor.ensure((size_t)g.sel_n * 4)) return rc;
        k_sel_anchor<<<(g.sel_n + 255) / 256, 256>>>(g, g.sel_shift, g.sel_n, (uint32_t)tot[5], G->sel_anchor.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        g.sel_anchor = G->sel_anchor.as<uint32_t>();
    }
    // node mask
    if (view->valid) {
        const uint8_t *valid = view->valid;
        if (!view->on_device) {
            if (int rc = dValid.ensure(n + 1)) return rc;
            HIP_TRY(hipMemcpy(dValid.p, view->valid, n + 1, hipMemcpyHostToDevice));
            valid = dValid.as<uint8_t>();
        }
        if (int rc = G->valid.ensure((size_t)n_blocks * 8)) return rc;
        k_pack_valid<<<(n_blocks + 255) / 256, 256>>>(valid, G->valid.as<uint64_t>(), n);
        HIP_TRY(hipGetLastError());
        g.valid = G->valid.as<uint64_t>();
    }
    // first characters: k - 2 rounds of D[e] <- D[bwd(e)]
    {
        DevBuf P, D0, D1;
        if (int rc = P.ensure((n + 1) * 4)) return rc;
        if (int rc = D0.ensure(n + 1)) return rc;
        if (int rc = D1.ensure(n + 1)) return rc;
        uint32_t nb = (uint32_t)((n + 1 + 255) / 256);
        k_parent<<<nb, 256>>>(g, P.as<uint32_t>(), D0.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        uint8_t *din = D0.as<uint8_t>(), *dout = D1.as<uint8_t>();
        // suffix-range table over the last m node characters, accumulated during the same rounds
        // the longest table whose 8 B x 4^m fit a sixteenth of the free HBM (m = 15: 8.6 GB, 14: 2.1 GB, 13: 0.5 GB)
        uint32_t cap_m = 12;
        {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            while (cap_m < 15 && (8ull << (2 * (cap_m + 1))) <= free_b / 16) ++cap_m;
        }
        if (int e; env_int("MGX_PREFIX_LEN_MAX", &e)) cap_m = (uint32_t)std::min(15, std::max(2, e));
        const uint32_t m = choose_prefix_len(n, g.k, cap_m);
        DevBuf key;
        if (int rc = key.ensure((n + 1) * 4)) return rc;
        const uint64_t entries = 1ull << (2 * m);
        if (int rc = G->prefix_tbl.ensure(entries * sizeof(uint2))) return rc;
        k_prefix_init<<<(uint32_t)((entries + 255) / 256), 256>>>(G->prefix_tbl.as<uint2>(), entries);
        k_key_step<<<nb, 256>>>(din, key.as<uint32_t>(), n, m, 0);
        for (uint32_t r = 0; r + 2 < g.k; ++r) {
            k_gather<<<nb, 256>>>(P.as<uint32_t>(), din, dout, n);
            std::swap(din, dout);
            if (r + 1 < m) k_key_step<<<nb, 256>>>(din, key.as<uint32_t>(), n, m, r + 1);
        }
        HIP_TRY(hipGetLastError());
        k_prefix_fill<<<nb, 256>>>(key.as<uint32_t>(), n, G->prefix_tbl.as<uint2>());
        HIP_TRY(hipGetLastError());
        g.prefix_tbl = G->prefix_tbl.as<uint2>();
        g.prefix_len = m;
        if (int rc = G->firstc.ensure(((n + 1 + 7) / 8) * 4 + 4)) return rc;
        k_pack_firstc<<<(uint32_t)(((n + 8) / 8 + 255) / 256), 256>>>(din, G->firstc.as<uint32_t>(), n);
        HIP_TRY(hipGetLastError());
        g.firstc = G->firstc.as<uint32_t>();
        HIP_TRY(hipDeviceSynchronize());
    }
    // MEM terminus bits
    // (PRIMARY graphs: terminus | terminus of the ids v + n | palindrome bits | rc_node table — canon_graph.hpp primary_tables().
    // MGX_PRIMARY_TABLES=0 leaves the last two out (4 bytes per BOSS node less) and the wrapper re-derives spellings and look-ups
    // per expansion: same results, ~7x the random lines)
    int primary_tables = 1;
    env_int("MGX_PRIMARY_TABLES", &primary_tables);
    G->primary_tables = G->mode == MGX_MODE_PRIMARY && primary_tables != 0;
    const size_t terminus_bytes = G->mode != MGX_MODE_PRIMARY ? (size_t)n_blocks * 8
                                  : (size_t)n_blocks * 8 * 3 + (G->primary_tables ? (size_t)(tot[5] + 2) * 4 : 0);
    if (int rc = G->terminus.ensure(terminus_bytes, true)) return rc;
    if (G->mode == MGX_MODE_PRIMARY) HIP_TRY(hipMemset(G->terminus.p, 0, terminus_bytes));
    g.terminus = G->terminus.as<uint64_t>();
    if (G->mode == MGX_MODE_PRIMARY) {
        k_terminus_primary<<<n_blocks, 64>>>(g, G->terminus.as<uint64_t>(), G->terminus.as<uint64_t>() + n_blocks);
        if (G->primary_tables)
            k_primary_tables<<<n_blocks, 64>>>(g, G->terminus.as<uint64_t>() + 2ull * n_blocks,
                                               reinterpret_cast<uint32_t *>(G->terminus.as<uint64_t>() + 3ull * n_blocks));
    } else {
        k_terminus<<<n_blocks, 64>>>(g, G->terminus.as<uint64_t>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    G->bytes = G->blocks.bytes + G->last_hint.bytes + G->sel_anchor.bytes + G->firstc.bytes + G->terminus.bytes + G->valid.bytes
               + G->prefix_tbl.bytes;
    for (int c = 0; c < 4; ++c) G->bytes += G->w_hint[c].bytes;
    *out = guard.release();
    return MGX_OK;
}

void mgx_graph_destroy(mgx_graph *g) { delete g; }
uint32_t mgx_graph_k(const mgx_graph *g) { return g->g.k; }
uint64_t mgx_graph_max_index(const mgx_graph *g) {
    return g->mode == MGX_MODE_PRIMARY ? 2 * g->g.n : g->g.n;            // CanonicalDBG::max_index (canonical_dbg.hpp:96)
}
uint64_t mgx_graph_device_bytes(const mgx_graph *g) { return g->bytes; }
uint64_t mgx_graph_num_edges(const mgx_graph *g) { return g->g.n; }
uint32_t mgx_graph_mode(const mgx_graph *g) { return g->mode; }

// ------------------------------------------------------------------------------------------------
// aligner
// ------------------------------------------------------------------------------------------------
static int aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *anno,
                          mgx_aligner **out) {
    if (!g || !config || !out) return fail(MGX_ERR_INVALID, "null argument");
    auto *A = new mgx_aligner();
    std::unique_ptr<mgx_aligner> guard(A);
    A->graph = g;
    A->anno = anno;
    A->device = g->device;
    // every device buffer of an aligner goes through the per-device block pool (DevPool): the next aligner takes them over
    for (DevBuf *b : { &A->mlen_fwd, &A->mlen_rc, &A->pk_fwd, &A->pk_rc, &A->iv_fwd, &A->iv_rc, &A->rng_fwd, &A->rng_rc, &A->score_matrix,
                       &A->seqs, &A->offsets, &A->counts, &A->node_begin, &A->nodes_fwd, &A->nodes_rc, &A->arena, &A->results, &A->stream,
                       &A->cursors, &A->d_stats, &A->d_stats_map, &A->scan_tmp, &A->dbg_seeds, &A->seed_hdr, &A->seed_stream, &A->work_key,
                       &A->work_key_sorted, &A->order_in, &A->order, &A->sort_tmp, &A->retry_list, &A->resume_pool[0], &A->resume_pool[1],
                       &A->retry_list2, &A->retry_key[0], &A->retry_key[1], &A->lane_scratch, &A->lane_params, &A->lane_bail, &A->lane_hist, &A->seedlane_scratch, &A->seedlane_params,
                       &A->seedlane_bail, &A->seedlane_hist, &A->ms_counts, &A->ms_nodes, &A->ms_sorted, &A->mf_threshold, &A->tf_headers, &A->tf_header_offsets,
                       &A->tf_names, &A->tf_len, &A->tf_begin, &A->tf_text, &A->tf_cap, &A->tf_patch, &A->rd_counts, &A->rd_begins, &A->rd_totals, &A->rd_alns,
                       &A->rd_nodes, &A->rd_cigar, &A->rd_seqs, &A->rd_status, &A->rd_labels })
        b->pooled = true;
    {
        std::string err;
        int rc = prepare_config(*config, g->g.k, &A->cfg, &A->dcfg, &err, anno != nullptr);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    if (anno) {
        // LabeledAligner<>(graph, config, annotator) (aligner_labeled.hpp:125-127).  On the device: BASIC-, PRIMARY- and
        // CANONICAL-mode graphs (labels looked up by base node through the CanonicalDBG wrapper, resp. by the k-mer's
        // representative: include/mgx.h), annotation without coordinates, as many alternative paths per label as the
        // labeled kernel build holds.
        if (A->cfg.num_alternative_paths > (uint64_t)std::min(mgx_lab64_max_alt(), mgx_grp_max_alt8_lab()))
            return fail(MGX_ERR_UNSUPPORTED, "label-aware alignment: num_alternative_paths <= %d on the device", std::min(mgx_lab64_max_alt(), mgx_grp_max_alt8_lab()));
        int adev = 0; uint64_t arows = 0; const uint64_t *h; const uint32_t *c, *m;
        mgx_annotation_device_view(anno, &adev, &arows, &h, &c, &m);
        if (adev != g->device) return fail(MGX_ERR_INVALID, "the annotation lives on device %d, the graph on device %d", adev, g->device);
        // An annotation with coordinates makes LabeledAligner chain seeds (aligner_labeled.cpp:457-462: chain_alignments on, global
        // x-drop off).  Of that mode the device has the annotation (mgx_annotation_get_row_tuples) and the chaining DP
        // (mgx_chain_seeds); the extension between chain seeds (dbg_aligner.cpp:155-250,388-529) is not built: refused, so that
        // the caller keeps the reference's aligner — never answered with the plain label-aware mode
        if (mgx_annotation_has_coordinates(anno) && g->mode == MGX_MODE_BASIC)
            return fail(MGX_ERR_UNSUPPORTED, "label-aware alignment with coordinates (seed chaining) is not on the device");
        if (arows < g->g.n) return fail(MGX_ERR_INVALID, "the annotation has %llu rows, the graph %llu nodes (row = node - 1)",
                                        (unsigned long long)arows, (unsigned long long)g->g.n);
    }
    if (g->mode == MGX_MODE_CANONICAL) { A->dcfg.canonical = 1; A->dcfg.fwd_and_rc = 1; }     // dbg_aligner.cpp:225-226
    if (g->mode == MGX_MODE_PRIMARY) { A->dcfg.canonical = g->primary_tables ? 3 : 2; A->dcfg.fwd_and_rc = 1; }   // through the wrapper
    mgx_config &c = A->cfg;
    if (limits) { A->user_lim = *limits; A->have_user_lim = true; }
    HIP_TRY(hipSetDevice(g->device));
    if (anno) {
        int adev = 0; uint64_t arows = 0; const uint64_t *h; const uint32_t *c, *m;
        mgx_annotation_device_view(anno, &adev, &arows, &h, &c, &m);
        std::lock_guard<std::mutex> lock(g->label_mu);
        const uint64_t key = mgx_annotation_uid(anno);
        auto it = g->dummy_clean.find(key);
        if (it == g->dummy_clean.end()) {
            uint32_t *d_flag = nullptr, flag = 1;
            HIP_TRY(hipMalloc(&d_flag, 4));
            HIP_TRY(hipMemset(d_flag, 0, 4));
            if (g->g.n) k_anno_dummy_rows<<<(uint32_t)((g->g.n + 255) / 256), 256>>>(g->g, h, arows, d_flag);
            HIP_TRY(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
            (void)hipFree(d_flag);
            it = g->dummy_clean.emplace(key, flag == 0).first;
        }
        A->anno_dummy_clean = it->second;
        if (g->mode == MGX_MODE_CANONICAL && !g->canon_repr_ready) {
            if (int rc = g->canon_repr.ensure((g->g.n + 1) * 4)) return rc;
            k_canon_repr<<<(uint32_t)((g->g.n + 256) / 256), 256>>>(g->g, g->canon_repr.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
            g->canon_repr_ready = true;
        }
    }
    if (int rc = A->score_matrix.ensure(128 * 128)) return rc;
    HIP_TRY(hipMemcpy(A->score_matrix.p, c.score_matrix, 128 * 128, hipMemcpyHostToDevice));
    if (int rc = A->cursors.ensure(CUR_WORDS * 8)) return rc;
    if (int rc = A->d_stats.ensure(sizeof(KernelStats))) return rc;
    if (int rc = A->d_stats_map.ensure(sizeof(KernelStats))) return rc;
    for (auto &e : A->ev) HIP_TRY(hipEventCreate(&e));
    memset(&A->hstats, 0, sizeof(A->hstats));
    memset(&A->lim, 0, sizeof(A->lim));
    *out = guard.release();
    return MGX_OK;
}
int mgx_aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, mgx_aligner **out) {
    return aligner_create(g, config, limits, nullptr, out);
}
int mgx_labeled_aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *annotation,
                               mgx_aligner **out) {
    if (!annotation) return fail(MGX_ERR_INVALID, "null argument");
    return aligner_create(g, config, limits, annotation, out);
}

void mgx_aligner_destroy(mgx_aligner *a) {
    if (!a) return;
    (void)hipSetDevice(a->device);                          // (its own copy: the graph may be gone by now — a binding's GC order)
    (void)hipStreamSynchronize(a->hstream);
    for (auto &e : a->ev) if (e) (void)hipEventDestroy(e);
    if (a->h_text) (void)hipHostFree(a->h_text);
    for (void *p : a->h_rd) if (p) (void)hipHostFree(p);
    if (a->own_stream) (void)hipStreamDestroy(a->hstream);
    delete a;
}

int mgx_aligner_get_config(const mgx_aligner *a, mgx_config *out) { *out = a->cfg; return MGX_OK; }

int mgx_aligner_get_limits(const mgx_aligner *a, mgx_limits *out) {
    if (!a || !out) return fail(MGX_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    out->max_query_length = a->lim.Lmax;
    out->max_columns = a->lim.max_columns;
    out->max_seeds = a->lim.max_seeds;
    out->cell_arena_bytes = (uint64_t)a->lim.cell_words * 4;
    return MGX_OK;
}

// a blocking copy that synchronises the aligner's stream only (hipMemcpy would synchronise the whole device's default stream)
static hipError_t copy_sync(mgx_aligner *A, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, A->hstream)) return e;
    return hipStreamSynchronize(A->hstream);
}

// stage inputs, compute k-mer slot offsets and Lmax on the device
// (window: the characters per node slot — the graph's k, or mgx_map_summary_batch's map_length < k)
static int stage_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device,
                       const char **d_seqs, const uint64_t **d_offsets, uint32_t *Lmax_out, uint32_t window = 0) {
    const uint32_t k = window ? window : A->graph->g.k;
    ++A->stage_generation;
    if (on_device) {
        *d_seqs = seqs;
        *d_offsets = offsets;
    } else {
        uint64_t total = offsets[n];
        if (int rc = A->seqs.ensure(total + 16)) return rc;
        if (int rc = A->offsets.ensure((n + 1) * 8)) return rc;
        HIP_TRY(hipMemcpyAsync(A->seqs.p, seqs, total, hipMemcpyHostToDevice, A->hstream));
        HIP_TRY(hipMemcpyAsync(A->offsets.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, A->hstream));
        *d_seqs = A->seqs.as<char>();
        *d_offsets = A->offsets.as<uint64_t>();
    }
    if (int rc = A->counts.ensure((n + 2) * 8)) return rc;
    if (int rc = A->node_begin.ensure((n + 2) * 8)) return rc;
    HIP_TRY(hipMemsetAsync(A->cursors.p, 0, CUR_WORDS * 8, A->hstream));
    k_kmer_counts<<<(uint32_t)((n + 1 + 255) / 256), 256, 0, A->hstream>>>(*d_offsets, n, k, A->counts.as<uint64_t>(), cursor(A, CUR_LMAX));
    HIP_TRY(hipGetLastError());
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, A->counts.as<uint64_t>(), A->node_begin.as<uint64_t>(), (int)(n + 1), A->hstream));
    if (int rc = A->scan_tmp.ensure(tmp_bytes + 16)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A->scan_tmp.p, tmp_bytes, A->counts.as<uint64_t>(), A->node_begin.as<uint64_t>(), (int)(n + 1), A->hstream));
    uint64_t total_kmers = 0;
    unsigned long long lmax = 0;
    HIP_TRY(copy_sync(A, &total_kmers, A->node_begin.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
    HIP_TRY(copy_sync(A, &lmax, cursor(A, CUR_LMAX), 8, hipMemcpyDeviceToHost));
    A->total_kmers = total_kmers;
    A->n_reads = n;
    *Lmax_out = (uint32_t)lmax;
    if (int rc = A->nodes_fwd.ensure((total_kmers + 1) * 4)) return rc;
    if (int rc = A->nodes_rc.ensure((total_kmers + 1) * 4)) return rc;
    if (int rc = A->mlen_fwd.ensure(total_kmers + 1)) return rc;
    if (int rc = A->mlen_rc.ensure(total_kmers + 1)) return rc;
    {
        // the range arrays are an optimisation: only when they fit comfortably next to everything else
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        free_b += g_pool.held_bytes();
        const size_t need = 2 * (total_kmers + 1) * sizeof(uint2);
        A->have_rng = need <= A->rng_fwd.bytes + A->rng_rc.bytes || need < free_b / 4;
        if (A->have_rng) {
            if (int rc = A->rng_fwd.ensure((total_kmers + 1) * sizeof(uint2))) return rc;
            if (int rc = A->rng_rc.ensure((total_kmers + 1) * sizeof(uint2))) return rc;
        }
    }
    return MGX_OK;
}

// raw_edges: BOSS::map_to_edges, the node mask not applied (mgx_map_summary_batch on CANONICAL graphs applies it after the minimum)
static int run_map(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, bool do_rc, bool mapped, uint32_t Lmax,
                   bool raw_edges = false) {
    DevGraph dg = A->graph->g;
    if (raw_edges) dg.valid = nullptr;
    // k_map's counters live in their own block: a re-run of the alignment stage (stream overflow) resets only its own
    HIP_TRY(hipMemsetAsync(A->d_stats_map.p, 0, sizeof(KernelStats), A->hstream));
    HIP_TRY(hipMemsetAsync(A->d_stats.p, 0, sizeof(KernelStats), A->hstream));
    A->packed_valid = false;
    if (!mapped) {
        // max_seed_length < k: nodes are not mapped (dbg_aligner.cpp:209-213)
        HIP_TRY(hipMemsetAsync(A->nodes_fwd.p, 0, (A->total_kmers + 1) * 4, A->hstream));
        HIP_TRY(hipMemsetAsync(A->nodes_rc.p, 0, (A->total_kmers + 1) * 4, A->hstream));
        HIP_TRY(hipMemsetAsync(A->mlen_fwd.p, 0xFF, A->total_kmers + 1, A->hstream));
        HIP_TRY(hipMemsetAsync(A->mlen_rc.p, 0xFF, A->total_kmers + 1, A->hstream));
        return MGX_OK;
    }
    unsigned long long *map_cursor = cursor(A, CUR_MAP);
    HIP_TRY(clear_cursors(A, CUR_MAP, CUR_MAP));
    HIP_TRY(hipMemsetAsync(A->mlen_fwd.p, 0xFF, A->total_kmers + 1, A->hstream));       // MLEN_UNKNOWN
    if (do_rc) HIP_TRY(hipMemsetAsync(A->mlen_rc.p, 0xFF, A->total_kmers + 1, A->hstream));
    HIP_TRY(hipEventRecord(A->ev[EV_MAP_BEGIN], A->hstream));
    {
        // persistent lanes: enough wavefronts to fill the device, never more lanes than chains
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, A->graph->device));
        const uint64_t chains = (do_rc ? 2 : 1) * n;
        uint64_t blocks = std::min<uint64_t>((uint64_t)prop.multiProcessorCount * MGX_MAP_BLOCKS_PER_CU, (chains + 255) / 256);
        if (blocks == 0) blocks = 1;
        const bool no_pack = probe_env_set("MGX_MAP_BYTES");          // A/B probe: the byte-per-character path
        if (A->graph->g.k <= 32 && Lmax > 0 && !no_pack) {
            // words: every read starts at (offset >> 5) + read and takes ceil(L / 32) of them
            const uint64_t words = ((A->total_kmers + n * (uint64_t)A->graph->g.k) >> 5) + n + 2;
            if (int rc = A->pk_fwd.ensure(words * 8)) return rc;
            if (int rc = A->iv_fwd.ensure(words * 4)) return rc;
            if (do_rc) { if (int rc = A->pk_rc.ensure(words * 8)) return rc; if (int rc = A->iv_rc.ensure(words * 4)) return rc; }
            const uint32_t wpr = (Lmax + 31) / 32;
            const uint64_t threads = n * wpr;
            k_pack_reads<<<(uint32_t)((threads + 255) / 256), 256, 0, A->hstream>>>(d_seqs, d_offsets, n, wpr, do_rc ? 1 : 0, A->pk_fwd.as<uint64_t>(),
                                                                    A->pk_rc.as<uint64_t>(), A->iv_fwd.as<uint32_t>(), A->iv_rc.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            A->packed_valid = true;
            // (a batch of few chains — config 0: 1000 long queries — leaves most lanes of either kernel idle; there the one-step-
            // per-lane machine's single iteration per k-mer beats the pipe's 2.4: 30 vs 46 ms, profiles/r05_config0_*.json)
            if (A->opt.map_pipe == 1 ? chains >= 65536 : A->opt.map_pipe > 1) {
                MapArgs ma;
                ma.offsets = d_offsets; ma.node_begin = A->node_begin.as<uint64_t>();
                ma.pk_fwd = A->pk_fwd.as<uint64_t>(); ma.pk_rc = A->pk_rc.as<uint64_t>();
                ma.iv_fwd = A->iv_fwd.as<uint32_t>(); ma.iv_rc = A->iv_rc.as<uint32_t>();
                ma.nodes_fwd = A->nodes_fwd.as<uint32_t>(); ma.nodes_rc = A->nodes_rc.as<uint32_t>();
                ma.mlen_fwd = A->mlen_fwd.as<uint8_t>(); ma.mlen_rc = A->mlen_rc.as<uint8_t>();
                ma.rng_fwd = A->have_rng ? A->rng_fwd.as<uint2>() : nullptr; ma.rng_rc = A->have_rng ? A->rng_rc.as<uint2>() : nullptr;
                ma.min_rng_len = (int32_t)std::min<uint64_t>(A->cfg.min_seed_length, 1u << 20);
                ma.n_reads = n; ma.do_rc = do_rc ? 1 : 0; ma.cursor = map_cursor;
                const uint64_t pblocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)prop.multiProcessorCount * MGX_MAP_PIPE_WAVES, (chains + 255) / 256));
                k_map_pipe<<<(uint32_t)pblocks, 256, 0, A->hstream>>>(dg, ma, A->d_stats_map.as<KernelStats>());
            } else
            k_map_packed<<<(uint32_t)blocks, 256, 0, A->hstream>>>(dg, d_offsets, A->node_begin.as<uint64_t>(),
                                         A->pk_fwd.as<uint64_t>(), A->pk_rc.as<uint64_t>(), A->iv_fwd.as<uint32_t>(), A->iv_rc.as<uint32_t>(),
                                         A->nodes_fwd.as<uint32_t>(), A->nodes_rc.as<uint32_t>(),
                                         A->mlen_fwd.as<uint8_t>(), A->mlen_rc.as<uint8_t>(),
                                         A->have_rng ? A->rng_fwd.as<uint2>() : nullptr, A->have_rng ? A->rng_rc.as<uint2>() : nullptr,
                                         (int)std::min<uint64_t>(A->cfg.min_seed_length, 1u << 20), n, do_rc ? 1 : 0,
                                         map_cursor, A->d_stats_map.as<KernelStats>());
        } else {
            k_map<<<(uint32_t)blocks, 256, 0, A->hstream>>>(dg, d_seqs, d_offsets, A->node_begin.as<uint64_t>(),
                                         A->nodes_fwd.as<uint32_t>(), A->nodes_rc.as<uint32_t>(),
                                         A->mlen_fwd.as<uint8_t>(), A->mlen_rc.as<uint8_t>(),
                                         A->have_rng ? A->rng_fwd.as<uint2>() : nullptr, A->have_rng ? A->rng_rc.as<uint2>() : nullptr,
                                         (int)std::min<uint64_t>(A->cfg.min_seed_length, 1u << 20), n, do_rc ? 1 : 0,
                                         map_cursor, A->d_stats_map.as<KernelStats>());
        }
    }
    HIP_TRY(hipGetLastError());
    if (A->graph->mode == MGX_MODE_PRIMARY && do_rc && n) {
        k_canon_merge<<<(uint32_t)std::min<uint64_t>((n + 3) / 4, 65536), 256, 0, A->hstream>>>(dg, d_seqs, d_offsets, A->node_begin.as<uint64_t>(),
                                                                             A->nodes_fwd.as<uint32_t>(), A->nodes_rc.as<uint32_t>(), n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(A->ev[EV_MAP_END], A->hstream));
    return MGX_OK;
}

// bits of the work-sort key: 12 of predicted work + the segment number (align_core.hpp, WORK_SEGMENT_SHIFT)
static int work_key_bits(uint64_t n) {
    int b = 12;
    for (uint64_t seg = n ? (n - 1) >> WORK_SEGMENT_SHIFT : 0; seg; seg >>= 1) ++b;
    return std::min(b, 32);
}

// ------------------------------------------------------------------------------------------------
// run_align: one staged and mapped batch through seeding, the work sort and extension
// ------------------------------------------------------------------------------------------------
// What the stages of run_align hand to one another (the limits of the batch are A->lim).
struct AlignPlan {
    uint64_t n = 0;                   // reads
    bool labeled = false;
    uint32_t cus = 0;                 // compute units of the device
    bool lane_ok = false;             // the lane-per-read kernel takes this batch's configuration (and got its scratch)
    uint32_t lane_blocks = 0;         // its resident wavefronts
    LaneParams LP;
    uint64_t agg_cap = 1;             // alignments kept per query
    const ExtBuild *grp = nullptr;    // the 8-lane-group build the configuration extends on (group_build)
    uint64_t wave_slots = 0;          // resident wavefronts of the seeding kernel (one per read)
    uint64_t stride = 0, slots = 0;   // the arena: bytes per slice, slices
    size_t sort_tmp_bytes = 0;
    AlignParams P;
};

// The lane-per-read kernel (mgx_lane.hip) in front of the group kernel: does this batch's configuration qualify?  Its scratch
// is taken before the arena is sized from what is free.
static int plan_lane(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    LaneParams &LP = pl.LP;
    memset(&LP, 0, sizeof(LP));
    std::string lane_why;
    pl.lane_blocks = pl.cus * 4u * (uint32_t)mgx_lane_waves_per_simd();
    // (label-aware batches, round 6: the lane takes the reads whose seeds and columns all carry one and the same single label —
    // lane_read.hpp; it needs the annotation's "no dummy node's row holds a label" flag, as it reads rows without the W test)
    pl.lane_ok = A->opt.lane != 0 && A->packed_valid && A->opt.multi_pass != 1
                 && lane_enabled(A->cfg, A->dcfg, A->graph->g.k, l.Lmax, A->no_fast, &LP, &lane_why,
                                 pl.labeled ? (1u | (A->anno_dummy_clean ? 2u : 0u)) : 0u)
                 && (A->opt.lane == 1 || pl.n >= (uint64_t)pl.lane_blocks * 16);       // (a small batch: the spread / 64-lane kernels are quicker)
    if (!pl.lane_ok) return MGX_OK;
    LP.max_cols = lane_max_cols(l.Lmax, A->dcfg.xdrop);
    LP.hash_slots = next_pow2(2ull * LP.max_cols);
    if (int hm; env_int("MGX_LANE_HASH_MULT", &hm)) LP.hash_slots *= (uint32_t)std::max(1, hm);
    LP.rest_stride = (lane_rest_bytes(LP.max_cols, LP.hash_slots) + 63) & ~63ull;
    LP.wave_stride = lane_wave_scratch_bytes(LP.max_cols, LP.rest_stride);
    const size_t before = A->lane_scratch.bytes;
    if (A->lane_scratch.ensure((size_t)pl.lane_blocks * LP.wave_stride, true) != MGX_OK) pl.lane_ok = false;      // (no room: the group kernel alone)
    else if (A->lane_scratch.bytes != before) HIP_TRY(hipMemsetAsync(A->lane_scratch.p, 0, A->lane_scratch.bytes, A->hstream));    // node tables start empty
    return MGX_OK;
}

// How many reads are in flight at once (slots), each with a slice of the arena: as many as the kernels keep resident, or as
// the free memory holds.
static int size_arena(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    const uint64_t n = pl.n, stride = arena_bytes(l);
    pl.stride = stride;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    pl.wave_slots = (uint64_t)pl.cus * 4 * MGX_ALIGN_WAVES_PER_SIMD;
    // (post_chain_alignments keeps up to MGX_MAX_ALTERNATIVE_PATHS alignments per query: the build with room for them)
    pl.agg_cap = std::max<uint64_t>(1, A->cfg.post_chain_alignments ? (uint64_t)post_chain_capacity(A->cfg.num_alternative_paths) : A->cfg.num_alternative_paths);
    pl.grp = &group_build(pl.labeled, A->dcfg.canonical >= 2, pl.agg_cap);
    // (label-aware batches: seeding as ever, extension on the labeled builds)
    const uint64_t want_slots = std::max<uint64_t>(pl.wave_slots, (uint64_t)pl.cus * waves_per_cu(*pl.grp) * 8);
    // The arena gets what is free after the buffers this stage allocates AFTER it (result records, output stream, seed
    // stream, sort arrays: estimated generously) and a margin; buffers kept from an earlier batch are already outside
    // `free_b`.  (Half of the free memory, as before, left 15 % of the extension kernel's groups without a slice at
    // 10 M reads next to a host framework's cached allocations.)
    const uint64_t later = n * (sizeof(ReadResult) + sizeof(SeedHdr) + 24 + 16)
                           + (n * (((uint64_t)l.Lmax + l.Lmax / 4 + 40) * pl.agg_cap) + 1024) * 4
                           + (n * 24 + A->total_kmers / 8 + 4096) * A->seed_scale * sizeof(DevSeed) + (1ull << 30);
    const uint64_t held = A->results.bytes + A->stream.bytes + A->seed_stream.bytes + A->seed_hdr.bytes;     // re-used as far as they reach
    const uint64_t need_later = later > held ? later - held : 0;
    const uint64_t avail = (uint64_t)free_b + A->arena.bytes + g_pool.held_bytes();     // a growing arena frees its old block first; what the
                                                                                          // block pool holds is handed out or freed on demand
    uint64_t budget = avail > need_later ? (avail - need_later) / 10 * 9 : avail / 2;
    // (device_share: this handle is one of several at work on the device — each gets its share of the slots the machine can keep
    // resident and of the memory, instead of the first handles taking all of it and the later ones what is left)
    const uint64_t share = (uint64_t)std::max(1, A->opt.device_share);
    budget /= share;
    uint64_t slots = std::min<uint64_t>(std::min<uint64_t>((want_slots + share - 1) / share, std::max<uint64_t>(n, 1)), std::max<uint64_t>(1, budget / stride));
    if (slots == 0) slots = 1;
    // The hash tables of the convergence checker are cleared by generation tags that persist in each slice,
    // so a slice only needs zeroing when its layout (stride) changes or the buffer is new.
    const size_t before = A->arena.bytes;
    if (int rc = A->arena.ensure(slots * stride, true)) return rc;
    if (A->arena.bytes != before || A->arena_stride != stride) {
        HIP_TRY(hipMemsetAsync(A->arena.p, 0, A->arena.bytes, A->hstream));
        A->arena_stride = stride;
    }
    pl.slots = slots;
    A->n_slots = (uint32_t)slots;
    if (probe_env_set("MGX_DEBUG_SLOTS")) fprintf(stderr, "run_align: n %llu stride %llu want_slots %llu slots %llu free %.1f GB\n", (unsigned long long)n, (unsigned long long)stride, (unsigned long long)want_slots, (unsigned long long)slots, free_b / 1e9);
    return MGX_OK;
}

// Result records, output stream, seed stream and sort arrays of the batch; the cursors and counters of this run start at zero.
static int size_buffers(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    const uint64_t n = pl.n;
    if (int rc = A->results.ensure(n * sizeof(ReadResult))) return rc;
    uint64_t words_per_read = ((uint64_t)l.Lmax + l.Lmax / 4 + 40) * pl.agg_cap;
    if (pl.labeled) words_per_read = words_per_read * 2 + 16;      // (an alignment per label group + the label lists; heuristic as below)
    // heuristic size (one alignment per read: nodes + CIGAR runs + path characters); a batch that needs more is re-run
    // with what it asked for (mgx_align_batch_device), so the size is never a correctness limit
    A->out_words = std::max<uint64_t>(n * words_per_read + 1024, A->out_min_words);
    if (int rc = A->stream.ensure(A->out_words * 4)) return rc;
    if (A->keep_seeds) {
        if (int rc = A->dbg_seeds.ensure(n * 2 * (uint64_t)l.max_seeds * sizeof(DevSeed))) return rc;
        HIP_TRY(hipMemsetAsync(A->dbg_seeds.p, 0, n * 2 * (uint64_t)l.max_seeds * sizeof(DevSeed), A->hstream));
    }
    HIP_TRY(clear_cursors(A, CUR_OUT, CUR_RETRY));
    HIP_TRY(hipMemsetAsync(A->d_stats.p, 0, sizeof(KernelStats), A->hstream));     // counters of this run of the stage only
    // Seeds travel from the seeding kernels to the extension kernels through a compact stream.  Typical reads carry a handful
    // of seeds; long or repetitive ones scale with their k-mer count.  The stream is sized by a heuristic times A->seed_scale;
    // mgx_align_batch_device re-runs the stage with a larger scale if the seeding kernel ran out of room (the cursor keeps
    // counting), so the size is never a correctness limit.
    A->seed_cap = std::min<uint64_t>(n * 2 * (uint64_t)l.max_seeds, (n * 24 + A->total_kmers / 8 + 4096) * A->seed_scale);
    if (int rc = A->seed_hdr.ensure(n * sizeof(SeedHdr))) return rc;
    if (int rc = A->seed_stream.ensure(A->seed_cap * sizeof(DevSeed))) return rc;
    if (int rc = A->work_key.ensure(n * 4)) return rc;
    if (int rc = A->work_key_sorted.ensure(n * 4)) return rc;
    if (int rc = A->order_in.ensure(n * 4)) return rc;
    if (int rc = A->order.ensure(n * 4)) return rc;
    if (int rc = A->retry_list.ensure(n * 4 + 4)) return rc;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, pl.sort_tmp_bytes, A->work_key.as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                               A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)n, 0, work_key_bits(n), A->hstream));
    return A->sort_tmp.ensure(pl.sort_tmp_bytes);
}

// the kernels' parameter block (host side only: every buffer it points to exists by now)
static void fill_params(mgx_aligner *A, AlignPlan &pl, const char *d_seqs, const uint64_t *d_offsets) {
    AlignParams &P = pl.P;
    memset(&P, 0, sizeof(P));
    P.g = A->graph->g;
    P.cfg = A->dcfg;
    P.lim = A->lim;
    P.score_matrix = A->score_matrix.as<int8_t>();
    P.seqs = d_seqs;
    P.offsets = d_offsets;
    P.node_begin = A->node_begin.as<uint64_t>();
    P.nodes_fwd = A->nodes_fwd.as<uint32_t>();
    P.nodes_rc = A->nodes_rc.as<uint32_t>();
    P.mlen_fwd = A->mlen_fwd.as<uint8_t>();
    P.mlen_rc = A->mlen_rc.as<uint8_t>();
    P.rng_fwd = A->have_rng ? A->rng_fwd.as<uint2>() : nullptr;
    P.rng_rc = A->have_rng ? A->rng_rc.as<uint2>() : nullptr;
    P.n_reads = pl.n;
    P.arena = A->arena.as<uint8_t>();
    P.arena_stride = pl.stride;
    P.results = A->results.as<ReadResult>();
    P.out_stream = A->stream.as<uint32_t>();
    P.out_capacity = A->out_words;
    P.out_cursor = cursor(A, CUR_OUT);
    P.read_cursor = cursor(A, CUR_READ);
    P.stats = A->d_stats.as<KernelStats>();
    P.dbg_seeds = A->keep_seeds ? A->dbg_seeds.as<DevSeed>() : nullptr;
    P.no_fast = A->no_fast;
    if (A->packed_valid) {
        P.pkw[0] = A->pk_fwd.as<uint64_t>(); P.ivw[0] = A->iv_fwd.as<uint32_t>();
        P.pkw[1] = A->dcfg.fwd_and_rc ? A->pk_rc.as<uint64_t>() : nullptr; P.ivw[1] = A->dcfg.fwd_and_rc ? A->iv_rc.as<uint32_t>() : nullptr;
    }
    P.no_compact = A->opt.no_compact != 0;
    P.no_alias = A->opt.no_alias != 0;
    P.no_bt_runs = A->opt.no_bt_runs != 0;
    P.no_flat = A->opt.no_flat != 0 || A->cfg.post_chain_alignments;       // (the flat group loop is the one-alignment-per-query driver)
    if (pl.labeled) {
        int adev = 0;
        mgx_annotation_device_view(A->anno, &adev, &P.anno_rows, &P.anno_head, &P.anno_count, &P.anno_more);
        P.labeled = 1u | (A->anno_dummy_clean ? 2u : 0u);
        P.anno_base = A->graph->mode == MGX_MODE_CANONICAL ? A->graph->canon_repr.as<uint32_t>() : nullptr;
        P.no_alias = 1;           // (a flush clears columns in place: convergence entries must not alias their S windows)
    }
    P.ablate = probe_env_u32("MGX_ABLATE", 0u);      // timing probes: WRONG results (probe builds only)
    P.seed_hdr = A->seed_hdr.as<SeedHdr>();
    P.seed_stream = A->seed_stream.as<DevSeed>();
    P.seed_capacity = A->seed_cap;
    P.seed_cursor = cursor(A, CUR_SEED);
    P.work_key = A->work_key.as<uint32_t>();
}

// The lane-per-read seeder (seed_lane.hpp, mgx_seedlane.hip) first: every lane seeds its own read and either publishes
// header, seeds and work key as the seeding kernel would, or lists the read for a second pass with bigger buffers; what that
// leaves is listed for the seeding kernel, which then seeds the list from scratch (no host round trip in between: the lists'
// lengths stay on the device).
static int seed_by_lanes(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    AlignParams &P = pl.P;
    const uint64_t n = pl.n;
    const bool seed_lane = A->opt.seed_lane != 0 && A->packed_valid && P.pkw[0] && P.ivw[0]
                           && (!A->dcfg.fwd_and_rc || (P.pkw[1] && P.ivw[1])) && P.mlen_fwd && P.rng_fwd
                           && (!A->dcfg.fwd_and_rc || (P.mlen_rc && P.rng_rc))
                           && seed_lane_enabled(A->dcfg, (uint32_t)A->graph->g.k, l.Lmax, true, true)
                           && (A->opt.seed_lane == 1 || n >= 4096);
    if (!seed_lane || !n) return MGX_OK;
    const bool long_reads = l.Lmax > (uint32_t)SL_SHORT_L;            // (the kernel's build with nine packed words per strand)
    const uint32_t resident = pl.cus * 4 * (uint32_t)mgx_seed_lane_waves_per_simd();
    const uint32_t blocks1 = (uint32_t)std::min<uint64_t>(resident, (n + 63) / 64);
    // (the second pass: what the first left — a sixth of a typical batch — with the big buffers)
    const uint32_t blocks2 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident / (long_reads ? 2 : 1), (n / 4 + 63) / 64));
    const bool many = (uint64_t)A->graph->g.k >= A->dcfg.max_seed_length;
    const uint32_t me1 = many ? (long_reads ? SL_SEEDS_1_MANY_LONG : SL_SEEDS_1_MANY) : SL_SEEDS_1, mp1 = many ? SL_PENDING_1_MANY : SL_PENDING_1;
    const uint32_t me2 = long_reads ? SL_SEEDS_2_LONG : SL_SEEDS_2, mp2 = long_reads ? SL_PENDING_2_LONG : SL_PENDING_2;
    const uint64_t words1 = seed_lane_wave_scratch_words(me1, mp1), words2 = seed_lane_wave_scratch_words(me2, mp2);
    if (int rc = A->seedlane_scratch.ensure((size_t)std::max<uint64_t>(blocks1 * words1, blocks2 * words2) * 4)) return rc;
    if (int rc = A->seedlane_params.ensure(2 * sizeof(SeedLaneParams))) return rc;
    if (int rc = A->seedlane_bail.ensure(2 * (n * 4 + 4))) return rc;
    if (int rc = A->seedlane_hist.ensure(32 * 8)) return rc;          // ([16 .. 24): section timers of -DMGX_SL_TIMERS builds)
    HIP_TRY(hipMemsetAsync(A->seedlane_hist.p, 0, 32 * 8, A->hstream));
    HIP_TRY(clear_cursors(A, CUR_SL_BAIL, CUR_SL_BAIL_BACK));
    SeedLaneParams SP[2];
    memset(SP, 0, sizeof(SP));
    uint32_t *list1 = A->seedlane_bail.as<uint32_t>(), *list2 = list1 + n + 1;
    for (int ps = 0; ps < 2; ++ps) {
        SP[ps].P = P;
        SP[ps].P.n_items = n;
        SP[ps].scratch = A->seedlane_scratch.as<uint32_t>();
        SP[ps].long_reads = long_reads ? 1u : 0u;
        SP[ps].second_pass = (uint32_t)ps;
        SP[ps].list_len = n;
        SP[ps].done_count = cursor(A, CUR_SL_DONE);
    }
    // first pass: every read; what it leaves goes to list1 from both ends
    SP[0].max_entries = me1; SP[0].max_pending = mp1;
    SP[0].bail_list = list1; SP[0].bail_count = cursor(A, CUR_SL_BAIL); SP[0].bail_count_back = cursor(A, CUR_SL_BAIL_BACK);
    // second pass: list1; what it leaves goes to list2 (why a read left is counted where it leaves for the wave program)
    SP[1].max_entries = me2; SP[1].max_pending = mp2;
    SP[1].in_list = list1; SP[1].in_count = cursor(A, CUR_SL_BAIL); SP[1].in_count_back = cursor(A, CUR_SL_BAIL_BACK);
    SP[1].bail_list = list2; SP[1].bail_count = cursor(A, CUR_SL_BAIL2);
    SP[1].bail_hist = A->seedlane_hist.as<unsigned long long>();
    HIP_TRY(copy_sync(A, A->seedlane_params.p, SP, sizeof(SP), hipMemcpyHostToDevice));
    if (int rc = mgx_launch_seed_lane(A->seedlane_params.p, blocks1, long_reads, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane-per-read seeder: %d", rc);
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    if (int rc = mgx_launch_seed_lane(A->seedlane_params.as<SeedLaneParams>() + 1, blocks2, long_reads, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane-per-read seeder, second pass: %d", rc);
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    P.seed_list = list2;
    P.n_items_ptr = cursor(A, CUR_SL_BAIL2);
    A->seedlane_launched = 1;
    return MGX_OK;
}

// The seeding kernel, one wavefront per read, on every read or on what the lane-per-read seeder listed: the instantiation at
// 8 wavefronts per SIMD for short reads on a full machine, else the one at MGX_ALIGN_WAVES_PER_SIMD; PRIMARY graphs: the
// builds with the CanonicalDBG branches (mgx_primary.hip).
static int seed_by_waves(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    AlignParams &P = pl.P;
    const bool primary = A->dcfg.canonical >= 2;
    // (static LDS of the seeding kernels: control block + the interval lists of the sdust scratch; no score rows — seed_kernel.hpp)
    const uint32_t static_lds = (uint32_t)((sizeof(Wave) + SDUST_LDS_BYTES_REGTAB + 16 + 127) & ~127ull);
    if (A->opt.seed_wps == 8 && l.Lmax <= 192 && pl.slots >= (uint64_t)pl.cus * 4 * 8) {
        // (measured on 150-bp reads: the kernel is 10 % faster with 4944 B of LDS per wavefront than with 5056 B, although
        // both leave room for 32 wavefronts per CU; hence the wider margin)
        uint32_t lds8 = lds_per_read(l.Lmax, 4 * MGX_SEED_WPS, static_lds, 192u);
        lds8 = std::min<uint32_t>(lds8, probe_env_u32("MGX_SEED_LDS_CAP", lds8)) & ~15u;     // tuning probe
        if (probe_env_set("MGX_SEED_LDS_PRINT")) fprintf(stderr, "k_seed: static_lds %u budget8 %u lds8 %u (fast_lds_bytes %u)\n", static_lds, lds_budget(4 * MGX_SEED_WPS, static_lds, 192u), lds8, fast_lds_bytes(l.Lmax));
        if (primary) {
            if (int rc = mgx_launch_seed_primary(&P, pl.cus * 4 * MGX_SEED_WPS, lds8, 1, A->hstream))
                return fail(MGX_ERR_NO_DEVICE, "seeding kernel (PRIMARY): %d", rc);
        } else {
            // tuning probe: MGX_SEED_WAVES_PCT=50 launches half the resident wavefronts (is the kernel bound by what each
            // wavefront waits for, or by what all of them move?)
            const uint32_t spct = probe_env_pct("MGX_SEED_WAVES_PCT");
            k_align<PH_SEED, MGX_SEED_WPS><<<std::max(1u, pl.cus * 4 * MGX_SEED_WPS * spct / 100), 64, lds8, A->hstream>>>(P, lds8);
        }
    } else {
        const uint32_t lds_bytes = lds_per_read(l.Lmax, 4 * MGX_ALIGN_WAVES_PER_SIMD, static_lds, 64u);
        const uint32_t w_slots = (uint32_t)std::min<uint64_t>(pl.slots, pl.wave_slots);
        if (primary) {
            if (int rc = mgx_launch_seed_primary(&P, w_slots, lds_bytes, 0, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "seeding kernel (PRIMARY): %d", rc);
        } else {
            k_align<PH_SEED><<<w_slots, 64, lds_bytes, A->hstream>>>(P, lds_bytes);
        }
    }
    HIP_TRY(hipGetLastError());
    P.seed_list = nullptr; P.n_items_ptr = nullptr;
    return MGX_OK;
}

// the reads in the order of their predicted extension work (the seeding kernels wrote the keys)
static int sort_by_work(mgx_aligner *A, AlignPlan &pl) {
    const uint64_t n = pl.n;
    k_iota<<<(uint32_t)((n + 255) / 256), 256, 0, A->hstream>>>(A->order_in.as<uint32_t>(), n);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(A->sort_tmp.p, pl.sort_tmp_bytes, A->work_key.as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                               A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)n, 0, work_key_bits(n), A->hstream));
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    pl.P.order = A->order.as<uint32_t>();
    return MGX_OK;
}

// Multi-pass extension (option multi_pass; default: when a batch carries many seeds per read): a pass extends at most one seed
// per read; reads with live seeds left write a resume record and are re-sorted by the work of their next seed for the next pass
// (AlignParams::resume_*).  Reads of a wavefront then differ by one extension at most, instead of waiting for the mate with
// the most seeds.
static int choose_multi_pass(mgx_aligner *A, const AlignPlan &pl, bool *multi) {
    *multi = false;
    if (pl.labeled || A->cfg.post_chain_alignments) return MGX_OK;      // (resume records hold num_alternative_paths alignments)
    *multi = A->opt.multi_pass == 1;
    if (A->opt.multi_pass < 0) {
        // automatic: worth it when reads run many extensions, i.e. carry many seeds (sub-k seeds of a pan-genome: ~100 per
        // read; a plain read: a handful).  The seeding kernel has finished counting them by now.
        unsigned long long seeds_total = 0;
        HIP_TRY(copy_sync(A, &seeds_total, cursor(A, CUR_SEED), 8, hipMemcpyDeviceToHost));
        *multi = pl.n > 0 && seeds_total / pl.n >= 24;
    }
    return MGX_OK;
}

// Every read through the lane-per-read kernel first, in the sorted order; what it lists goes on to the extension kernel
// (the plan's order and item count become that list; *all_done: it is empty).
static int extend_by_lanes(mgx_aligner *A, AlignPlan &pl, bool *all_done) {
    AlignParams &P = pl.P;
    LaneParams &LP = pl.LP;
    const uint64_t n = pl.n;
    if (int rc = A->lane_bail.ensure(n * 4 + 4)) return rc;
    if (int rc = A->lane_params.ensure(sizeof(LaneParams))) return rc;
    if (int rc = A->lane_hist.ensure(64 * 8)) return rc;          // ([32 .. 63]: section timers of -DMGX_LANE_TIMERS builds)
    HIP_TRY(hipMemsetAsync(A->lane_hist.p, 0, 64 * 8, A->hstream));
    HIP_TRY(clear_cursors(A, CUR_LANE_BAIL, CUR_LANE_DONE));
    LP.P = P;
    LP.P.n_items = n;
    LP.pk[0] = A->pk_fwd.as<uint64_t>(); LP.pk[1] = A->pk_rc.as<uint64_t>();
    LP.iv[0] = A->iv_fwd.as<uint32_t>(); LP.iv[1] = A->iv_rc.as<uint32_t>();
    LP.scratch = A->lane_scratch.as<uint8_t>();
    LP.tag_seed = ++A->lane_epoch * 0x632BE5ABu;
    LP.bail_list = A->lane_bail.as<uint32_t>();
    LP.bail_count = cursor(A, CUR_LANE_BAIL);
    LP.done_count = cursor(A, CUR_LANE_DONE);
    LP.bail_hist = A->lane_hist.as<unsigned long long>();
    HIP_TRY(copy_sync(A, A->lane_params.p, &LP, sizeof(LP), hipMemcpyHostToDevice));
    uint32_t blocks = (uint32_t)std::min<uint64_t>(pl.lane_blocks, (n + 63) / 64);
    if (int pct; env_int("MGX_LANE_BLOCKS_PCT", &pct)) blocks = std::max<uint32_t>(1u, (uint32_t)((uint64_t)blocks * (uint64_t)pct / 100));
    if (int rc = mgx_launch_lane(A->lane_params.p, blocks, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane kernel: %d", rc);
    A->kernels_ran |= MGX_KERNEL_LANE;
    ++g_kernel_launches[CNT_LANE];
    HIP_TRY(hipEventRecord(A->ev[EV_LANE_END], A->hstream));
    unsigned long long counts[2] = { 0, 0 };      // CUR_LANE_BAIL, CUR_LANE_DONE
    HIP_TRY(copy_sync(A, counts, cursor(A, CUR_LANE_BAIL), 16, hipMemcpyDeviceToHost));     // (synchronises with the kernel)
    A->lane_done = counts[1];
    HIP_TRY(copy_sync(A, A->lane_hist_h, A->lane_hist.p, 32 * 8, hipMemcpyDeviceToHost));
    if (int on; env_int("MGX_LANE_TIMERS", &on)) {
        unsigned long long t[16];
        HIP_TRY(copy_sync(A, t, A->lane_hist.as<unsigned long long>() + 32, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "k_lane timers (cycles of lane 0, summed over %u wavefronts): setup %llu children %llu column %llu node-table %llu commit %llu frontier %llu trace %llu result %llu | emit %llu kernel %llu\n",
                blocks, t[0], t[1], t[2], t[7], t[3], t[4], t[5], t[6], t[8], t[9]);
    }
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    P.order = A->lane_bail.as<uint32_t>();
    P.n_items = counts[0];
    *all_done = counts[0] == 0;
    return MGX_OK;
}

// One launch of the extension kernel on the plan's work items (P.order / P.n_items): which build, on how many groups or
// wavefronts (never more than arena slices), with how much LDS per read.  Returns the launcher's hipError_t.
static int launch_extension(mgx_aligner *A, AlignPlan &pl) {
    const uint32_t Lmax = A->lim.Lmax;
    const int gpw_opt = A->opt.groups_per_wave;                             // -1 = automatic, 0 = all 8
    const uint64_t items = pl.P.n_items ? pl.P.n_items : pl.n;             // (a later pass of the multi-pass extension: its retry positions)
    const ExtBuild *b = pl.grp;
    uint32_t gpw, count, lds;         // AlignParams::groups_per_wave (0 = all 8); groups (8-lane builds) or wavefronts; LDS per read
    if (pl.labeled) {
        // label-aware extension: the labeled builds — 8 reads per wavefront (mgx_grp.hip, per-read program), or one read
        // per wavefront on the 64-lane kernel (mgx_lab64.hip) for batches with fewer reads than resident wavefronts
        const ExtBuild &lab64 = g_ext_builds[EXT_LAB64];
        const uint64_t resident64 = (uint64_t)pl.cus * waves_per_cu(lab64);
        if ((items <= resident64 && A->opt.ext64 != 0) || A->opt.ext64 == 2) {
            b = &lab64; gpw = 1;
            count = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(pl.slots, resident64));
        } else {
            gpw = gpw_opt > 0 ? (uint32_t)std::min(8, gpw_opt) : 0u;
            count = (uint32_t)pl.slots;
        }
    } else {
        // tuning probe: MGX_EXT_GROUPS_PCT=50 launches half the resident groups (occupancy experiments)
        const uint32_t pct = probe_env_pct("MGX_EXT_GROUPS_PCT");
        count = (uint32_t)std::min<uint64_t>(pl.slots, std::max<uint64_t>(1, pl.slots * pct / 100));
        // Fewer reads than resident groups (long-read batches, single queries): spread them over the wavefronts.  The 8
        // groups of a wavefront execute in lock-step, and reads of 1 .. 12 kbp side by side wait for each other's general
        // steps two thirds of the time (config 0: 1.35 s with 8 reads per wavefront on 125 of 3072 wavefronts).  The arena
        // slices stay what they are: slot = wavefront x groups_per_wave + group.
        const uint64_t resident_waves = (uint64_t)pl.cus * waves_per_cu(*pl.grp);
        const uint64_t busy = std::min<uint64_t>(count, std::max<uint64_t>(1, items));
        const uint64_t want_gpw = std::min<uint64_t>(8, std::max<uint64_t>(1, (busy + resident_waves - 1) / resident_waves));
        gpw = gpw_opt >= 0 ? (uint32_t)std::min(8, gpw_opt) : (want_gpw < 8 ? (uint32_t)want_gpw : 0u);
        // One read per wavefront: the 64-lane instantiation (mgx_ext64.hip) — the read has the wavefront to itself, so it may as
        // well use all of its lanes.  (Option ext64=0: the 8-lane groups all the same.)
        if (A->opt.ext64 != 0 && gpw == 1) b = &g_ext_builds[EXT_EXT64];
    }
    if (b->launch_64) {
        lds = lds_per_read(Lmax, waves_per_cu(*b), b->static_lds(), 128u);
    } else {
        lds = lds_per_read(Lmax, waves_per_cu(*b), b->static_lds(), 64u, 8);
        if (!pl.labeled) lds = std::min<uint32_t>(lds, probe_env_u32("MGX_EXT_LDS_CAP", lds)) & ~15u;   // tuning probe
    }
    pl.P.groups_per_wave = gpw;
    A->kernels_ran |= b->kernel_bit;
    if (b->counter != CNT_NONE) ++g_kernel_launches[b->counter];
    // (8-lane builds: a partial last wavefront is fine, the kernel returns for slot >= n_groups)
    return b->launch_64 ? b->launch_64(&pl.P, count, lds, A->hstream) : b->launch_grp(&pl.P, count, lds, PH_EXTEND, A->hstream);
}

// The passes of the multi-pass extension (choose_multi_pass): launch, count the reads that want another pass, sort their
// retry positions by the work of their next seed, again.
static int extend_multi_pass(mgx_aligner *A, AlignPlan &pl) {
    AlignParams &P = pl.P;
    const uint64_t n = pl.n;
    const uint32_t rb = resume_rec_bytes(A->lim, (uint32_t)std::max<uint64_t>(1, A->cfg.num_alternative_paths));
    size_t fb = 0, tb = 0;
    HIP_TRY(hipMemGetInfo(&fb, &tb));
    fb += g_pool.held_bytes();
    const uint64_t have = A->resume_pool[0].bytes + A->resume_pool[1].bytes;
    uint64_t cap = std::min<uint64_t>(n, ((uint64_t)fb / 2 + have) / (2ull * rb));      // two pools
    if (cap > 0xFFFFFFF0ull) cap = 0xFFFFFFF0ull;
    if (cap == 0) {               // (no room for resume records: every seed of a read in one launch)
        HIP_TRY((hipError_t)launch_extension(A, pl));
        return MGX_OK;
    }
    for (int b = 0; b < 2; ++b) {
        if (int rc = A->resume_pool[b].ensure(cap * rb, true)) return rc;
        if (int rc = A->retry_key[b].ensure(n * 4 + 4)) return rc;
    }
    if (int rc = A->retry_list2.ensure(n * 4 + 4)) return rc;
    DevBuf *lists[2] = { &A->retry_list, &A->retry_list2 };
    P.resume_rec_bytes = rb; P.resume_cap = (uint32_t)cap;
    P.retry_count = cursor(A, CUR_RETRY);
    P.resume_in = nullptr; P.resume_reads = nullptr;
    int out = 0;
    for (uint32_t pass = 0;; ++pass) {
        P.resume_out = A->resume_pool[out].as<uint8_t>();
        P.retry_list = lists[out]->as<uint32_t>();
        P.retry_key = A->retry_key[out].as<uint32_t>();
        // later passes take more seeds per read, so that the number of launches stays small
        P.seed_limit = pass < 8 ? 1 : pass < 16 ? 4 : pass < 24 ? 16 : 0;
        HIP_TRY((hipError_t)launch_extension(A, pl));
        unsigned long long c = 0;
        HIP_TRY(copy_sync(A, &c, cursor(A, CUR_RETRY), 8, hipMemcpyDeviceToHost));     // (synchronises with the pass)
        c = std::min<unsigned long long>(c, cap);
        A->n_passes = pass + 1;
        if (c == 0 || P.seed_limit == 0) break;
        // next pass: the retry positions of this one, sorted by their work key
        k_iota<<<(uint32_t)((c + 255) / 256), 256, 0, A->hstream>>>(A->order_in.as<uint32_t>(), c);
        size_t tmp_bytes = pl.sort_tmp_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(A->sort_tmp.p, tmp_bytes, A->retry_key[out].as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                                   A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)c, 0, 12, A->hstream));
        HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
        HIP_TRY(clear_cursors(A, CUR_RETRY, CUR_RETRY));
        P.order = A->order.as<uint32_t>();
        P.n_items = c;
        P.resume_in = A->resume_pool[out].as<uint8_t>();
        P.resume_reads = lists[out]->as<uint32_t>();
        out ^= 1;
    }
    return MGX_OK;
}

static int run_align(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax) {
    {
        std::string err;
        int rc = derive_limits(A->cfg, A->have_user_lim ? &A->user_lim : nullptr, Lmax, &A->lim, &err, A->anno != nullptr, A->label_scale);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, A->graph->device));
    AlignPlan pl;
    pl.n = n;
    pl.labeled = A->anno != nullptr;
    pl.cus = (uint32_t)prop.multiProcessorCount;
    if (int rc = plan_lane(A, pl)) return rc;
    if (int rc = size_arena(A, pl)) return rc;
    if (int rc = size_buffers(A, pl)) return rc;
    fill_params(A, pl, d_seqs, d_offsets);
    HIP_TRY(hipEventRecord(A->ev[EV_ALIGN_BEGIN], A->hstream));
    A->kernels_ran = 0;
    A->seedlane_launched = 0;
    if (int rc = seed_by_lanes(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SEED_LANE_END], A->hstream));
    if (int rc = seed_by_waves(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SEEDED], A->hstream));
    if (int rc = sort_by_work(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SORTED], A->hstream));
    bool multi = false;
    if (int rc = choose_multi_pass(A, pl, &multi)) return rc;
    A->n_passes = 1;
    A->lane_done = 0;
    memset(A->lane_hist_h, 0, sizeof(A->lane_hist_h));
    HIP_TRY(hipEventRecord(A->ev[EV_LANE_END], A->hstream));      // (recorded again behind the lane kernel, if it runs)
    bool all_done = false;        // every read finished in the lane kernel
    if (pl.lane_ok && !multi && n) {
        if (int rc = extend_by_lanes(A, pl, &all_done)) return rc;
    }
    if (multi) {
        if (int rc = extend_multi_pass(A, pl)) return rc;
    } else if (!all_done) {
        HIP_TRY((hipError_t)launch_extension(A, pl));
    }
    HIP_TRY(hipEventRecord(A->ev[EV_ALIGN_END], A->hstream));
    return MGX_OK;
}

static int collect_stats(mgx_aligner *A, bool mapped, bool aligned) {
    HIP_TRY(hipStreamSynchronize(A->hstream));
    KernelStats ks, km;
    HIP_TRY(copy_sync(A, &ks, A->d_stats.p, sizeof(ks), hipMemcpyDeviceToHost));
    HIP_TRY(copy_sync(A, &km, A->d_stats_map.p, sizeof(km), hipMemcpyDeviceToHost));
    ks.rank_lines += km.rank_lines; ks.select_lines += km.select_lines; ks.bit_lines += km.bit_lines; ks.map_lines += km.map_lines;
    mgx_stats &s = A->hstats;
    memset(&s, 0, sizeof(s));
    s.n_reads = A->n_reads;
    s.n_rank_lines = ks.rank_lines; s.n_select_lines = ks.select_lines; s.n_bit_lines = ks.bit_lines;
    s.n_columns = ks.columns; s.n_extensions = ks.extensions; s.n_seeds = ks.seeds;
    s.n_map_lines = ks.map_lines; s.n_capacity_errors = ks.capacity_errors; s.n_seed_lines = ks.seed_lines;
    s.n_fast_columns = ks.fast_columns;
    s.extend_kernels = A->kernels_ran;
    s.n_lane_reads = A->lane_done;
    s.n_lane_lines = ks.lane_lines; s.n_lane_columns = ks.lane_columns;
    for (int x = 0; x < 32; ++x) s.lane_bail_reads[x] = A->lane_hist_h[x];
    if (int on; aligned && A->seedlane_launched && env_int("MGX_SL_TIMERS", &on)) {
        unsigned long long t[8];
        HIP_TRY(copy_sync(A, t, A->seedlane_hist.as<unsigned long long>() + 16, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "k_seed_lane timers (cycles of lane 0, summed over the wavefronts): strands %llu masks %llu scan %llu walks %llu dust %llu ranges+enumerate %llu publish %llu wave-mates %llu\n",
                t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
    if (aligned && A->seedlane_launched) {
        unsigned long long done = 0, why[16];
        HIP_TRY(copy_sync(A, &done, cursor(A, CUR_SL_DONE), 8, hipMemcpyDeviceToHost));
        HIP_TRY(copy_sync(A, why, A->seedlane_hist.p, sizeof(why), hipMemcpyDeviceToHost));
        s.n_seed_lane_reads = done;
        for (int x = 0; x < 16; ++x) s.seed_lane_left_reads[x] = why[x];
    }
    for (int x = 0; x < 8; ++x) { s.phase_cycles[x] = ks.cyc[x]; s.extend_cycles[x] = ks.xcyc[x]; }
    float ms = 0;
    if (mapped) { HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_MAP_BEGIN], A->ev[EV_MAP_END])); s.seed_kernel_ms = ms; }
    if (aligned) {
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_ALIGN_END])); s.align_kernel_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_SEEDED])); s.seeding_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SEEDED], A->ev[EV_SORTED])); s.sort_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SORTED], A->ev[EV_ALIGN_END])); s.extend_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SORTED], A->ev[EV_LANE_END])); s.lane_ms = ms;
        if (A->seedlane_launched) { HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_SEED_LANE_END])); s.seed_lane_ms = ms; }
    }
    return MGX_OK;
}

int mgx_map_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device, mgx_mapping *out) {
    if (!A || !seqs || !offsets || !out) return fail(MGX_ERR_INVALID, "null argument");
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const char *d_seqs; const uint64_t *d_offsets; uint32_t Lmax;
    if (int rc = stage_batch(A, seqs, offsets, n, on_device, &d_seqs, &d_offsets, &Lmax)) return rc;
    if (int rc = run_map(A, d_seqs, d_offsets, n, true, true, Lmax)) return rc;
    if (int rc = collect_stats(A, true, false)) return rc;
    A->m_node_begin.resize(n + 1);
    HIP_TRY(copy_sync(A, A->m_node_begin.data(), A->node_begin.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> f(A->total_kmers), r(A->total_kmers);
    if (A->total_kmers) {
        HIP_TRY(copy_sync(A, f.data(), A->nodes_fwd.p, A->total_kmers * 4, hipMemcpyDeviceToHost));
        HIP_TRY(copy_sync(A, r.data(), A->nodes_rc.p, A->total_kmers * 4, hipMemcpyDeviceToHost));
    }
    A->m_fwd.assign(f.begin(), f.end());
    A->m_rc.assign(r.begin(), r.end());
    out->n_queries = n;
    out->node_begin = A->m_node_begin.data();
    out->nodes_fwd = A->m_fwd.data();
    out->nodes_rc = A->m_rc.data();
    return MGX_OK;
}

// `align --map` (cli/align.cpp:71-179): DeBruijnGraph::map_to_nodes summarised on the device (map_summary.hpp, mgx_mapsum.hip)
static std::atomic<uint64_t> g_map_summary_counts[4];        // mgx_map_kernel_launch_counts
int mgx_map_summary_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device, uint32_t map_length,
                          uint32_t flags, mgx_map_summary *out) {
    if (!A || !seqs || !offsets || !out) return fail(MGX_ERR_INVALID, "null argument");
    const uint32_t k = A->graph->g.k;
    if (map_length > k) return fail(MGX_ERR_INVALID, "map_length %u exceeds k = %u", map_length, k);
    A->ms_generation = 0;
    if (flags & ~(uint32_t)(MGX_MAP_WANT_NODES | MGX_MAP_KEEP_NODES)) return fail(MGX_ERR_INVALID, "unknown flags %u", flags);
    const bool sub_k = map_length != 0 && map_length < k;
    const uint32_t mode = A->graph->mode;
    // the reference casts the CanonicalDBG wrapper to a DBGSuccinct here (cli/align.cpp:117 after :347): undefined, so refused
    if (sub_k && mode == MGX_MODE_PRIMARY) return fail(MGX_ERR_UNSUPPORTED, "map_length < k on a PRIMARY graph is undefined in the reference");
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const char *d_seqs; const uint64_t *d_offsets; uint32_t Lmax;
    if (int rc = stage_batch(A, seqs, offsets, n, on_device, &d_seqs, &d_offsets, &Lmax, sub_k ? map_length : 0)) return rc;
    const bool want_nodes = (flags & MGX_MAP_WANT_NODES) != 0;                               // the node array comes to the host
    const bool keep_nodes = want_nodes || (flags & MGX_MAP_KEEP_NODES) != 0;                 // k_map_summary writes it to ms_nodes
    const uint32_t window = sub_k ? map_length : k;
    const bool any_long = Lmax >= window && Lmax - window + 1 > mgx_map_summary_short_max();
    if (int rc = A->ms_counts.ensure((n + 1) * sizeof(mgx_map_counts))) return rc;
    if (keep_nodes) if (int rc = A->ms_nodes.ensure((A->total_kmers + 1) * 8)) return rc;
    if (any_long) if (int rc = A->ms_sorted.ensure((A->total_kmers + 1) * 4)) return rc;
    int rule = MGX_MODE_BASIC;
    if (sub_k) {
        if (mgx_launch_map_subk(&A->graph->g, d_seqs, d_offsets, A->node_begin.as<uint64_t>(), A->nodes_fwd.as<uint32_t>(), n, map_length, A->hstream))
            return fail(MGX_ERR_NO_DEVICE, "k_map_subk launch failed");
        if (n) ++g_map_summary_counts[2];
    } else {
        // BASIC: the forward strand alone.  CANONICAL: both strands' BOSS edges, the mask after the minimum.  PRIMARY: the wrapper's path.
        rule = (int)mode;
        if (int rc = run_map(A, d_seqs, d_offsets, n, mode != MGX_MODE_BASIC, true, Lmax, mode == MGX_MODE_CANONICAL)) return rc;
    }
    for (int long_form = 0; long_form <= (any_long ? 1 : 0); ++long_form) {
        if (mgx_launch_map_summary(A->node_begin.as<uint64_t>(), A->nodes_fwd.as<uint32_t>(), A->nodes_rc.as<uint32_t>(), A->ms_sorted.as<uint32_t>(),
                                   A->ms_counts.p, keep_nodes ? A->ms_nodes.as<uint64_t>() : nullptr, A->graph->g.valid, n,
                                   (uint32_t)A->graph->g.n, rule, long_form, A->hstream))
            return fail(MGX_ERR_NO_DEVICE, "k_map_summary launch failed");
        if (n) ++g_map_summary_counts[long_form];
    }
    if (!sub_k) { if (int rc = collect_stats(A, true, false)) return rc; }
    A->h_ms_counts.resize(n);
    if (n) HIP_TRY(copy_sync(A, A->h_ms_counts.data(), A->ms_counts.p, n * sizeof(mgx_map_counts), hipMemcpyDeviceToHost));
    else HIP_TRY(hipStreamSynchronize(A->hstream));
    out->n_queries = n;
    out->counts = A->h_ms_counts.data();
    out->node_begin = nullptr;
    out->nodes = nullptr;
    if (want_nodes) {
        A->m_node_begin.resize(n + 1);
        HIP_TRY(copy_sync(A, A->m_node_begin.data(), A->node_begin.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        A->h_ms_nodes.resize(A->total_kmers + 1);
        if (A->total_kmers) HIP_TRY(copy_sync(A, A->h_ms_nodes.data(), A->ms_nodes.p, A->total_kmers * 8, hipMemcpyDeviceToHost));
        g_map_summary_counts[3] += A->total_kmers * 8;
        out->node_begin = A->m_node_begin.data();
        out->nodes = A->h_ms_nodes.data();
    }
    A->ms_generation = A->stage_generation;
    A->ms_d_seqs = d_seqs; A->ms_d_offsets = d_offsets;
    A->ms_map_length = map_length; A->ms_lmax = Lmax; A->ms_have_nodes = keep_nodes;
    return MGX_OK;
}
void mgx_map_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_map_summary_counts[x].load(); }

// the device blocks kept from destroyed aligners (DevPool) go back to the driver
int mgx_device_trim(int device) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    HIP_TRY(hipSetDevice(device));
    g_pool.flush();
    HIP_TRY(hipSetDevice(cur));
    return MGX_OK;
}

int mgx_aligner_set_stream(mgx_aligner *A, void *hip_stream) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(A->graph->device));
    HIP_TRY(hipStreamSynchronize(A->hstream));              // what the handle has in flight finishes where it was issued
    if (A->own_stream) { (void)hipStreamDestroy(A->hstream); A->own_stream = false; }
    A->hstream = (hipStream_t)hip_stream;
    return MGX_OK;
}
int mgx_aligner_create_stream(mgx_aligner *A) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(A->graph->device));
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (int rc = mgx_aligner_set_stream(A, st)) { (void)hipStreamDestroy(st); return rc; }
    A->own_stream = true;
    return MGX_OK;
}
void *mgx_aligner_get_stream(const mgx_aligner *A) { return A ? (void *)A->hstream : nullptr; }

int mgx_aligner_set_pipeline(mgx_aligner *A, const char *name) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    if (!name) return fail(MGX_ERR_INVALID, "unknown pipeline '(null)'");
    // "+general" / "+chain" suffix-free test switches: the extension's register-resident chain path off / on
    if (!strcmp(name, "general")) { A->no_fast = true; return MGX_OK; }
    if (!strcmp(name, "chain")) { A->no_fast = false; return MGX_OK; }
    if (strchr(name, '=')) {
        const std::string key(name, strchr(name, '=') - name);
        const int v = atoi(strchr(name, '=') + 1);
        mgx_aligner::Options &o = A->opt;
        if (key == "ext64") o.ext64 = v;
        else if (key == "groups_per_wave") o.groups_per_wave = std::min(8, v);
        else if (key == "multi_pass") o.multi_pass = v;
        else if (key == "no_compact") o.no_compact = v;
        else if (key == "decode_on_device") o.decode_on_device = v != 0;
        else if (key == "no_alias") o.no_alias = v;
        else if (key == "no_bt_runs") o.no_bt_runs = v;
        else if (key == "no_flat") o.no_flat = v;
        else if (key == "lane") o.lane = v;
        else if (key == "device_share") o.device_share = std::max(1, std::min(v, 64));
        else if (key == "map_pipe") o.map_pipe = v;
        else if (key == "seed_wps") o.seed_wps = v;
        else if (key == "seed_lane") {
            if (v < -1 || v > 1) return fail(MGX_ERR_INVALID, "unknown option '%s'", name);
            o.seed_lane = v;
        }
        else if (key == "retry_capacity") A->retry_capacity = v != 0;
        else return fail(MGX_ERR_INVALID, "unknown option '%s'", name);
        return MGX_OK;
    }
    // (the one pipeline there is, see the top of this file: its name selects nothing)
    if (strcmp(name, "split8")) return fail(MGX_ERR_INVALID, "unknown pipeline '%s'", name);
    return MGX_OK;
}

// MGX_HOST_TIMERS=1: host-side wall time per stage of a batch on stderr (where does a one-read batch spend its 2 ms?)
struct HostStageTimer {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    static bool on() { static const bool v = probe_env_set("MGX_HOST_TIMERS"); return v; }
    explicit HostStageTimer(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostStageTimer() {
        if (on()) fprintf(stderr, "mgx host stage %-14s %8.1f us\n", name,
                          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// kernels only; results stay in HBM
int mgx_align_batch_device(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device) {
    if (!A || !seqs || !offsets) return fail(MGX_ERR_INVALID, "null argument");
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const char *d_seqs; const uint64_t *d_offsets; uint32_t Lmax;
    if (n == 0) { A->n_reads = 0; A->aligned_empty = true; return MGX_OK; }
    A->aligned_empty = false;
    { HostStageTimer t("stage_batch"); if (int rc = stage_batch(A, seqs, offsets, n, on_device, &d_seqs, &d_offsets, &Lmax)) return rc; }
    A->last_d_seqs = d_seqs; A->last_d_offsets = d_offsets; A->aligned_generation = A->stage_generation;
    bool mapped = A->cfg.max_seed_length >= A->graph->g.k;
    { HostStageTimer t("run_map"); if (int rc = run_map(A, d_seqs, d_offsets, n, A->dcfg.fwd_and_rc != 0, mapped, Lmax)) return rc; }
    for (;;) {
        { HostStageTimer t("run_align"); if (int rc = run_align(A, d_seqs, d_offsets, n, Lmax)) return rc; }
        { HostStageTimer t("collect_stats"); if (int rc = collect_stats(A, mapped, true)) return rc; }
        // both streams keep counting past their capacity: reads that found no room got a capacity status and the
        // stage is redone with what it asked for
        unsigned long long out_wanted = 0, seeds_wanted = 0;
        HIP_TRY(copy_sync(A, &out_wanted, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
        bool again = false;
        if (out_wanted > A->out_words) { A->out_min_words = out_wanted + out_wanted / 8 + 1024; again = true; }
        HIP_TRY(copy_sync(A, &seeds_wanted, cursor(A, CUR_SEED), 8, hipMemcpyDeviceToHost));
        if (seeds_wanted > A->seed_cap) {
            A->seed_scale = seeds_wanted / std::max<uint64_t>(1, A->seed_cap / A->seed_scale) + 2;
            again = true;
        }
        if (!again) break;
    }
    A->h_results.clear();          // host copies of an earlier batch must not be mistaken for this one's
    return MGX_OK;
}

static int retry_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, mgx_results *out);

// ---- the mgx_results layout of a batch, written by kernels (results_decode.hpp, mgx_decode.hip): the one host
// sequence behind mgx_decode_results_device (RD_TO_DEVICE: `out` points at the device arrays) and the option decode_on_device of
// mgx_fetch_results (RD_TO_HOST: the seven arrays are copied to the handle's pinned buffers).  The caller has checked that the
// aligned batch is the staged one and that n = A->n_reads > 0.
enum { RD_CNT_SIZE = 0, RD_CNT_WRITE, RD_CNT_D2H_BYTES, RD_CNT_FETCHES };
static std::atomic<uint64_t> g_decode_counts[4];        // mgx_decode_kernel_launch_counts
void mgx_decode_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_decode_counts[x].load(); }

enum RdWhere { RD_TO_DEVICE, RD_TO_HOST };
static int decode_on_device(mgx_aligner *A, RdWhere where, mgx_results *out, mgx_results_sizes *sizes) {
    const char *fn = where == RD_TO_DEVICE ? "mgx_decode_results_device" : "mgx_fetch_results (decode_on_device=1)";
    const uint64_t n = A->n_reads;
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 queries in a batch", fn);
    const uint64_t stride = n + 1;
    if (int rc = A->rd_counts.ensure(RD_ARRAYS * stride * 8)) return rc;
    if (int rc = A->rd_begins.ensure(RD_ARRAYS * stride * 8)) return rc;
    if (int rc = A->rd_totals.ensure(RD_ARRAYS * 8)) return rc;
    if (int rc = A->rd_status.ensure(n * 4 + 16)) return rc;
    uint64_t *d_counts = A->rd_counts.as<uint64_t>(), *d_begins = A->rd_begins.as<uint64_t>();
    RdBatch b;
    memset(&b, 0, sizeof(b));
    b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
    b.counts = d_counts; b.begins = d_begins; b.status = A->rd_status.as<int32_t>();
    b.n_queries = n; b.stride = stride; b.labeled = A->anno ? 1u : 0u;
    // pass 1: what every query takes in the five arrays (and the zeros that close the scans); the scans give the begins
    HIP_TRY((hipError_t)mgx_launch_decode_size(&b, A->hstream));
    ++g_decode_counts[RD_CNT_SIZE];
    for (int x = 0; x < RD_ARRAYS; ++x) {
        size_t tmp_bytes = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_counts + x * stride, d_begins + x * stride, (int)(n + 1), A->hstream));
        if (int rc = A->scan_tmp.ensure(tmp_bytes + 16)) return rc;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A->scan_tmp.p, tmp_bytes, d_counts + x * stride, d_begins + x * stride, (int)(n + 1), A->hstream));
        // the totals side by side, so that one copy of 40 bytes brings them
        HIP_TRY(hipMemcpyAsync(A->rd_totals.as<uint64_t>() + x, d_begins + x * stride + n, 8, hipMemcpyDeviceToDevice, A->hstream));
    }
    uint64_t total[RD_ARRAYS] = { 0, 0, 0, 0, 0 };
    HIP_TRY(copy_sync(A, total, A->rd_totals.p, sizeof(total), hipMemcpyDeviceToHost));
    g_decode_counts[RD_CNT_D2H_BYTES] += sizeof(total);
    // pass 2: the arrays
    const size_t bytes[mgx_aligner::RD_H_N] = { (size_t)(n + 1) * 8, (size_t)total[RD_ALN] * sizeof(mgx_alignment), (size_t)total[RD_NODES] * 8,
                                                (size_t)total[RD_CIGAR] * sizeof(mgx_cigar_op), (size_t)total[RD_SEQ], (size_t)n * 4,
                                                (size_t)total[RD_LABELS] * 4 };
    size_t all_bytes = 0;
    for (size_t x : bytes) all_bytes += x;
    auto no_buffer = [&](const char *which) {
        return fail(MGX_ERR_OOM, "%s: the results of %llu queries need %llu bytes and no %s buffer of that size could be allocated", fn,
                    (unsigned long long)n, (unsigned long long)all_bytes, which);
    };
    // (16 bytes more than needed: an array without elements still has an address)
    if (A->rd_alns.ensure(bytes[mgx_aligner::RD_H_ALNS] + 16) != MGX_OK || A->rd_nodes.ensure(bytes[mgx_aligner::RD_H_NODES] + 16) != MGX_OK
        || A->rd_cigar.ensure(bytes[mgx_aligner::RD_H_CIGAR] + 16) != MGX_OK || A->rd_seqs.ensure(bytes[mgx_aligner::RD_H_SEQS] + 16) != MGX_OK
        || A->rd_labels.ensure(bytes[mgx_aligner::RD_H_LABELS] + 16) != MGX_OK)
        return no_buffer("device");
    b.alignments = A->rd_alns.as<RdAlignment>(); b.nodes = A->rd_nodes.as<uint64_t>(); b.cigar = A->rd_cigar.as<RdCigarOp>();
    b.seqs = A->rd_seqs.as<char>(); b.labels = A->rd_labels.as<uint32_t>();
    HIP_TRY((hipError_t)mgx_launch_decode_write(&b, A->hstream));
    ++g_decode_counts[RD_CNT_WRITE];
    const void *d_arrays[mgx_aligner::RD_H_N] = { d_begins + RD_ALN * stride, A->rd_alns.p, A->rd_nodes.p, A->rd_cigar.p, A->rd_seqs.p, A->rd_status.p,
                                                  A->rd_labels.p };
    const void *arrays[mgx_aligner::RD_H_N];
    if (where == RD_TO_DEVICE) {
        HIP_TRY(hipStreamSynchronize(A->hstream));       // (the arrays are complete when the call returns, whatever stream reads them)
        for (int x = 0; x < mgx_aligner::RD_H_N; ++x) arrays[x] = d_arrays[x];
    } else {
        for (int x = 0; x < mgx_aligner::RD_H_N; ++x) {
            if (bytes[x] + 1 > A->h_rd_bytes[x]) {
                if (A->h_rd[x]) { (void)hipHostFree(A->h_rd[x]); A->h_rd[x] = nullptr; A->h_rd_bytes[x] = 0; }
                const size_t want = bytes[x] + bytes[x] / 8 + 4096;
                void *p = nullptr;
                if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return no_buffer("pinned host"); }
                A->h_rd[x] = p; A->h_rd_bytes[x] = want;
            }
            if (bytes[x]) HIP_TRY(hipMemcpyAsync(A->h_rd[x], d_arrays[x], bytes[x], hipMemcpyDeviceToHost, A->hstream));
            g_decode_counts[RD_CNT_D2H_BYTES] += bytes[x];
            arrays[x] = A->h_rd[x];
        }
        HIP_TRY(hipStreamSynchronize(A->hstream));
    }
    out->n_queries = n;
    out->aln_begin = static_cast<const uint64_t *>(arrays[mgx_aligner::RD_H_ALN_BEGIN]);
    out->alignments = static_cast<const mgx_alignment *>(arrays[mgx_aligner::RD_H_ALNS]);
    out->nodes = static_cast<const uint64_t *>(arrays[mgx_aligner::RD_H_NODES]);
    out->cigar = static_cast<const mgx_cigar_op *>(arrays[mgx_aligner::RD_H_CIGAR]);
    out->seqs = static_cast<const char *>(arrays[mgx_aligner::RD_H_SEQS]);
    out->status = static_cast<const int32_t *>(arrays[mgx_aligner::RD_H_STATUS]);
    out->labels = total[RD_LABELS] ? static_cast<const uint32_t *>(arrays[mgx_aligner::RD_H_LABELS]) : nullptr;     // (as HostResults::view)
    if (sizes) {
        sizes->n_alignments = total[RD_ALN]; sizes->n_nodes = total[RD_NODES]; sizes->n_cigar = total[RD_CIGAR];
        sizes->n_seq_bytes = total[RD_SEQ]; sizes->n_labels = total[RD_LABELS];
    }
    return MGX_OK;
}

int mgx_decode_results_device(mgx_aligner *A, mgx_results *out, mgx_results_sizes *sizes) {
    if (!A || !out || !sizes) return fail(MGX_ERR_INVALID, "null argument");
    const uint64_t n = A->n_reads;
    memset(sizes, 0, sizeof(*sizes));
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    const bool staged = n ? A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets : A->aligned_empty;
    if (!staged)
        return fail(MGX_ERR_INVALID, "mgx_decode_results_device: no aligned batch on this handle, or another batch was staged after mgx_align_batch_device");
    HIP_TRY(hipSetDevice(A->graph->device));
    if (!n) {
        // no query: aln_begin is its one zero, every other array is empty (and has an address)
        if (int rc = A->rd_begins.ensure(64)) return rc;
        HIP_TRY(hipMemsetAsync(A->rd_begins.p, 0, 64, A->hstream));
        HIP_TRY(hipStreamSynchronize(A->hstream));
        memset(out, 0, sizeof(*out));
        out->aln_begin = A->rd_begins.as<uint64_t>();
        out->alignments = reinterpret_cast<const mgx_alignment *>(A->rd_begins.as<uint64_t>() + 1);
        out->nodes = A->rd_begins.as<uint64_t>() + 1;
        out->cigar = reinterpret_cast<const mgx_cigar_op *>(A->rd_begins.as<uint64_t>() + 1);
        out->seqs = reinterpret_cast<const char *>(A->rd_begins.as<uint64_t>() + 1);
        out->status = reinterpret_cast<const int32_t *>(A->rd_begins.as<uint64_t>() + 1);
        return MGX_OK;
    }
    return decode_on_device(A, RD_TO_DEVICE, out, sizes);
}

int mgx_fetch_results(mgx_aligner *A, mgx_results *out) {
    HostStageTimer t_fetch("fetch_results");
    const uint64_t n = A->n_reads;
    HIP_TRY(hipSetDevice(A->graph->device));
    // the aligned batch is read back below (post-chaining, the capacity retry): only while the staging buffers still hold it —
    // mgx_map_batch on this aligner re-stages them; a caller's device buffers are the caller's to keep until the fetch
    const bool batch_intact = A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets;
    if (A->opt.decode_on_device && n && batch_intact) {
        // the option decode_on_device: the seven arrays come decoded (no records, no stream, no per-element work here)
        A->h_results.clear();                            // (mgx_fetch_seed_info reads the records itself)
        mgx_results_sizes sizes;
        if (int rc = decode_on_device(A, RD_TO_HOST, out, &sizes)) return rc;
        ++g_decode_counts[RD_CNT_FETCHES];
        // the capacity retry tells a queue overflow (final) from an arena overflow by the record: the rare batch with a capacity
        // status brings its records as well
        if (std::find(out->status, out->status + n, (int32_t)MGX_ERR_CAPACITY) != out->status + n) {
            A->h_results.resize(n);
            HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
            g_decode_counts[RD_CNT_D2H_BYTES] += n * sizeof(ReadResult);
        }
    } else {
        A->h_results.resize(n);
        unsigned long long used = 0;
        if (n) {
            HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
            HIP_TRY(copy_sync(A, &used, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
            used = std::min<unsigned long long>(used, A->out_words);
        }
        A->h_stream.resize(used);
        if (used) HIP_TRY(copy_sync(A, A->h_stream.data(), A->stream.p, used * 4, hipMemcpyDeviceToHost));
        A->host.decode(A->h_results.data(), n, A->h_stream.data(), ~0ull, A->anno != nullptr);
        A->host.view(out);
    }
    if (A->cfg.post_chain_alignments && n) {
        // chain_alignments (dbg_aligner.cpp:328-332) on the host: needs the reads of the queries with two or more alignments once
        // more — one transfer of the span of the batch that holds them (none at all when no query has two)
        uint64_t q_lo = n, q_hi = 0;
        for (uint64_t q = 0; q < n; ++q) if (out->aln_begin[q + 1] - out->aln_begin[q] >= 2) { q_lo = std::min(q_lo, q); q_hi = q + 1; }
        if (!batch_intact)
            return fail(MGX_ERR_INVALID, "post_chain_alignments: another batch was staged on this aligner between mgx_align_batch_device and mgx_fetch_results");
        std::vector<uint64_t> offs(n + 1, 0);
        HIP_TRY(copy_sync(A, offs.data(), A->last_d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
        std::vector<char> reads(1);
        uint64_t b0 = 0;
        if (q_lo < q_hi) {
            b0 = offs[q_lo];
            const uint64_t b1 = offs[q_hi];
            reads.resize(b1 - b0 + 1);
            if (b1 > b0) HIP_TRY(copy_sync(A, reads.data(), A->last_d_seqs + b0, b1 - b0, hipMemcpyDeviceToHost));
        }
        mgx_results plain = *out;
        chain_results(plain, reads.data(), offs.data(), A->cfg, A->graph->g.k, &A->host_chained, b0);
        A->host_chained.view(out);
    }
    // reads the batch's limits were too small for: once more, with larger ones (below)
    if (!batch_intact) return MGX_OK;              // (statuses stay: the reads are no longer where they were)
    return retry_capacity_queries(A, A->last_d_seqs, A->last_d_offsets, n, out);
}

int mgx_device_results(mgx_aligner *A, const void **headers, uint64_t *header_bytes, uint64_t *n_queries,
                       const void **stream, uint64_t *stream_words) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    unsigned long long used = 0;
    if (A->n_reads) HIP_TRY(copy_sync(A, &used, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
    used = std::min<unsigned long long>(used, A->out_words);
    *headers = A->results.p; *header_bytes = sizeof(ReadResult); *n_queries = A->n_reads;
    *stream = A->stream.p; *stream_words = used;
    return MGX_OK;
}

uint64_t mgx_device_stream_capacity(const mgx_aligner *A) { return A ? A->out_words : 0; }

struct mgx_raw_store { HostResults host; };

int mgx_results_from_raw(const void *headers, uint64_t n, const uint32_t *stream, uint64_t stream_words,
                         mgx_raw_store **store, mgx_results *out) {
    return mgx_results_from_raw_labeled(headers, n, stream, stream_words, 0, store, out);
}
int mgx_results_from_raw_labeled(const void *headers, uint64_t n, const uint32_t *stream, uint64_t stream_words, int labeled,
                                 mgx_raw_store **store, mgx_results *out) {
    if ((!headers && n) || !store || !out || (!stream && stream_words)) return fail(MGX_ERR_INVALID, "null argument");
    const ReadResult *rr = static_cast<const ReadResult *>(headers);
    auto *S = new mgx_raw_store();
    if (!S->host.decode(rr, n, stream, stream_words, labeled != 0)) {
        delete S;
        return fail(MGX_ERR_INVALID, "a record points outside the stream (%llu words)", (unsigned long long)stream_words);
    }
    S->host.view(out);
    *store = S;
    return MGX_OK;
}

void mgx_raw_store_free(mgx_raw_store *store) { delete store; }

// chain_alignments (aligner_chainer.cpp:555-720) over decoded results — what mgx_fetch_results does itself when the aligner's
// config has post_chain_alignments set; for results decoded elsewhere (mgx_results_from_raw after a gather).  Host code.
int mgx_chain_alignments(const mgx_config *config, uint32_t k, const mgx_results *in, const char *seqs, const uint64_t *offsets,
                         mgx_raw_store **store, mgx_results *out) {
    if (!config || !in || !store || !out || (in->n_queries && (!seqs || !offsets))) return fail(MGX_ERR_INVALID, "null argument");
    if (k < 2) return fail(MGX_ERR_INVALID, "k out of range");
    auto *S = new mgx_raw_store();
    chain_results(*in, seqs, offsets, *config, k, &S->host);
    S->host.view(out);
    *store = S;
    return MGX_OK;
}

// Queries whose per-read arenas overflowed (status MGX_ERR_CAPACITY: the reference has no such limit, its tables grow on the
// heap) are aligned again by a temporary aligner with doubled limits, up to six doublings, and take their place in the
// results — what the C++ adapter (host/hip_dbg_aligner.hpp) did for its callers since round 2, now for every caller of
// mgx_fetch_results / mgx_align_batch (the Python binding and the device-resident batches among them).  What doubling cannot cure stays a capacity status: a query with more
// alignments than the post_chain_alignments queue holds.  (Label-aware alignment: the retry also doubles the label arenas —
// alignments per backtracking, aggregator pool, label queues, label sets; derive_limits' label_scale.)
// The re-alignment itself, for the queries `todo` (ascending) of the batch the device holds: fixed[t] = the results of todo[t]
// where have[t]; h_off = the batch's offsets, h_seq = its bytes from h_off[todo.front()] on (mgx_format_tsv_batch prints from them).
static int realign_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, const std::vector<uint64_t> &todo,
                                    std::vector<HostResults> &fixed, std::vector<uint8_t> &have, std::vector<uint64_t> &h_off,
                                    std::vector<char> &h_seq) {
    // the reads in question, from the batch as the device holds it (the caller's buffers, or the upload of a host batch): ONE
    // transfer of the span of the batch between the first and the last of them
    h_off.resize(n + 1);
    HIP_TRY(copy_sync(A, h_off.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t b0 = h_off[todo.front()], b1 = h_off[todo.back() + 1];
    h_seq.resize(b1 - b0 + 1);
    if (b1 > b0) HIP_TRY(copy_sync(A, h_seq.data(), d_seqs + b0, b1 - b0, hipMemcpyDeviceToHost));
    const char *seqs = h_seq.data();
    auto seq_of = [&](uint64_t q) { return seqs + (h_off[q] - b0); };
    const uint64_t *offsets = h_off.data();
    // results so far, query by query (replaced below)
    fixed.assign(todo.size(), HostResults());
    have.assign(todo.size(), 0);
    mgx_limits lim;
    mgx_aligner_get_limits(A, &lim);
    mgx_aligner *tmp = nullptr;
    struct Guard { mgx_aligner *&p; ~Guard() { if (p) mgx_aligner_destroy(p); } } guard{ tmp };
    std::vector<uint64_t> pending(todo.size());
    for (size_t t = 0; t < todo.size(); ++t) pending[t] = t;
    for (int attempt = 0; attempt < 6 && !pending.empty(); ++attempt) {
        lim.max_query_length = 0;                       // the (smaller) batch sets its own
        lim.max_columns = lim.max_columns * 2;
        lim.max_seeds = std::min<uint32_t>(65535u, lim.max_seeds * 2);
        lim.cell_arena_bytes = lim.cell_arena_bytes * 2;
        if (tmp) { mgx_aligner_destroy(tmp); tmp = nullptr; }
        // (an attempt that fails — out of memory at the inflated limits, say — ends the retry: what the batch and the earlier
        // attempts produced stays valid and is what the caller gets, statuses included)
        if (aligner_create(A->graph, &A->cfg, &lim, A->anno, &tmp) != MGX_OK) break;
        tmp->opt = A->opt; tmp->no_fast = A->no_fast;
        tmp->hstream = A->hstream;                        // (borrowed: the retry runs where the batch ran)
        tmp->retry_capacity = false;
        tmp->label_scale = 2u << attempt;
        std::string blob;
        std::vector<uint64_t> offs(pending.size() + 1, 0);
        for (size_t t = 0; t < pending.size(); ++t) {
            const uint64_t q = todo[pending[t]];
            blob.append(seq_of(q), offsets[q + 1] - offsets[q]);
            offs[t + 1] = blob.size();
        }
        mgx_results sub{};
        if (mgx_align_batch(tmp, blob.data(), offs.data(), pending.size(), 0, &sub) != MGX_OK) break;
        std::vector<uint64_t> again;
        for (size_t t = 0; t < pending.size(); ++t) {
            if (sub.status[t] == MGX_ERR_CAPACITY) {
                // (its queue overflowed this time: final)
                if (!(t < tmp->h_results.size() && tmp->h_results[t].orientation == RR_CAUSE_QUEUE)) again.push_back(pending[t]);
                continue;
            }
            fixed[pending[t]].append_query(sub, t);
            have[pending[t]] = 1;
        }
        pending.swap(again);
        mgx_aligner_get_limits(tmp, &lim);
    }
    return MGX_OK;
}

static int retry_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, mgx_results *out) {
    std::vector<uint64_t> todo;
    // (a query whose post_chain_alignments queue overflowed is flagged by the kernel — RR_CAUSE_QUEUE — and stays a status: no
    // limit cures it, and six rounds of ever larger arenas would be paid for nothing)
    for (uint64_t q = 0; q < n; ++q)
        if (out->status[q] == MGX_ERR_CAPACITY && !(q < A->h_results.size() && A->h_results[q].orientation == RR_CAUSE_QUEUE)) todo.push_back(q);
    if (todo.empty() || !A->retry_capacity || !d_seqs || !d_offsets) return MGX_OK;
    std::vector<HostResults> fixed;
    std::vector<uint8_t> have;
    std::vector<uint64_t> h_off;
    std::vector<char> h_seq;
    if (int rc = realign_capacity_queries(A, d_seqs, d_offsets, n, todo, fixed, have, h_off, h_seq)) return rc;
    bool any = false;
    for (uint8_t h : have) any |= h != 0;
    if (!any) return MGX_OK;
    HostResults merged;
    size_t t = 0;
    for (uint64_t q = 0; q < n; ++q) {
        if (t < todo.size() && todo[t] == q) {
            if (have[t]) { mgx_results v; fixed[t].view(&v); merged.append_query(v, 0); }
            else merged.append_query(*out, q);
            ++t;
        } else merged.append_query(*out, q);
    }
    A->host_retried = std::move(merged);
    A->host_retried.view(out);
    A->hstats.n_capacity_retried = (uint64_t)std::count(have.begin(), have.end(), (uint8_t)1);
    return MGX_OK;
}

int mgx_align_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device, mgx_results *out) {
    if (!out) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = mgx_align_batch_device(A, seqs, offsets, n, on_device)) return rc;
    return mgx_fetch_results(A, out);          // (with the capacity retry)
}

// test hook: keep the per-read seed lists of the next batches (device -> mgx_fetch_seeds)
void mgx_aligner_keep_seeds(mgx_aligner *A, int keep) { A->keep_seeds = keep != 0; }

// per read: num_matches fwd/rc, n_seeds fwd/rc, n_extensions, n_columns (6 x u32), and optionally the seeds
int mgx_fetch_seed_info(mgx_aligner *A, uint32_t *info6, uint32_t *seeds /* [n][2][max_seeds][4] or NULL */, uint32_t *max_seeds_out) {
    const uint64_t n = A->n_reads;
    if (A->h_results.size() != n || n == 0) {
        A->h_results.resize(n);
        if (n) HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < n; ++i) {
        const ReadResult &r = A->h_results[i];
        uint32_t *o = info6 + 6 * i;
        o[0] = r.num_matches_fwd; o[1] = r.num_matches_rc; o[2] = r.n_seeds_fwd; o[3] = r.n_seeds_rc;
        o[4] = r.n_extensions; o[5] = r.n_columns;
    }
    if (max_seeds_out) *max_seeds_out = A->lim.max_seeds;
    if (seeds && A->keep_seeds && n) {
        std::vector<DevSeed> h(n * 2 * (uint64_t)A->lim.max_seeds);
        HIP_TRY(copy_sync(A, h.data(), A->dbg_seeds.p, h.size() * sizeof(DevSeed), hipMemcpyDeviceToHost));
        for (size_t x = 0; x < h.size(); ++x) {
            seeds[4 * x] = h[x].clipping; seeds[4 * x + 1] = h[x].length; seeds[4 * x + 2] = h[x].offset;
            seeds[4 * x + 3] = h[x].offset ? h[x].node : h[x].n_nodes;
        }
    }
    return MGX_OK;
}

int mgx_aligner_stats(const mgx_aligner *A, mgx_stats *out) { *out = A->hstats; return MGX_OK; }
void mgx_kernel_launch_counts(uint64_t *out5) { for (int x = 0; x < 5; ++x) out5[x] = g_kernel_launches[x].load(); }

size_t mgx_format_tsv(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                      int32_t min_path_score, char *buf, size_t buf_len) {
    return mgx_format_tsv_labeled(res, qi, header, query, query_len, min_path_score, nullptr, 0, buf, buf_len);
}
size_t mgx_format_tsv_labeled(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                              int32_t min_path_score, const char *const *label_names, uint32_t n_label_names,
                              char *buf, size_t buf_len) {
    // cli/align.cpp:262-285 + alignment.hpp:426-433; the query is printed normalised (AlignmentResults ctor)
    std::string s(header);
    s += '\t';
    for (size_t i = 0; i < query_len; ++i) {
        int8_t c = (int8_t)query[i];
        s += c >= 0 ? (char)toupper(c) : (char)127;
    }
    if (res->aln_begin[qi] == res->aln_begin[qi + 1]) {
        s += "\t*\t*\t" + std::to_string(min_path_score) + "\t*\t*\t*\n";
    } else {
        static const char ops[] = "SX=DIG";
        for (uint64_t ai = res->aln_begin[qi]; ai < res->aln_begin[qi + 1]; ++ai) {
            const mgx_alignment &a = res->alignments[ai];
            s += a.orientation ? "\t-\t" : "\t+\t";
            s.append(res->seqs + a.seq_begin, a.seq_len);
            s += '\t' + std::to_string(a.score) + '\t' + std::to_string(a.num_matches) + '\t';
            for (uint32_t x = 0; x < a.n_cigar; ++x) {
                const mgx_cigar_op &op = res->cigar[a.cigar_begin + x];
                s += std::to_string(op.len) + ops[op.op];
            }
            s += '\t' + std::to_string(a.offset);
            if (res->labels && a.n_labels) {
                // cli/align.cpp:274-281: the label names (LabelEncoder::decode), joined by ';'
                s += '\t';
                for (uint32_t x = 0; x < a.n_labels; ++x) {
                    const uint32_t lbl = res->labels[a.labels_begin + x];
                    if (x) s += ';';
                    if (label_names && lbl < n_label_names) s += label_names[lbl];
                    else s += std::to_string(lbl);
                }
            }
        }
        s += '\n';
    }
    if (buf && buf_len) {
        size_t nc = std::min(buf_len - 1, s.size());
        memcpy(buf, s.data(), nc);
        buf[nc] = 0;
    }
    return s.size();
}

// ---- the text of a batch, written by kernels: the one host sequence behind mgx_format_tsv_batch, mgx_format_map_batch and
// mgx_format_json_batch.  An entry point checks its arguments and describes its job; format_on_device runs it.
struct FormatJob {
    const char *fn;                                  // the entry point's name, for messages
    const char *oom_advice;                          // the end of the two out-of-memory messages ("" or what the caller can do)
    std::atomic<uint64_t> *size_launches, *write_launches, *d2h_bytes, *h2d_bytes, *host_lines;    // its counters; null: it has none
    int (*launch_size)(const void *, void *);        // the two kernels' launchers ...
    int (*launch_write)(const void *, void *);
    const void *params;                              // ... their TfBatch / MfBatch / JfBatch ...
    char **text;                                     // ... and its `text` field (set here, once the size of the text is known)
    const char *headers;                             // header i of the range: headers[header_offsets[i] .. header_offsets[i + 1])
    const uint64_t *header_offsets;
    uint64_t header_from;                            // header_offsets[0] as the kernels see it: the uploaded bytes start there
    uint64_t first, n, n_batch;                      // queries first .. first + n of the staged batch of n_batch
    // Called once tf_headers, tf_header_offsets, tf_len, tf_begin (and tf_cap, with host_line) are large enough and the headers are
    // on the stream: fills *params but for `text`, uploads the entry point's own tables.
    std::function<int()> bind;
    // The text of a query that the host aligned again: (view of that query's results alone, header, query bytes, their count).
    // None: the formatter leaves no query to the host; no tf_cap, no retry.
    std::function<std::string(const mgx_results &, const char *, const char *, size_t)> host_line;
};

// what a per-query host formatter writes, as a string: size the line, fill it, drop the formatter's NUL
static std::string host_formatted(const std::function<size_t(char *, size_t)> &format) {
    std::string line(format(nullptr, 0) + 1, '\0');
    format(&line[0], line.size());
    line.pop_back();
    return line;
}

static int format_on_device(mgx_aligner *A, const FormatJob &job, mgx_text *out) {
    const uint64_t first = job.first, n = job.n;
    auto count = [](std::atomic<uint64_t> *c, uint64_t by) { if (c) *c += by; };
    auto d2h = [&](void *dst, const void *src, size_t bytes) {
        count(job.d2h_bytes, bytes);
        return copy_sync(A, dst, src, bytes, hipMemcpyDeviceToHost);
    };
    auto h2d = [&](void *dst, const void *src, size_t bytes) {
        count(job.h2d_bytes, bytes);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, A->hstream);
    };
    // the range's headers and their offsets (as the caller counts them: uploaded with every call)
    const uint64_t header_bytes = job.header_offsets[n] - job.header_from;
    if (int rc = A->tf_headers.ensure(header_bytes + 16)) return rc;
    if (int rc = A->tf_header_offsets.ensure((n + 1) * 8)) return rc;
    if (int rc = A->tf_len.ensure((n + 1) * 8)) return rc;
    if (int rc = A->tf_begin.ensure((n + 2) * 8)) return rc;
    if (job.host_line) if (int rc = A->tf_cap.ensure((n + 1) * 4)) return rc;
    if (header_bytes) HIP_TRY(h2d(A->tf_headers.p, job.headers + job.header_from, header_bytes));
    HIP_TRY(h2d(A->tf_header_offsets.p, job.header_offsets, (n + 1) * 8));
    if (int rc = job.bind()) return rc;
    uint64_t *d_len = A->tf_len.as<uint64_t>(), *d_begin = A->tf_begin.as<uint64_t>();
    // pass 1: the line lengths (d_len[n] = 0 closes the scan), the capacity-status queries; the scan gives line_begin
    HIP_TRY(hipMemsetAsync(d_len + n, 0, 8, A->hstream));
    HIP_TRY(hipMemsetAsync(d_begin + n + 1, 0, 8, A->hstream));
    HIP_TRY((hipError_t)job.launch_size(job.params, A->hstream));
    count(job.size_launches, 1);
    auto scan = [&]() -> int {
        size_t tmp_bytes = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_len, d_begin, (int)(n + 1), A->hstream));
        if (int rc = A->scan_tmp.ensure(tmp_bytes + 16)) return rc;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A->scan_tmp.p, tmp_bytes, d_len, d_begin, (int)(n + 1), A->hstream));
        return MGX_OK;
    };
    if (int rc = scan()) return rc;
    uint64_t counters[2] = { 0, 0 };                  // the text's bytes, the capacity-status queries (0 without host_line)
    HIP_TRY(d2h(counters, d_begin + n, 16));
    // the capacity-status queries of the range: aligned again with larger limits, formatted by host_line, their lengths patched in
    std::vector<uint64_t> todo;
    std::vector<std::string> host_lines;
    if (job.host_line && counters[1]) {
        std::vector<uint32_t> cap(counters[1]);
        HIP_TRY(d2h(cap.data(), A->tf_cap.p, cap.size() * 4));
        std::sort(cap.begin(), cap.end());
        for (uint32_t i : cap) todo.push_back(first + i);
        if (!A->retry_capacity)
            return fail(MGX_ERR_CAPACITY, "%s: query %llu (and %llu more) has a capacity status and retry_capacity is off", job.fn,
                        (unsigned long long)todo.front(), (unsigned long long)todo.size() - 1);
        std::vector<HostResults> fixed;
        std::vector<uint8_t> have;
        std::vector<uint64_t> h_off;
        std::vector<char> h_seq;
        if (int rc = realign_capacity_queries(A, A->last_d_seqs, A->last_d_offsets, job.n_batch, todo, fixed, have, h_off, h_seq)) return rc;
        count(job.d2h_bytes, (job.n_batch + 1) * 8 + (h_seq.size() - 1));
        std::vector<uint64_t> patch_len(todo.size());
        host_lines.resize(todo.size());
        for (size_t t = 0; t < todo.size(); ++t) {
            const uint64_t q = todo[t];
            if (!have[t]) return fail(MGX_ERR_CAPACITY, "%s: query %llu keeps its capacity status after the retry", job.fn, (unsigned long long)q);
            mgx_results v;
            fixed[t].view(&v);
            const std::string header(job.headers + job.header_offsets[q - first], job.headers + job.header_offsets[q - first + 1]);
            host_lines[t] = job.host_line(v, header.c_str(), h_seq.data() + (h_off[q] - h_off[todo.front()]), h_off[q + 1] - h_off[q]);
            patch_len[t] = host_lines[t].size();
        }
        A->hstats.n_capacity_retried = todo.size();
        count(job.host_lines, todo.size());
        // (i, length) pairs: the i as 4-byte words behind the 8-byte lengths
        if (int rc = A->tf_patch.ensure(todo.size() * 12 + 16)) return rc;
        uint32_t *d_pq = reinterpret_cast<uint32_t *>(A->tf_patch.as<uint64_t>() + todo.size());
        HIP_TRY(h2d(A->tf_patch.p, patch_len.data(), todo.size() * 8));
        HIP_TRY(h2d(d_pq, cap.data(), todo.size() * 4));
        HIP_TRY((hipError_t)mgx_launch_format_patch(d_len, d_pq, A->tf_patch.as<uint64_t>(), (uint32_t)todo.size(), A->hstream));
        if (int rc = scan()) return rc;
        HIP_TRY(d2h(counters, d_begin + n, 8));
        HIP_TRY(hipStreamSynchronize(A->hstream));   // (patch_len and cap are read by the copies above)
    }
    // pass 2: the text
    const uint64_t text_bytes = counters[0];
    auto no_buffer = [&](const char *which) {
        return fail(MGX_ERR_OOM, "%s: the text of queries %llu .. %llu needs %llu bytes and no %s buffer of that size could be allocated%s", job.fn,
                    (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)text_bytes, which, job.oom_advice);
    };
    if (A->tf_text.ensure(text_bytes + 16) != MGX_OK) return no_buffer("device");
    if (text_bytes + 1 > A->h_text_bytes) {
        if (A->h_text) { (void)hipHostFree(A->h_text); A->h_text = nullptr; A->h_text_bytes = 0; }
        const size_t want = text_bytes + text_bytes / 8 + 4096;
        void *p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            out->text = "";                          // (what it pointed at is freed)
            return no_buffer("pinned host");
        }
        A->h_text = static_cast<char *>(p); A->h_text_bytes = want;
    }
    *job.text = A->tf_text.as<char>();
    HIP_TRY((hipError_t)job.launch_write(job.params, A->hstream));
    count(job.write_launches, 1);
    count(job.d2h_bytes, text_bytes);
    if (text_bytes) HIP_TRY(hipMemcpyAsync(A->h_text, A->tf_text.p, text_bytes, hipMemcpyDeviceToHost, A->hstream));
    HIP_TRY(d2h(A->h_line_begin.data(), d_begin, (n + 1) * 8));
    for (size_t t = 0; t < todo.size(); ++t) memcpy(A->h_text + A->h_line_begin[todo[t] - first], host_lines[t].data(), host_lines[t].size());
    out->text = A->h_text;
    return MGX_OK;
}

// ---- the TSV text of a batch (tsv_format.hpp, mgx_format.hip) ------------------------------------------------------------
enum { TF_CNT_SIZE = 0, TF_CNT_WRITE, TF_CNT_HOST_LINES, TF_CNT_D2H_BYTES };
static std::atomic<uint64_t> g_format_counts[4];        // mgx_format_kernel_launch_counts
void mgx_format_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_format_counts[x].load(); }

int mgx_format_tsv_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, const char *const *label_names,
                         uint32_t n_label_names, mgx_text *out) {
    static_assert(sizeof(TfBatch) == MGX_FORMAT_ARGS_BYTES, "TfBatch differs from what mgx_format.hip takes");
    if (!A || !out || (n_label_names && !label_names)) return fail(MGX_ERR_INVALID, "null argument");
    const uint64_t n = A->n_reads;
    if (n && (!headers || !header_offsets)) return fail(MGX_ERR_INVALID, "null argument");
    if (A->cfg.post_chain_alignments)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_format_tsv_batch: with post_chain_alignments the chained alignments exist on the host only "
                                         "(mgx_fetch_results + mgx_format_tsv print them)");
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    if (!(A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets))
        return fail(MGX_ERR_INVALID, "mgx_format_tsv_batch: no aligned batch on this handle, or another batch was staged after mgx_align_batch_device");
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_tsv_batch: more than 2^31 - 2 queries in a batch");
    HIP_TRY(hipSetDevice(A->graph->device));
    // the label names (uploaded with every call: a few hundred bytes): for the kernels a blob, for the host formatter C strings
    std::string name_blob;
    std::vector<uint32_t> name_begin(1, 0);
    std::vector<const char *> names(n_label_names);
    for (uint32_t j = 0; j < n_label_names; ++j) {
        names[j] = label_names[j] ? label_names[j] : "";
        name_blob += names[j];
        name_begin.push_back((uint32_t)name_blob.size());
    }
    const size_t names_at = (name_blob.size() + 3) & ~(size_t)3;                 // the begins follow the bytes, 4-byte aligned
    TfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_tsv_batch"; job.oom_advice = "";
    job.size_launches = &g_format_counts[TF_CNT_SIZE]; job.write_launches = &g_format_counts[TF_CNT_WRITE];
    job.d2h_bytes = &g_format_counts[TF_CNT_D2H_BYTES]; job.host_lines = &g_format_counts[TF_CNT_HOST_LINES];
    job.launch_size = mgx_launch_format_size; job.launch_write = mgx_launch_format_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets;
    job.n = job.n_batch = n;
    job.bind = [&]() -> int {
        if (int rc = A->tf_names.ensure(names_at + name_begin.size() * 4 + 16)) return rc;
        if (n_label_names) {
            if (!name_blob.empty()) HIP_TRY(hipMemcpyAsync(A->tf_names.p, name_blob.data(), name_blob.size(), hipMemcpyHostToDevice, A->hstream));
            HIP_TRY(hipMemcpyAsync(A->tf_names.as<char>() + names_at, name_begin.data(), name_begin.size() * 4, hipMemcpyHostToDevice, A->hstream));
        }
        memset(&b, 0, sizeof(b));
        b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
        b.seqs = A->last_d_seqs; b.offsets = A->last_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.name_bytes = A->tf_names.as<char>(); b.name_begin = reinterpret_cast<const uint32_t *>(A->tf_names.as<char>() + names_at);
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.cap_list = A->tf_cap.as<uint32_t>(); b.cap_count = reinterpret_cast<unsigned long long *>(A->tf_begin.as<uint64_t>() + n + 1);
        b.n_queries = n; b.n_names = n_label_names; b.min_path_score = A->cfg.min_path_score; b.labeled = A->anno ? 1u : 0u;
        return MGX_OK;
    };
    job.host_line = [&](const mgx_results &v, const char *header, const char *query, size_t qlen) {
        return host_formatted([&](char *buf, size_t buf_len) {
            return mgx_format_tsv_labeled(&v, 0, header, query, qlen, A->cfg.min_path_score, names.data(), n_label_names, buf, buf_len);
        });
    };
    return format_on_device(A, job, out);
}

// ---- the text of `align --map` for a batch (map_format.hpp, mgx_mapfmt.hip) ---------------------------------
enum { MF_CNT_SIZE = 0, MF_CNT_WRITE, MF_CNT_D2H_BYTES, MF_CNT_H2D_BYTES };
static std::atomic<uint64_t> g_mapfmt_counts[4];        // mgx_format_map_kernel_launch_counts
void mgx_format_map_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_mapfmt_counts[x].load(); }

int mgx_format_map_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, int format, double discovery_fraction,
                         mgx_text *out) {
    static_assert(sizeof(MfBatch) == MGX_MAPFMT_ARGS_BYTES, "MfBatch differs from what mgx_mapfmt.hip takes");
    static_assert(MF_NODES == MGX_MAP_FMT_NODES && MF_COUNT_KMERS == MGX_MAP_FMT_COUNT_KMERS && MF_QUERY_PRESENCE == MGX_MAP_FMT_QUERY_PRESENCE
                  && MF_FILTER_PRESENT == MGX_MAP_FMT_FILTER_PRESENT, "map formats");
    if (!A || !out || !headers || !header_offsets) return fail(MGX_ERR_INVALID, "mgx_format_map_batch: null argument");
    if (format != MGX_MAP_FMT_NODES && format != MGX_MAP_FMT_COUNT_KMERS && format != MGX_MAP_FMT_QUERY_PRESENCE && format != MGX_MAP_FMT_FILTER_PRESENT)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: unknown format %d", format);
    if (!A->ms_generation)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: no summary batch staged: mgx_map_summary_batch has not run on this handle");
    if (A->ms_generation != A->stage_generation)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: no summary batch staged: mgx_align_batch_device or mgx_map_batch ran on this "
                                     "handle after mgx_map_summary_batch");
    if (format == MGX_MAP_FMT_NODES && !A->ms_have_nodes)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: MGX_MAP_FMT_NODES needs the node array: run mgx_map_summary_batch with "
                                     "MGX_MAP_KEEP_NODES (or MGX_MAP_WANT_NODES)");
    const uint64_t n = A->n_reads;
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_map_batch: more than 2^31 - 2 queries in a batch");
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const uint32_t k = A->graph->g.k, map_length = A->ms_map_length;
    const bool sub_k = map_length != 0 && map_length < k;
    const uint32_t window = sub_k ? map_length : k;
    // the presence threshold for every k-mer count a read of this batch can have, by mgx_map_present's own expressions (the same
    // compiler, the same flags, the same doubles): the kernels compare integers
    const uint32_t max_kmers = A->ms_lmax >= window ? A->ms_lmax - window + 1 : 0;
    const bool presence = format == MGX_MAP_FMT_QUERY_PRESENCE || format == MGX_MAP_FMT_FILTER_PRESENT;
    std::vector<uint64_t> &threshold = A->h_mf_threshold;
    HIP_TRY(hipStreamSynchronize(A->hstream));       // (no earlier upload still reads the table)
    threshold.assign(presence ? (size_t)max_kmers + 1 : 1, 0);
    if (presence)
        for (size_t n_kmers = 0; n_kmers <= max_kmers; ++n_kmers)
            threshold[n_kmers] = mf_threshold_host(n_kmers, discovery_fraction, sub_k);
    MfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_map_batch"; job.oom_advice = "";
    job.size_launches = &g_mapfmt_counts[MF_CNT_SIZE]; job.write_launches = &g_mapfmt_counts[MF_CNT_WRITE];
    job.d2h_bytes = &g_mapfmt_counts[MF_CNT_D2H_BYTES]; job.h2d_bytes = &g_mapfmt_counts[MF_CNT_H2D_BYTES];
    job.launch_size = mgx_launch_mapfmt_size; job.launch_write = mgx_launch_mapfmt_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets;
    job.n = job.n_batch = n;
    job.bind = [&]() -> int {
        if (int rc = A->mf_threshold.ensure(threshold.size() * 8)) return rc;
        g_mapfmt_counts[MF_CNT_H2D_BYTES] += threshold.size() * 8;
        HIP_TRY(hipMemcpyAsync(A->mf_threshold.p, threshold.data(), threshold.size() * 8, hipMemcpyHostToDevice, A->hstream));
        memset(&b, 0, sizeof(b));
        b.counts = A->ms_counts.as<uint32_t>(); b.nodes = A->ms_nodes.as<uint64_t>(); b.node_begin = A->node_begin.as<uint64_t>();
        b.seqs = A->ms_d_seqs; b.offsets = A->ms_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.threshold = A->mf_threshold.as<uint64_t>();
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.n_queries = n; b.max_kmers = presence ? max_kmers : 0; b.k = k; b.window = window; b.sub_k = sub_k ? 1u : 0u; b.format = format;
        return MGX_OK;
    };
    return format_on_device(A, job, out);            // (no host_line: this formatter leaves no line to the host)
}

// ---- metagraph align --json (cli/align.cpp:287-305): Alignment::to_json (alignment.cpp:883-963) + path_json (:704-881),
// written the way Json::writeString does with indentation "" (jsoncpp: object keys in lexicographic order, no white
// space, doubles as %.17g with ".0" appended to integral values, strings with the standard escapes).
namespace {
void json_string(std::string &o, const char *p, size_t n) {
    o += '"';
    for (size_t i = 0; i < n; ++i) {
        const unsigned char c = (unsigned char)p[i];
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20 || c >= 0x7F) { char b[8]; snprintf(b, sizeof(b), "\\u%04X", (unsigned)c); o += b; }
                else o += (char)c;
        }
    }
    o += '"';
}
void json_double(std::string &o, double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    o += b;
    if (!strpbrk(b, ".eEn")) o += ".0";
}
// one edit object: keys from_length, sequence, to_length (only those set)
void json_edit(std::string &o, bool &first, long long from_len, const char *seq, size_t seq_len, long long to_len) {
    if (!first) o += ',';
    first = false;
    o += '{';
    bool f2 = true;
    if (from_len >= 0) { o += "\"from_length\":" + std::to_string(from_len); f2 = false; }
    if (seq) { if (!f2) o += ','; o += "\"sequence\":"; json_string(o, seq, seq_len); f2 = false; }
    if (to_len >= 0) { if (!f2) o += ','; o += "\"to_length\":" + std::to_string(to_len); }
    o += '}';
}
}  // namespace

size_t mgx_format_json(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                       uint32_t k, char *buf, size_t buf_len) {
    // the query as AlignmentResults keeps it (alignment.cpp:1348-1372): upper case, bytes < 0 -> 127; and its reverse
    // complement (COMPL_TAB, reverse_complement.hpp:31-62)
    std::string fwd(query_len, 0), rc(query_len, 0);
    for (size_t i = 0; i < query_len; ++i) {
        const int8_t c = (int8_t)query[i];
        fwd[i] = c >= 0 ? (char)toupper(c) : (char)127;
    }
    for (size_t i = 0; i < query_len; ++i) {
        const unsigned char c = (unsigned char)fwd[query_len - 1 - i];
        static const char up[] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
        rc[i] = (c >= 'A' && c <= 'Z') ? up[c - 'A'] : (c >= 'a' && c <= 'z') ? (char)(up[c - 'a'] + 32) : c == 96 ? (char)64 : (char)c;
    }
    std::string s;
    const size_t hl = strlen(header);
    if (res->aln_begin[qi] == res->aln_begin[qi + 1]) {
        // Alignment().to_json: an empty alignment carries its name and an empty sequence
        s += "{\"name\":"; json_string(s, header, hl); s += ",\"sequence\":\"\"}\n";
    }
    for (uint64_t ai = res->aln_begin[qi]; ai < res->aln_begin[qi + 1]; ++ai) {
        const mgx_alignment &a = res->alignments[ai];
        const bool secondary = ai != res->aln_begin[qi];
        const std::string &full = a.orientation ? rc : fwd;
        const char *qv = full.data() + a.clipping;                     // query_view_
        const size_t qv_len = query_len - a.clipping - a.end_clipping;
        const mgx_cigar_op *cg = res->cigar + a.cigar_begin;
        // mgx_cigar_op.op: 0 clipped, 1 mismatch, 2 match, 3 deletion, 4 insertion, 5 node insertion (aligner_cigar.hpp:19-26)
        static const char opc[] = "SX=DIG";
        s += "{\"annotation\":{\"cigar\":\"";
        for (uint32_t x = 0; x < a.n_cigar; ++x) s += std::to_string(cg[x].len) + opc[cg[x].op];
        s += '"';
        if (a.seq_len) { s += ",\"ref_sequence\":"; json_string(s, res->seqs + a.seq_begin, a.seq_len); }
        s += "},\"identity\":";
        json_double(s, qv_len ? (double)a.num_matches / (double)qv_len : 0.0);
        if (secondary) s += ",\"is_secondary\":true";
        s += ",\"name\":"; json_string(s, header, hl);
        if (a.n_nodes) {
            // path_json: mappings of the first node (may cover up to node_size characters), then one per further node
            const uint64_t *nodes = res->nodes + a.nodes_begin;
            uint32_t ci = 0;
            if (a.n_cigar && cg[0].op == 0) ++ci;
            uint64_t c_off = 0;
            const char *qs = qv;
            s += ",\"path\":{";
            if (nodes[0] == nodes[a.n_nodes - 1]) s += "\"is_circular\":true,";
            s += "\"length\":" + std::to_string(a.n_nodes) + ",\"mapping\":[";
            long long rank = 1;
            size_t cur = a.offset;
            {
                s += "{\"edit\":[";
                bool first = true;
                while (cur < k && ci < a.n_cigar) {
                    size_t next_pos = std::min<size_t>(k, cur + (cg[ci].len - c_off));
                    const size_t next_size = next_pos - cur;
                    const uint32_t op = cg[ci].op;
                    if (op == 0) { ++ci; c_off = 0; continue; }               // trailing clip
                    if (op == 1) { json_edit(s, first, (long long)next_size, qs, next_size, (long long)next_size); qs += next_size; }
                    else if (op == 4) { json_edit(s, first, -1, qs, next_size, (long long)next_size); qs += next_size; next_pos = cur; }
                    else if (op == 3) json_edit(s, first, (long long)next_size, nullptr, 0, -1);
                    else if (op == 2) { json_edit(s, first, (long long)next_size, nullptr, 0, (long long)next_size); qs += next_size; }
                    c_off += next_size;
                    cur = next_pos;
                    if (c_off == cg[ci].len) { ++ci; c_off = 0; }
                }
                s += "],\"position\":{\"node_id\":" + std::to_string(nodes[0]);
                if (a.offset) s += ",\"offset\":" + std::to_string(a.offset);
                s += "},\"rank\":" + std::to_string(rank++) + "}";
            }
            for (uint32_t ni = 1; ni < a.n_nodes && ci < a.n_cigar; ++ni) {
                s += ",{\"edit\":[";
                bool first = true;
                if (cg[ci].op == 4 || cg[ci].op == 0) {
                    const size_t len = cg[ci].len - c_off;
                    json_edit(s, first, -1, qs, len, (long long)len);
                    qs += len;
                    ++ci; c_off = 0;
                }
                if (ci < a.n_cigar) {
                    const uint32_t op = cg[ci].op;
                    if (op == 1) { json_edit(s, first, 1, qs, 1, 1); ++qs; }
                    else if (op == 3) json_edit(s, first, 1, nullptr, 0, -1);
                    else if (op == 2) { json_edit(s, first, 1, nullptr, 0, 1); ++qs; }
                    if (++c_off == cg[ci].len) { c_off = 0; ++ci; }
                }
                s += "],\"position\":{\"node_id\":" + std::to_string(nodes[ni]) + ",\"offset\":" + std::to_string(k - 1);
                s += "},\"rank\":" + std::to_string(rank++) + "}";
            }
            s += "],\"name\":\"\"}";
        }
        if (a.clipping) s += ",\"query_position\":" + std::to_string(a.clipping);
        s += std::string(",\"read_mapped\":") + (qv_len ? "true" : "false");
        if (a.orientation) s += ",\"read_on_reverse_strand\":true";
        s += ",\"score\":" + std::to_string(a.score);
        s += ",\"sequence\":"; json_string(s, full.data(), full.size());
        if (a.clipping) s += ",\"soft_clipped\":true";
        s += "}\n";
    }
    if (buf && buf_len) {
        size_t nc = std::min(buf_len - 1, s.size());
        memcpy(buf, s.data(), nc);
        buf[nc] = 0;
    }
    return s.size();
}

// ---- the `align --json` text of a range of a batch (json_format.hpp, mgx_jsonfmt.hip) -------------------------
enum { JF_CNT_SIZE = 0, JF_CNT_WRITE, JF_CNT_HOST_QUERIES, JF_CNT_D2H_BYTES };
static std::atomic<uint64_t> g_jsonfmt_counts[4];       // mgx_format_json_kernel_launch_counts
void mgx_format_json_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_jsonfmt_counts[x].load(); }

int mgx_format_json_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, uint64_t first, uint64_t n, mgx_text *out) {
    static_assert(sizeof(JfBatch) == MGX_JSONFMT_ARGS_BYTES, "JfBatch differs from what mgx_jsonfmt.hip takes");
    if (!A || !out || (n && (!headers || !header_offsets))) return fail(MGX_ERR_INVALID, "mgx_format_json_batch: null argument");
    if (A->cfg.post_chain_alignments)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_format_json_batch: post_chain_alignments is set and JSON output for chains is not supported");
    const uint64_t n_batch = A->n_reads;
    if (first > n_batch || n > n_batch - first)
        return fail(MGX_ERR_INVALID, "mgx_format_json_batch: queries %llu .. %llu are beyond the staged batch of %llu", (unsigned long long)first,
                    (unsigned long long)(first + n), (unsigned long long)n_batch);
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    if (!(A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets))
        return fail(MGX_ERR_INVALID, "mgx_format_json_batch: no alignment batch staged: mgx_align_batch_device has not run on this handle, or a "
                                     "map / summary call ran since");
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_json_batch: more than 2^31 - 2 queries in a range");
    HIP_TRY(hipSetDevice(A->graph->device));
    const uint32_t k = A->graph->g.k;
    JfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_json_batch"; job.oom_advice = ": take a smaller range";
    job.size_launches = &g_jsonfmt_counts[JF_CNT_SIZE]; job.write_launches = &g_jsonfmt_counts[JF_CNT_WRITE];
    job.d2h_bytes = &g_jsonfmt_counts[JF_CNT_D2H_BYTES]; job.host_lines = &g_jsonfmt_counts[JF_CNT_HOST_QUERIES];
    job.launch_size = mgx_launch_jsonfmt_size; job.launch_write = mgx_launch_jsonfmt_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets; job.header_from = header_offsets[0];    // (the kernels subtract it)
    job.first = first; job.n = n; job.n_batch = n_batch;
    job.bind = [&]() -> int {
        memset(&b, 0, sizeof(b));
        b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
        b.seqs = A->last_d_seqs; b.offsets = A->last_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_from = job.header_from; b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.cap_list = A->tf_cap.as<uint32_t>(); b.cap_count = reinterpret_cast<unsigned long long *>(A->tf_begin.as<uint64_t>() + n + 1);
        b.first = first; b.n_queries = n; b.k = k; b.labeled = A->anno ? 1u : 0u;
        return MGX_OK;
    };
    job.host_line = [&](const mgx_results &v, const char *header, const char *query, size_t qlen) {
        return host_formatted([&](char *buf, size_t buf_len) { return mgx_format_json(&v, 0, header, query, qlen, k, buf, buf_len); });
    };
    return format_on_device(A, job, out);
}

} // extern "C"
