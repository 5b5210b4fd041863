// mgx_map.hip — reads to graph nodes: the mapping kernels (k_kmer_counts, k_pack_reads, k_map, k_map_packed, k_map_pipe,
// k_canon_merge) with the host code that stages a batch and sizes and launches them (stage_batch, run_map), and the two entry
// points that hand the mapping itself to the caller (mgx_map_batch, mgx_map_summary_batch).
#include <hip/hip_runtime.h>
#include "pack_swar.hpp"

#include <atomic>

#define MGX_NO_EXTEND 1      // the mapping kernels use the graph primitives only
#include "graph_build.hpp"
#include "map_pipe.hpp"
#include "host_state.hpp"
#include "kernel_units.hpp"

using namespace mgx;

// =================================================================================================
// kernels
// =================================================================================================
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
#define MGX_MAP_BLOCKS_PER_CU 8         // 256-thread blocks resident per CU (8 = 32 waves: full occupancy if registers allow)
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

// =================================================================================================
// host side
// =================================================================================================
hipError_t load_map_kernels() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_map));
}

int stage_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device,
                const char **d_seqs, const uint64_t **d_offsets, uint32_t *Lmax_out, uint32_t window) {
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
    if (int rc = exclusive_sum(A, A->counts.as<uint64_t>(), A->node_begin.as<uint64_t>(), n + 1)) return rc;
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

int run_map(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, bool do_rc, bool mapped, uint32_t Lmax, bool raw_edges) {
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

extern "C" {

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

} // extern "C"
