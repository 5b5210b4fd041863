// mgx_graph.hip — the device index of a BOSS graph: the index-build kernels (graph_build.hpp) with mgx_graph_create, which sizes
// and launches them, and the two label tables that label-aware aligners derive from the whole graph (k_canon_repr,
// k_anno_dummy_rows), computed once per graph and kept with it.
#include <hip/hip_runtime.h>
#include "pack_swar.hpp"

#include <memory>

#define MGX_NO_EXTEND 1      // the builders use the graph primitives only
#include "graph_build.hpp"
#include "host_state.hpp"
#include "kernel_units.hpp"

using namespace mgx;

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

// label-aware alignment on a CANONICAL-mode graph: node -> the representative of its k-mer (canon_repr_node), whose row holds
// the node's labels
__global__ void k_canon_repr(DevGraph g, uint32_t *out) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > g.n) return;
    out[v] = v ? canon_repr_node(g, v) : 0u;
}

// label-aware alignment: does any dummy node (W == 0: the reference's AnnotationBuffer gives those no labels whatever their row
// says, annotation_buffer.cpp:64-68) have a label in the matrix?  Checked once per graph and annotation; if none does —
// annotations are built from real k-mers — the kernels skip the W look-up in front of every row access.
__global__ void k_anno_dummy_rows(DevGraph g, const uint64_t *head, uint64_t n_rows, uint32_t *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (v > g.n || v - 1 >= n_rows || head[v - 1] == 0) return;
    LineCtr lc = { 0, 0, 0 };
    if (get_W(g, v, lc) == 0) atomicOr(flag, 1u);
}

// =================================================================================================
// host side
// =================================================================================================
int graph_dummy_rows_clean(const mgx_graph *g, const mgx_annotation *anno, bool *clean) {
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
    *clean = it->second;
    return MGX_OK;
}

int graph_canon_repr(const mgx_graph *g) {
    std::lock_guard<std::mutex> lock(g->label_mu);
    if (g->canon_repr_ready) return MGX_OK;
    if (int rc = g->canon_repr.ensure((g->g.n + 1) * 4)) return rc;
    k_canon_repr<<<(uint32_t)((g->g.n + 256) / 256), 256>>>(g->g, g->canon_repr.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    g->canon_repr_ready = true;
    return MGX_OK;
}

extern "C" {

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
    // the code objects a batch launches first, onto this device now (host_state.hpp, load_map_kernels)
    HIP_TRY(load_map_kernels());
    HIP_TRY((hipError_t)mgx_seed_load());
    HIP_TRY(load_sort_kernels());
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

} // extern "C"
