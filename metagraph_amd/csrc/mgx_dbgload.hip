// mgx_dbgload.hip — `.dbg` files decoded on the device: mgx_graph_load_dbg_device and the test hook mgx_boss_file_decode_device
// (include/mgx.h, "files").  The host reads the file and walks the container headers (dbg_plan.hpp: parse_dbg's own Cursor,
// skip functions, checks and messages); every payload goes, as it stands in the file, into a device buffer of its own and the
// kernels below (bodies: dbg_decode.hpp) decode W and last into the byte arrays of mgx_boss_view, which mgx_graph_create takes
// with on_device = 1.  DESIGN 3.16.
//
// Shapes: one lane per item everywhere (an rrr block, an output word, an element of W, eight bytes of last, a word of an
// sd_vector's high part, a set bit).  k_rrr_block and k_wt_decode keep their table (the binomials, 15.8 KB; the tree's nodes,
// at most 12 KB) in LDS and stride over the items with a bounded grid so that a workgroup fills it once for many items.  Scans:
// hipcub, 64-bit, on the null stream like everything here (the loader runs before any aligner exists).  No atomics on data; the
// error record is one atomicMin word.
#include <memory>
#include <new>

#include "dbg_kernels.hpp"

// =================================================================================================
// kernels (the shared ones: dbg_kernels.hpp)
// =================================================================================================
__global__ void __launch_bounds__(256) k_wt_decode(const uint64_t *bv, const uint64_t *dir, uint64_t bits, const DdRawNode *raw, uint32_t n_nodes,
                                                   uint32_t alphabet2, uint8_t *W, uint64_t n, uint64_t *err) {
    __shared__ DdNode nodes[DD_MAX_NODES];
    for (uint32_t x = threadIdx.x; x < n_nodes; x += blockDim.x) nodes[x] = dd_wt_node(raw[x], bv, dir, bits);
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        W[i] = dd_wt_decode(bv, dir, bits, nodes, n_nodes, alphabet2, i, err);
}

__global__ void __launch_bounds__(256) k_unpack_int(const uint64_t *w, uint32_t width, uint32_t alphabet2, uint8_t *W, uint64_t n, uint64_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) W[i] = dd_unpack_int(w, width, alphabet2, i, err);
}

__global__ void __launch_bounds__(256) k_expand_bits(const uint64_t *w, uint64_t bits, uint64_t *out8, uint64_t n_lanes) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_lanes) out8[t] = dd_expand8(w, bits, t);
}

__global__ void __launch_bounds__(256) k_sd_word(const uint64_t *high, uint64_t high_bits, const uint64_t *rank, const uint64_t *low, uint64_t low_n,
                                                 uint32_t wl, uint64_t *pos, uint64_t m, uint64_t n_words, uint64_t *err, uint32_t check_select) {
    const uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi < n_words) dd_sd_word(high, high_bits, rank, low, low_n, wl, wi, pos, m, err, check_select);
}

__global__ void __launch_bounds__(256) k_sd_scatter(const uint64_t *pos, uint64_t m, uint64_t size, uint8_t *out, int inverted, uint64_t *err,
                                                    uint32_t check_order) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) dd_sd_scatter(pos, i, size, out, inverted != 0, err, check_order);
}

// =================================================================================================
// host
// =================================================================================================
namespace {

int expand_bits(const uint64_t *w, uint64_t bits, DBuf &out) {
    TRY_D(out.alloc(dd_byte_alloc(bits)));
    const uint64_t lanes = (bits + 7) / 8;
    k_expand_bits<<<grid_for(lanes), 256>>>(w, bits, out.as<uint64_t>(), lanes);
    LAUNCHED(1);
    return MGX_OK;
}

int decode_stat_last(const StatPlan &s, uint64_t *err, DBuf &out) {
    DBuf v, dir;
    TRY_D(upload(v, s.v));
    TRY_D(rank_directory(v.as<uint64_t>(), s.v.bits, dir));
    k_check_total<<<1, 64>>>(dir.as<uint64_t>() + s.v.words(), s.ones, DD_L_ONES, err);
    LAUNCHED(1);
    return expand_bits(v.as<uint64_t>(), s.v.bits, out);
}

int decode_sd_last(const SdPlan &s, uint64_t *err, DBuf &out) {
    DBuf low, high, rank, pos;
    TRY_D(upload(low, s.low));
    TRY_D(upload(high, s.high));
    TRY_D(rank_directory(high.as<uint64_t>(), s.high.bits, rank));
    uint64_t m = 0;
    TRY_D(d2h(&m, rank.as<uint64_t>() + s.high.words(), 8));                    // (a scan total: it sizes pos)
    if (m != s.ones || s.zeros != s.high.bits - m || s.low.size() < m) {
        k_fail<<<1, 64>>>(err, DD_L_SD_SELECT, m);                                // the host's check of the total, into the same record
        LAUNCHED(1);
        return MGX_OK;
    }
    TRY_D(pos.alloc(m * 8));
    TRY_D(out.alloc(dd_byte_alloc(s.size)));
    HIP_TRY_D(hipMemset(out.p, 0, dd_byte_alloc(s.size)));
    if (s.inverted && s.size) HIP_TRY_D(hipMemset(out.p, 1, s.size));
    if (!m) return MGX_OK;
    const uint64_t nw = s.high.words();
    k_sd_word<<<grid_for(nw), 256>>>(high.as<uint64_t>(), s.high.bits, rank.as<uint64_t>(), low.as<uint64_t>(), s.low.size(), s.wl,
                                     pos.as<uint64_t>(), m, nw, err, DD_L_SD_SELECT);
    LAUNCHED(1);
    k_sd_scatter<<<grid_for(m), 256>>>(pos.as<uint64_t>(), m, s.size, out.as<uint8_t>(), s.inverted ? 1 : 0, err, DD_L_SD_ORDER);
    LAUNCHED(1);
    return MGX_OK;
}

int decode_W(const DbgPlan &p, Tables &t, uint64_t *err, DBuf &W) {
    const uint32_t alphabet2 = 2 * p.head.sigma;
    TRY_D(W.alloc(dd_byte_alloc(p.w_size)));
    if (p.w_kind == W_INT_VECTOR) {
        DBuf iv;
        TRY_D(upload(iv, p.w_bv));
        k_unpack_int<<<grid_for(p.w_size), 256>>>(iv.as<uint64_t>(), p.w_bv.width, alphabet2, W.as<uint8_t>(), p.w_size, err);
        LAUNCHED(1);
        return MGX_OK;
    }
    DBuf bv, dir, nodes;
    if (p.w_kind == W_TREE_RRR) TRY_D(decode_rrr(p.w_rrr, t, err, DD_W_RRR_EARLY, bv));
    else TRY_D(upload(bv, p.w_bv));
    const uint64_t bits = p.level_bits();
    TRY_D(rank_directory(bv.as<uint64_t>(), bits, dir));
    if (p.w_kind == W_TREE_PLAIN) {
        k_check_total<<<1, 64>>>(dir.as<uint64_t>() + (bits + 63) / 64, p.w_ones, DD_W_SELECT, err);
        LAUNCHED(1);
    }
    std::vector<DdRawNode> raw(p.nodes.size());
    for (size_t x = 0; x < raw.size(); ++x) raw[x] = DdRawNode{ p.nodes[x].bv_pos, p.nodes[x].bv_pos_rank, { p.nodes[x].child[0], p.nodes[x].child[1] }, 0 };
    TRY_D(nodes.alloc(raw.size() * sizeof(DdRawNode)));
    TRY_D(h2d(nodes.p, raw.data(), raw.size() * sizeof(DdRawNode)));
    k_wt_decode<<<grid_for(p.w_size, 4096), 256>>>(bv.as<uint64_t>(), dir.as<uint64_t>(), bits, nodes.as<DdRawNode>(), (uint32_t)raw.size(), alphabet2,
                                                   W.as<uint8_t>(), p.w_size, err);
    LAUNCHED(1);
    return MGX_OK;
}

struct Decoded {
    BossFile head;
    DBuf W, last;                        // n_edges + 1 bytes each, on `device`
};

template <class F>
int guarded(const char *path, F &&f) {
    try {
        return f();
    } catch (const Unsupported &e) {
        return dfail(MGX_ERR_UNSUPPORTED, "%s: %s", path, e.what());
    } catch (const ParseError &e) {
        return dfail(MGX_ERR_INVALID, "%s: %s", path, e.what());
    } catch (const std::bad_alloc &) {
        return dfail(MGX_ERR_OOM, "%s: out of host memory", path);
    }
}

// the file's W and last in device memory.  dna_only: mgx_graph_load_dbg's refusal of other alphabets, before the device is touched
int decode_file(const char *path, int device, bool dna_only, Decoded *out) {
    return guarded(path, [&]() -> int {
        const std::vector<uint8_t> image = read_whole_file(path);
        const DbgPlan p = plan_dbg(image.data(), image.size());
        if (dna_only && p.head.sigma != 5)
            return dfail(MGX_ERR_UNSUPPORTED, "%s: alphabet of %u characters; the device index holds DNA ($ACGT) graphs only", path, p.head.sigma);
        if (mgx_device_count() <= device || device < 0) return dfail(MGX_ERR_NO_DEVICE, "HIP device %d not available", device);
        HIP_TRY_D(hipSetDevice(device));
        out->head = p.head;
        const uint64_t n = p.w_size;
        if (p.host_decode) {                                     // (a node table that is no tree: the host decoder, then a plain upload)
            const BossFile g = parse_dbg(image.data(), image.size());
            TRY_D(out->W.alloc(n));
            TRY_D(out->last.alloc(n));
            TRY_D(h2d(out->W.p, g.W.data(), n));
            return h2d(out->last.p, g.last.data(), n);
        }
        DBuf err;
        Tables tables;
        TRY_D(err.alloc(8));
        HIP_TRY_D(hipMemset(err.p, 0xFF, 8));
        uint64_t *e = err.as<uint64_t>();
        TRY_D(decode_W(p, tables, e, out->W));
        if (p.last_code == CODE_RRR) {
            DBuf bits;
            TRY_D(decode_rrr(p.l_rrr, tables, e, DD_L_RRR_EARLY, bits));
            TRY_D(expand_bits(bits.as<uint64_t>(), p.l_rrr.bits, out->last));
        } else if (p.last_code == CODE_SD) TRY_D(decode_sd_last(p.l_sd, e, out->last));
        else TRY_D(decode_stat_last(p.l_stat, e, out->last));
        uint64_t key = DD_NO_ERROR;
        TRY_D(d2h(&key, e, 8));                                  // (synchronises with the kernels)
        if (key != DD_NO_ERROR)
            return dfail(MGX_ERR_INVALID, "%s: %s (at %llu)", path, dd_check_message((uint32_t)(key >> 48)), (unsigned long long)(key & ((1ull << 48) - 1)));
        return MGX_OK;
    });
}

}  // namespace

extern "C" {

void mgx_dbg_decode_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_counts[x].load(); }

int mgx_boss_file_decode_device(const char *path, int device, mgx_boss_file *out) {
    if (!path || !out) return dfail(MGX_ERR_INVALID, "mgx_boss_file_decode_device: bad arguments");
    memset(out, 0, sizeof(*out));
    Decoded d;
    if (int rc = decode_file(path, device, false, &d)) return rc;
    return guarded(path, [&]() -> int {
        std::unique_ptr<BossFile> g(new BossFile(d.head));
        g->W.resize(g->n_edges + 1);
        g->last.resize(g->n_edges + 1);
        TRY_D(d2h(g->W.data(), d.W.p, g->W.size()));
        TRY_D(d2h(g->last.data(), d.last.p, g->last.size()));
        out->k = g->k; out->sigma = g->sigma; out->mode = g->mode; out->state = g->state; out->n_edges = g->n_edges;
        out->F = g->F.data(); out->W = g->W.data(); out->last = g->last.data();
        out->owner = g.release();
        return (int)MGX_OK;
    });
}

int mgx_graph_load_dbg_device(const char *path, int device, mgx_graph **out) {
    if (!path || !out) return dfail(MGX_ERR_INVALID, "mgx_graph_load_dbg_device: bad arguments");
    Decoded d;
    if (int rc = decode_file(path, device, true, &d)) return rc;
    mgx_boss_view view;
    memset(&view, 0, sizeof(view));
    view.k = d.head.k; view.sigma = 5; view.n_edges = d.head.n_edges; view.W = d.W.as<uint8_t>(); view.last = d.last.as<uint8_t>();
    view.F = d.head.F.data(); view.mode = d.head.mode; view.on_device = 1;
    return mgx_graph_create(&view, device, out);       // its message stays in mgx_last_error; W and last are released on return
}

}  // extern "C"
