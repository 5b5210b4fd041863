// mgx_mapsum.hip — `metagraph align --map` on the device (map_summary.hpp): the per-read counts of DeBruijnGraph::map_to_nodes
// from the mapping kernels' node arrays (k_map_summary), the windows of --align-length L < k (k_map_subk), and the host-side
// presence rule and text of cli/align.cpp:91-173 (mgx_map_present, mgx_format_map; no GPU).
//
// Shapes.  k_map_summary: one wavefront per read; the short form (n <= MS_SHORT_MAX k-mers) runs four reads per 256-thread
// workgroup with 1 KiB of LDS each, the long form one read per 64-thread workgroup with a 16 KiB chunk buffer and the read's
// row of a global scratch array.  A launch takes the reads of its form and skips the others, so a batch with long reads is
// two launches.  k_map_subk: one wavefront per read, the lanes take neighbouring windows (their characters and, mostly, their
// BOSS ranges' block lines are the same cache lines).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#define mgx mgx_mapsum_ns
#include "wave.hpp"
#include "map_summary.hpp"
#include "kernel_units.hpp"
#include "../../include/mgx.h"

using namespace mgx;

static_assert(sizeof(MsCounts) == sizeof(mgx_map_counts) && sizeof(MsCounts) == 12, "the device record is the C-ABI's");
static_assert(MS_MODE_BASIC == MGX_MODE_BASIC && MS_MODE_CANONICAL == MGX_MODE_CANONICAL && MS_MODE_PRIMARY == MGX_MODE_PRIMARY, "graph modes");

struct MapSumArgs {
    const uint64_t *node_begin;
    const uint32_t *fwd, *rc;
    uint32_t *sorted;                // long form: total k-mers words
    MsCounts *counts;
    uint64_t *out_nodes;             // null: counts only
    const uint64_t *valid;
    uint64_t n_reads;
    uint32_t n_edges;
    int mode;
};

template <bool LONG>
__global__ void __launch_bounds__(LONG ? 64 : 256) k_map_summary(MapSumArgs a) {
    __shared__ uint32_t s_buf[LONG ? MS_CHUNK : 4 * MS_SHORT_MAX];
    const int wave = (int)(threadIdx.x >> 6);
    uint32_t *buf = s_buf + wave * MS_SHORT_MAX;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t read = (((uint64_t)blockIdx.x * blockDim.x) >> 6) + (uint64_t)wave; read < a.n_reads; read += n_waves) {
        const uint64_t nb = uni(gld(a.node_begin + read));
        const int32_t n = (int32_t)(uni(gld(a.node_begin + read + 1)) - nb);
        if ((n > MS_SHORT_MAX) != LONG) continue;
        MsRead r = { a.fwd + nb, a.rc + nb, n, a.mode, a.n_edges, a.valid };
        uint64_t *out = a.out_nodes ? a.out_nodes + nb : nullptr;
        MsCounts c;
        if constexpr (LONG) c = ms_summary_long(r, buf, a.sorted + nb, out);
        else c = ms_summary_short(r, buf, out);
        if ((threadIdx.x & 63) == 0) {
            MsCounts *d = a.counts + read;
            gst(&d->n_discovered, c.n_discovered); gst(&d->n_kmers, c.n_kmers); gst(&d->n_unique, c.n_unique);
        }
    }
}

__global__ void __launch_bounds__(256) k_map_subk(DevGraph g, const char *seqs, const uint64_t *offsets, const uint64_t *node_begin,
                                                  uint32_t *nodes, uint64_t n_reads, int32_t len) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = (int)(threadIdx.x & 63);
    LineCtr ctr = { 0, 0, 0 };
    for (uint64_t read = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; read < n_reads; read += n_waves) {
        const uint64_t off = gld(offsets + read), nb = gld(node_begin + read);
        const int32_t n = (int32_t)(gld(node_begin + read + 1) - nb);          // windows: L - len + 1, or none
        for (int32_t i = lane; i < n; i += 64) gst(nodes + nb + i, ms_subk_node(g, seqs + off + i, len, ctr));
    }
}

extern "C" {

int mgx_launch_map_summary(const uint64_t *node_begin, const uint32_t *fwd, const uint32_t *rc, uint32_t *sorted, void *counts,
                           uint64_t *out_nodes, const uint64_t *valid, uint64_t n_reads, uint32_t n_edges, int mode, int long_form,
                           void *stream) {
    if (!n_reads) return 0;
    MapSumArgs a = { node_begin, fwd, rc, sorted, static_cast<MsCounts *>(counts), out_nodes, valid, n_reads, n_edges, mode };
    if (long_form) k_map_summary<true><<<(uint32_t)(n_reads < 2048 ? n_reads : 2048), 64, 0, (hipStream_t)stream>>>(a);
    else k_map_summary<false><<<(uint32_t)((n_reads + 3) / 4 < 16384 ? (n_reads + 3) / 4 : 16384), 256, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

int mgx_launch_map_subk(const void *dev_graph, const char *seqs, const uint64_t *offsets, const uint64_t *node_begin, uint32_t *nodes,
                        uint64_t n_reads, uint32_t map_length, void *stream) {
    static_assert(sizeof(DevGraph) == MGX_DEV_GRAPH_BYTES, "DevGraph differs from what mgx_map.hip passes");
    if (!n_reads) return 0;
    k_map_subk<<<(uint32_t)((n_reads + 3) / 4 < 16384 ? (n_reads + 3) / 4 : 16384), 256, 0, (hipStream_t)stream>>>(
        *static_cast<const DevGraph *>(dev_graph), seqs, offsets, node_begin, nodes, n_reads, (int32_t)map_length);
    return (int)hipGetLastError();
}

uint32_t mgx_map_summary_short_max(void) { return (uint32_t)MS_SHORT_MAX; }

// ------------------------------------------------------------------------------------------------
// host side: presence and text (no GPU)
// ------------------------------------------------------------------------------------------------
int mgx_map_present(const mgx_map_counts *c, uint64_t query_len, uint32_t k, uint32_t map_length, double discovery_fraction) {
    if (!c) return 0;
    const size_t n_kmers = c->n_kmers, n_discovered = c->n_discovered;
    if (map_length == 0 || map_length >= k) {
        // DeBruijnGraph::find (sequence_graph.cpp:65-89)
        if (query_len < k) return 0;
        const size_t max_kmers_missing = (size_t)(n_kmers * (1 - discovery_fraction));
        return n_kmers - n_discovered <= max_kmers_missing ? 1 : 0;
    }
    // cli/align.cpp:139-149
    const size_t min_kmers_discovered = (size_t)(n_kmers - n_kmers * (1 - discovery_fraction));
    return n_discovered >= min_kmers_discovered ? 1 : 0;
}

size_t mgx_format_map(const mgx_map_summary *s, uint64_t qi, const char *header, const char *query, size_t query_len, uint32_t k,
                      uint32_t map_length, int format, double discovery_fraction, char *buf, size_t buf_len) {
    std::string t;
    if (s && qi < s->n_queries && header && query) {
        const mgx_map_counts &c = s->counts[qi];
        const uint32_t len = map_length == 0 || map_length >= k ? k : map_length;
        if (format == MGX_MAP_FMT_QUERY_PRESENCE) {
            t = mgx_map_present(&c, query_len, k, map_length, discovery_fraction) ? "1\n" : "0\n";
        } else if (format == MGX_MAP_FMT_FILTER_PRESENT) {
            if (mgx_map_present(&c, query_len, k, map_length, discovery_fraction)) {
                t = ">";
                t += header;
                t += '\n';
                t.append(query, query_len);
                t += '\n';
            }
        } else if (format == MGX_MAP_FMT_COUNT_KMERS) {
            t = header;
            t += '\t' + std::to_string(c.n_discovered) + '/' + std::to_string(c.n_kmers) + '/' + std::to_string(c.n_unique) + '\n';
        } else if (format == MGX_MAP_FMT_NODES && s->node_begin && s->nodes) {
            for (uint64_t i = s->node_begin[qi]; i < s->node_begin[qi + 1]; ++i) {
                const uint64_t w = i - s->node_begin[qi];
                if (w + len > query_len) break;
                t.append(query + w, len);
                t += ": " + std::to_string(s->nodes[i]) + '\n';
            }
        }
    }
    if (buf && buf_len) {
        const size_t n = t.size() < buf_len - 1 ? t.size() : buf_len - 1;
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return t.size();
}

}  // extern "C"
