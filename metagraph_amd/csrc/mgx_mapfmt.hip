// mgx_mapfmt.hip — the text of `align --map` for a whole batch on the device (map_format.hpp; host side: mgx_format_map_batch in
// mgx_text.hip).
//
// Shapes.  k_mapfmt_size: NODES — one wavefront per query, four per 256-thread workgroup, grid-strided (the node array is read
// 64 nodes at a time); the other formats — one query per lane.  k_mapfmt_write: one wavefront per query in the same grid
// shape (NODES: a lane per line, 64 lines per round; COUNT_KMERS / FILTER_PRESENT: lane-strided bulk copies); QUERY_PRESENCE —
// one query per lane, its text is two bytes.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#define mgx mgx_mapfmt_ns
#include "wave.hpp"
#include "map_format.hpp"
#include "kernel_units.hpp"

using namespace mgx;

static_assert(sizeof(MfBatch) == MGX_MAPFMT_ARGS_BYTES, "MfBatch differs from what mgx_text.hip passes");

__global__ void __launch_bounds__(256) k_mapfmt_size(MfBatch b) {
    if (b.format == MF_NODES) {
        const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
        for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < b.n_queries; q += n_waves) {
            const uint64_t len = mf_nodes_size(b, uni(q));
            if ((threadIdx.x & 63) == 0) gst(b.line_len + q, len);
        }
    } else {
        const uint64_t n_lanes = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < b.n_queries; q += n_lanes) gst(b.line_len + q, mf_line_size(b, q));
    }
}

__global__ void __launch_bounds__(256) k_mapfmt_write(MfBatch b) {
    if (b.format == MF_QUERY_PRESENCE) {
        const uint64_t n_lanes = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < b.n_queries; q += n_lanes) mf_write_presence(b, q);
    } else {
        const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
        for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < b.n_queries; q += n_waves) mf_write_line(b, uni(q));
    }
}

// blocks of 256 threads for n_queries items of one lane (per_wave == 0) or one wavefront each
static uint32_t mapfmt_blocks(uint64_t n_queries, bool per_wave) {
    const uint64_t blocks = per_wave ? (n_queries + 3) / 4 : (n_queries + 255) / 256;
    return (uint32_t)(blocks < 32768 ? blocks : 32768);
}

extern "C" {

int mgx_launch_mapfmt_size(const void *args, void *stream) {
    const MfBatch &b = *static_cast<const MfBatch *>(args);
    if (!b.n_queries) return 0;
    k_mapfmt_size<<<mapfmt_blocks(b.n_queries, b.format == MF_NODES), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

int mgx_launch_mapfmt_write(const void *args, void *stream) {
    const MfBatch &b = *static_cast<const MfBatch *>(args);
    if (!b.n_queries) return 0;
    k_mapfmt_write<<<mapfmt_blocks(b.n_queries, b.format != MF_QUERY_PRESENCE), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

}  // extern "C"
