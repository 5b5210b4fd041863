// mgx_decode.hip — the structured results of an alignment batch (the mgx_results layout) on the device (results_decode.hpp; host
// side: decode_on_device in mgx_results.hip, behind mgx_decode_results_device and the pipeline option decode_on_device).
//
// Shapes.  k_decode_size: one query per lane (a serial walk over the headers of the query's few alignments: five sums), plus one
// lane for the zeros that close the scans.  k_decode_write: one wavefront per query, four per 256-thread workgroup, grid-strided
// — a 150-bp read has ~120 nodes (two lane-strided 8-byte stores), a handful of runs and ~150 path characters.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#define mgx mgx_decode_ns
#include "wave.hpp"
#include "results_decode.hpp"
#include "kernel_units.hpp"

using namespace mgx;

static_assert(sizeof(RdBatch) == MGX_DECODE_ARGS_BYTES, "RdBatch differs from what mgx_results.hip passes");

__global__ void __launch_bounds__(256) k_decode_size(RdBatch b) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= b.n_queries) rd_query_counts(b, q);
}

__global__ void __launch_bounds__(256) k_decode_write(RdBatch b) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < b.n_queries; q += n_waves) rd_write_query(b, uni(q));
}

extern "C" {

int mgx_launch_decode_size(const void *args, void *stream) {
    const RdBatch &b = *static_cast<const RdBatch *>(args);
    if (!b.n_queries) return 0;
    k_decode_size<<<(uint32_t)((b.n_queries + 1 + 255) / 256), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

int mgx_launch_decode_write(const void *args, void *stream) {
    const RdBatch &b = *static_cast<const RdBatch *>(args);
    if (!b.n_queries) return 0;
    const uint64_t blocks = (b.n_queries + 3) / 4;
    k_decode_write<<<(uint32_t)(blocks < 32768 ? blocks : 32768), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

}  // extern "C"
