// mgx_format.hip — the TSV text of an alignment batch on the device (tsv_format.hpp; host side: mgx_format_tsv_batch in mgx_text.hip).
//
// Shapes.  k_format_size: one query per lane (a serial walk over the query's few alignments; 4 bytes of arithmetic per CIGAR
// run).  k_format_write: one wavefront per query, four per 256-thread workgroup, grid-strided — the text of a 150-bp read is
// ~350 bytes, i.e. two lane-strided dword stores per bulk copy.  k_format_patch: the lengths of the few lines the host
// formatted (capacity retries) into the size pass's array before the scan is repeated.  No LDS, no atomics but the counter of
// the capacity list.
#include <hip/hip_runtime.h>

#define mgx mgx_format_ns
#include "wave.hpp"
#include "tsv_format.hpp"
#include "kernel_units.hpp"

using namespace mgx;

static_assert(sizeof(TfBatch) == MGX_FORMAT_ARGS_BYTES, "TfBatch differs from what mgx_text.hip passes");

__global__ void __launch_bounds__(256) k_format_size(TfBatch b) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < b.n_queries) gst(b.line_len + q, tf_line_size(b, q));
}

__global__ void __launch_bounds__(256) k_format_write(TfBatch b) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < b.n_queries; q += n_waves) tf_write_line(b, uni(q));
}

__global__ void __launch_bounds__(256) k_format_patch(uint64_t *line_len, const uint32_t *queries, const uint64_t *lens, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) gst(line_len + gld(queries + i), gld(lens + i));
}

extern "C" {

int mgx_launch_format_size(const void *args, void *stream) {
    const TfBatch &b = *static_cast<const TfBatch *>(args);
    if (!b.n_queries) return 0;
    k_format_size<<<(uint32_t)((b.n_queries + 255) / 256), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

int mgx_launch_format_write(const void *args, void *stream) {
    const TfBatch &b = *static_cast<const TfBatch *>(args);
    if (!b.n_queries) return 0;
    const uint64_t blocks = (b.n_queries + 3) / 4;
    k_format_write<<<(uint32_t)(blocks < 32768 ? blocks : 32768), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

int mgx_launch_format_patch(uint64_t *line_len, const uint32_t *queries, const uint64_t *lens, uint32_t m, void *stream) {
    if (!m) return 0;
    k_format_patch<<<(m + 255) / 256, 256, 0, (hipStream_t)stream>>>(line_len, queries, lens, m);
    return (int)hipGetLastError();
}

}  // extern "C"
