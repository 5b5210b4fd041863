// mgx_jsonfmt.hip — the text of `align --json` for a range of an alignment batch on the device (json_format.hpp; host side:
// mgx_format_json_batch in mgx_text.hip).
//
// Shapes.  k_jsonfmt_size and k_jsonfmt_write: one wavefront per query, four per 256-thread workgroup, grid-strided — both are
// the one walk jf_line, which counts or stores (a line is ~60 bytes per path node, so a 150-bp read is a few thousand lane-sized
// objects' worth of work per wavefront).  No LDS, no atomics but the counter of the capacity list.
#include <hip/hip_runtime.h>

#define mgx mgx_jsonfmt_ns
#include "wave.hpp"
#include "json_format.hpp"
#include "kernel_units.hpp"

using namespace mgx;

static_assert(sizeof(JfBatch) == MGX_JSONFMT_ARGS_BYTES, "JfBatch differs from what mgx_text.hip passes");

__global__ void __launch_bounds__(256) k_jsonfmt_size(JfBatch b) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < b.n_queries; i += n_waves) {
        const uint64_t len = jf_line<false>(b, uni(i));
        if ((threadIdx.x & 63) == 0) gst(b.line_len + i, len);
    }
}

__global__ void __launch_bounds__(256) k_jsonfmt_write(JfBatch b) {
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < b.n_queries; i += n_waves) jf_line<true>(b, uni(i));
}

static uint32_t jsonfmt_blocks(uint64_t n_queries) {
    const uint64_t blocks = (n_queries + 3) / 4;
    return (uint32_t)(blocks < 32768 ? blocks : 32768);
}

extern "C" {

int mgx_launch_jsonfmt_size(const void *args, void *stream) {
    const JfBatch &b = *static_cast<const JfBatch *>(args);
    if (!b.n_queries) return 0;
    k_jsonfmt_size<<<jsonfmt_blocks(b.n_queries), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

int mgx_launch_jsonfmt_write(const void *args, void *stream) {
    const JfBatch &b = *static_cast<const JfBatch *>(args);
    if (!b.n_queries) return 0;
    k_jsonfmt_write<<<jsonfmt_blocks(b.n_queries), 256, 0, (hipStream_t)stream>>>(b);
    return (int)hipGetLastError();
}

}  // extern "C"
