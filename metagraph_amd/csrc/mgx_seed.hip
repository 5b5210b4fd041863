// mgx_seed.hip — the wave-per-read seeding kernel (seed_kernel.hpp: one 64-lane wavefront per read), its two instantiations
// (MGX_SEED_WPS wavefronts per SIMD for short reads on a full machine, else MGX_ALIGN_WAVES_PER_SIMD) behind one launcher.
// Two builds of this file go into libmgx.so, each in a namespace of its own: the plain one, and -DMGX_WITH_PRIMARY=1 with the
// CanonicalDBG (PRIMARY graph) branches of align_core.hpp compiled in (reverse-complement sub-k seeds, wrapper terminus bits;
// canon_graph.hpp), so that the seeding kernel of every other graph stays the code it was.  The extension half for PRIMARY
// graphs is the MGX_WITH_PRIMARY build of mgx_grp.hip.
#include <hip/hip_runtime.h>

#if MGX_WITH_PRIMARY
#define mgx mgx_primary
#define MGX_SUFFIX(x) x##_primary
#else
#define MGX_SUFFIX(x) x
#endif
#define MGX_NO_EXTEND 1      // this unit only seeds; the extension lives in mgx_grp.hip, mgx_ext64.hip, mgx_lab64.hip
#include "wave.hpp"
#include "seed_kernel.hpp"
#include "kernel_units.hpp"

using namespace mgx;

extern "C" int MGX_SUFFIX(mgx_launch_seed)(const void *params, uint32_t blocks, uint32_t lds_bytes, int wps8, void *stream) {
    static_assert(sizeof(AlignParams) == MGX_ALIGN_PARAMS_BYTES, "AlignParams differs from what mgx.hip passes");
    const AlignParams &P = *static_cast<const AlignParams *>(params);
    if (wps8) k_align<PH_SEED, MGX_SEED_WPS><<<blocks, 64, lds_bytes, (hipStream_t)stream>>>(P, lds_bytes);
    else k_align<PH_SEED><<<blocks, 64, lds_bytes, (hipStream_t)stream>>>(P, lds_bytes);
    return (int)hipGetLastError();
}
// static LDS of the seeding kernels: control block + the interval lists of the sdust scratch; no score rows (seed_kernel.hpp)
static_assert(((sizeof(Wave) + SDUST_LDS_BYTES_REGTAB + 16 + 127) & ~127ull) == MGX_SEED_STATIC_LDS_BYTES, "the seeding kernel's static LDS differs from what mgx.hip sizes its dynamic LDS with");
#if !MGX_WITH_PRIMARY
extern "C" unsigned mgx_seed_static_lds(void) { return MGX_SEED_STATIC_LDS_BYTES; }
extern "C" int mgx_seed_load(void) {
    hipFuncAttributes attr;
    return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_align<PH_SEED>));
}
#endif
