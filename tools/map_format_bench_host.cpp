// map_format_bench_host.cpp — the baseline leg of tools/map_format_bench.py: what a caller of the C-ABI did for the text of
// `align --map` before mgx_format_map_batch existed — mgx_map_summary_batch (with MGX_MAP_WANT_NODES for the k-mer: node form),
// then mgx_format_map query by query into one preallocated buffer.  Built by map_format_bench.py (g++, host code; links libmgx.so).
#include <cstdint>
#include <cstring>

#include "../include/mgx.h"

extern "C" int64_t map_format_bench_summary_and_format(mgx_aligner *a, const char *headers, const uint64_t *header_offsets, const char *seqs,
                                                       const uint64_t *offsets, uint64_t n, uint32_t k, int format, double discovery_fraction,
                                                       char *buf, uint64_t cap, uint64_t *line_begin) {
    mgx_map_summary s;
    if (int rc = mgx_map_summary_batch(a, seqs, offsets, n, 0, 0, format == MGX_MAP_FMT_NODES ? MGX_MAP_WANT_NODES : 0, &s)) return -(int64_t)rc;
    uint64_t at = 0;
    char header[4096];
    for (uint64_t q = 0; q < n; ++q) {
        const uint64_t hl = header_offsets[q + 1] - header_offsets[q];
        if (hl >= sizeof(header)) return -100;
        memcpy(header, headers + header_offsets[q], hl);            // (mgx_format_map takes the header as a C string)
        header[hl] = 0;
        line_begin[q] = at;
        const size_t need = mgx_format_map(&s, q, header, seqs + offsets[q], offsets[q + 1] - offsets[q], k, 0, format, discovery_fraction,
                                           buf + at, cap - at);
        if (need + 1 > cap - at) return -101;
        at += need;
    }
    line_begin[n] = at;
    return (int64_t)at;
}
