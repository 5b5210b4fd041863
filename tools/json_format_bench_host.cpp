// json_format_bench_host.cpp — the baseline leg of tools/json_format_bench.py: what a caller of the C-ABI did for the `align --json`
// text of a batch before mgx_format_json_batch existed — mgx_fetch_results, then mgx_format_json query by query into one
// preallocated buffer.  Built by json_format_bench.py (g++, host code; links libmgx.so).
#include <cstdint>
#include <cstring>

#include "../include/mgx.h"

extern "C" int64_t json_format_bench_fetch_and_format(mgx_aligner *a, const char *headers, const uint64_t *header_offsets, const char *seqs,
                                                      const uint64_t *offsets, uint64_t n, uint32_t k, char *buf, uint64_t cap,
                                                      uint64_t *line_begin) {
    mgx_results res;
    if (int rc = mgx_fetch_results(a, &res)) return rc;
    uint64_t at = 0;
    char header[4096];
    for (uint64_t q = 0; q < n; ++q) {
        const uint64_t hl = header_offsets[q + 1] - header_offsets[q];
        if (hl >= sizeof(header)) return -1;
        memcpy(header, headers + header_offsets[q], hl);            // (mgx_format_json takes the header as a C string)
        header[hl] = 0;
        line_begin[q] = at;
        const size_t need = mgx_format_json(&res, q, header, seqs + offsets[q], offsets[q + 1] - offsets[q], k, buf + at, cap - at);
        if (need + 1 > cap - at) return -1;
        at += need;
    }
    line_begin[n] = at;
    return (int64_t)at;
}
