// format_bench_host.cpp — the baseline leg of tools/format_bench.py: what a caller of the C-ABI did for the TSV text of a batch
// before mgx_format_tsv_batch existed — mgx_fetch_results, then mgx_format_tsv query by query into one preallocated buffer.
// Built by format_bench.py (g++, host code; links libmgx.so).
#include <cstdint>
#include <cstring>

#include "../include/mgx.h"

extern "C" int64_t format_bench_fetch_and_format(mgx_aligner *a, const char *headers, const uint64_t *header_offsets, const char *seqs,
                                                 const uint64_t *offsets, uint64_t n, int32_t min_path_score, char *buf, uint64_t cap,
                                                 uint64_t *line_begin) {
    mgx_results res;
    if (int rc = mgx_fetch_results(a, &res)) return rc;
    uint64_t at = 0;
    char header[4096];
    for (uint64_t q = 0; q < n; ++q) {
        const uint64_t hl = header_offsets[q + 1] - header_offsets[q];
        if (hl >= sizeof(header)) return -1;
        memcpy(header, headers + header_offsets[q], hl);            // (mgx_format_tsv takes the header as a C string)
        header[hl] = 0;
        line_begin[q] = at;
        const size_t need = mgx_format_tsv(&res, q, header, seqs + offsets[q], offsets[q + 1] - offsets[q], min_path_score, buf + at, cap - at);
        if (need + 1 > cap - at) return -1;
        at += need;
    }
    line_begin[n] = at;
    return (int64_t)at;
}
