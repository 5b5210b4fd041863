// mgx_parse.hip — FASTA / FASTQ text to read batches on the device (reads_parse.hpp): the kernels, their launchers
// and the host side of mgx_parse_reads.
//
// Shapes.  Every kernel is a lane per item, 256-thread workgroups, no LDS: k_parse_count / k_parse_table a 64-byte span of the
// text per lane, k_parse_classify / k_parse_records a line per lane, k_parse_copy 16 destination bytes per lane (its search of the line table: once per wavefront, then within that bracket).  The text is
// read by k_parse_count and k_parse_copy (plus the first and last bytes of every line by k_parse_classify); the sequences are
// written once.  Scans: hipcub on the handle's stream.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/mgx.h"
#define mgx mgx_parse_ns
#include "wave.hpp"
#include "reads_parse.hpp"
#include "kernel_units.hpp"

using namespace mgx;

static_assert(sizeof(RpChunk) == MGX_PARSE_ARGS_BYTES && sizeof(RpSum) == 16 && sizeof(RpCounters) == 48, "the parser's blocks changed size");
static_assert(RP_FASTA == MGX_READS_FASTA && RP_FASTQ == MGX_READS_FASTQ, "format constants");

__global__ void __launch_bounds__(256) k_parse_count(RpChunk c) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < c.n_spans) rp_line_count(c, s);
}

__global__ void __launch_bounds__(256) k_parse_table(RpChunk c) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < c.n_spans) rp_line_table(c, s);
}

__global__ void __launch_bounds__(256) k_parse_classify(RpChunk c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nonempty = i <= c.n_lines ? rp_classify(c, i) : 0u;
    // the last line with a payload: one atomic per wavefront
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)nonempty, d); nonempty = o > nonempty ? o : nonempty; }
    if ((threadIdx.x & 63) == 0 && nonempty) atomicMax(&c.ctr->last_nonempty, nonempty);
}

__global__ void __launch_bounds__(256) k_parse_records(RpChunk c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= c.n_lines) rp_records(c, i);
}

template <int FIELD>
__global__ void __launch_bounds__(256) k_parse_copy(RpChunk c) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, limit = FIELD ? c.name_bytes : c.seq_bytes;
    const uint32_t lane = threadIdx.x & 63u;
    if (16 * (t - lane) >= limit) return;                                   // (the whole wavefront)
    // lanes 0 and 63 search the whole table (the same loop, side by side); the others only between the two lines they found
    uint32_t line = 0;
    if (lane == 0 || lane == 63) line = rp_wave_line<FIELD>(c, t - lane, lane != 0);
    const uint32_t lo = (uint32_t)__shfl((int)line, 0), hi = (uint32_t)__shfl((int)line, 63) + 1u;
    if (16 * t < limit) rp_copy16<FIELD>(c, t, lo, hi);
}

__global__ void __launch_bounds__(256) k_parse_rebase(const uint64_t *offsets, uint64_t first, uint64_t n, uint64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) rp_rebase(offsets, first, out, i);
}

struct RpAdd {
    __host__ __device__ __forceinline__ RpSum operator()(const RpSum &a, const RpSum &b) const {
        RpSum r;
        r.seq = a.seq + b.seq; r.name = a.name + b.name; r.rec = a.rec + b.rec;
        return r;
    }
};

static uint32_t blocks_for(uint64_t lanes) { return (uint32_t)((lanes + 255) / 256); }

extern "C" {

int mgx_launch_parse_count(const void *args, void *stream) {
    const RpChunk &c = *static_cast<const RpChunk *>(args);
    if (!c.n_spans) return 0;
    k_parse_count<<<blocks_for(c.n_spans), 256, 0, (hipStream_t)stream>>>(c);
    return (int)hipGetLastError();
}
int mgx_launch_parse_table(const void *args, void *stream) {
    const RpChunk &c = *static_cast<const RpChunk *>(args);
    if (!c.n_spans) return 0;
    k_parse_table<<<blocks_for(c.n_spans), 256, 0, (hipStream_t)stream>>>(c);
    return (int)hipGetLastError();
}
int mgx_launch_parse_classify(const void *args, void *stream) {
    const RpChunk &c = *static_cast<const RpChunk *>(args);
    k_parse_classify<<<blocks_for((uint64_t)c.n_lines + 1), 256, 0, (hipStream_t)stream>>>(c);
    return (int)hipGetLastError();
}
int mgx_launch_parse_records(const void *args, void *stream) {
    const RpChunk &c = *static_cast<const RpChunk *>(args);
    k_parse_records<<<blocks_for((uint64_t)c.n_lines + 1), 256, 0, (hipStream_t)stream>>>(c);
    return (int)hipGetLastError();
}
int mgx_launch_parse_copy(const void *args, int names, void *stream) {
    const RpChunk &c = *static_cast<const RpChunk *>(args);
    const uint64_t bytes = names ? c.name_bytes : c.seq_bytes;
    if (!bytes) return 0;
    if (names) k_parse_copy<1><<<blocks_for((bytes + 15) / 16), 256, 0, (hipStream_t)stream>>>(c);
    else k_parse_copy<0><<<blocks_for((bytes + 15) / 16), 256, 0, (hipStream_t)stream>>>(c);
    return (int)hipGetLastError();
}

}  // extern "C"

// =================================================================================================
// host side
// =================================================================================================
namespace {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    mgx_set_last_error(buf);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? MGX_ERR_OOM : MGX_ERR_NO_DEVICE, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

// a device (or pinned host) block that only grows; its contents are undefined after ensure()
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pinned_host = false;
    ~Buf() { release(); }
    void release() {
        if (p) { if (pinned_host) (void)hipHostFree(p); else (void)hipFree(p); }
        p = nullptr; bytes = 0;
    }
    int ensure(size_t n) {
        if (n <= bytes) return MGX_OK;
        release();
        const size_t want = n + n / 8 + 256;
        const hipError_t e = pinned_host ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(MGX_ERR_OOM, "mgx_parse_reads: allocating %zu bytes failed: %s", want, hipGetErrorString(e)); }
        bytes = want;
        return MGX_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

enum { RP_CNT_LINE = 0, RP_CNT_COPY, RP_CNT_H2D_BYTES, RP_CNT_D2H_BYTES };
std::atomic<uint64_t> g_parse_counts[4];        // mgx_parse_kernel_launch_counts

}  // namespace

struct mgx_read_parser {
    int device = 0;
    hipStream_t stream = nullptr;
    Buf text, mask, span_count, span_first, line_begin, items, sums, ctr, scan_tmp, offsets, name_offsets, seqs, names, slice;
    Buf h_offsets, h_name_offsets, h_names;
    uint64_t n_records = 0, seq_bytes = 0;
    mgx_read_parser() { h_offsets.pinned_host = h_name_offsets.pinned_host = h_names.pinned_host = true; }
};

extern "C" {

int mgx_read_parser_create(int device, mgx_read_parser **out) {
    if (!out) return fail(MGX_ERR_INVALID, "null argument");
    *out = nullptr;
    if (mgx_device_count() <= device || device < 0) return fail(MGX_ERR_NO_DEVICE, "no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    mgx_read_parser *p = new mgx_read_parser;
    p->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete p; return fail(MGX_ERR_NO_DEVICE, "hipStreamCreateWithFlags: %s", hipGetErrorString(e)); }
    *out = p;
    return MGX_OK;
}

void mgx_read_parser_destroy(mgx_read_parser *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) { (void)hipStreamSynchronize(p->stream); (void)hipStreamDestroy(p->stream); }
    delete p;
}

void *mgx_pinned_alloc(size_t bytes) {
    void *q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); fail(MGX_ERR_OOM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return nullptr; }
    return q;
}
void mgx_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

void mgx_parse_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_parse_counts[x].load(); }

int mgx_parse_reads(mgx_read_parser *p, const char *text, uint64_t n_bytes, int text_on_device, int final_chunk, uint32_t flags, mgx_reads *out) {
    static_assert(sizeof(RpChunk) == MGX_PARSE_ARGS_BYTES, "RpChunk differs from what the launchers take");
    if (!p || !out || (n_bytes && !text)) return fail(MGX_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)(MGX_READS_FASTA | MGX_READS_FASTQ) || flags == (MGX_READS_FASTA | MGX_READS_FASTQ))
        return fail(MGX_ERR_INVALID, "mgx_parse_reads: flags may force one format (MGX_READS_FASTA or MGX_READS_FASTQ)");
    if (n_bytes >= 0xFFFFFFFFull) return fail(MGX_ERR_INVALID, "mgx_parse_reads: a chunk of %llu bytes (chunks stay below 2^32 - 1 bytes)", (unsigned long long)n_bytes);
    HIP_TRY(hipSetDevice(p->device));
    // the views of the previous parse end here, whatever becomes of this one: after a refusal the handle holds no records
    p->n_records = 0; p->seq_bytes = 0;
    hipStream_t st = p->stream;
    auto d2h = [&](void *dst, const void *src, size_t bytes) {
        g_parse_counts[RP_CNT_D2H_BYTES] += bytes;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    };
    // the text on the device (it crosses the bus once)
    const char *d_text = text;
    if (!text_on_device && n_bytes) {
        if (int rc = p->text.ensure(n_bytes + 16)) return rc;
        HIP_TRY(hipMemcpyAsync(p->text.p, text, n_bytes, hipMemcpyHostToDevice, st));
        g_parse_counts[RP_CNT_H2D_BYTES] += n_bytes;
        d_text = p->text.as<char>();
    }
    // the format: the first byte of the first non-empty line (a device text is looked at through windows of 4 KB)
    char window[4096];
    uint64_t window_at = ~0ull;
    hipError_t window_err = hipSuccess;
    auto at = [&](uint64_t q) -> char {
        if (!text_on_device) return text[q];
        if (q / sizeof(window) != window_at) {
            window_at = q / sizeof(window);
            const uint64_t b = window_at * sizeof(window), len = std::min<uint64_t>(sizeof(window), n_bytes - b);
            hipError_t e = d2h(window, d_text + b, len);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { window_err = e; memset(window, '\n', sizeof(window)); }
        }
        return window[q % sizeof(window)];
    };
    uint64_t pos = 0;
    int fmt = rp_detect_format(at, n_bytes, final_chunk != 0, &pos);
    HIP_TRY(window_err);
    if (fmt < 0)
        return fail(MGX_ERR_INVALID, "mgx_parse_reads: the line at byte %llu begins with neither '>' (FASTA) nor '@' (FASTQ)", (unsigned long long)pos);
    if (flags) fmt = (int)flags;
    if (int rc = p->h_offsets.ensure(8)) return rc;
    if (int rc = p->h_name_offsets.ensure(8)) return rc;
    if (int rc = p->h_names.ensure(1)) return rc;
    if (int rc = p->offsets.ensure(8)) return rc;
    if (int rc = p->seqs.ensure(16)) return rc;
    auto finish = [&](uint64_t n_records, uint64_t consumed) {
        p->n_records = n_records; p->seq_bytes = n_records ? p->h_offsets.as<uint64_t>()[n_records] : 0;
        out->n_records = n_records; out->consumed = consumed; out->format = (uint32_t)fmt;
        out->seqs = p->seqs.as<char>(); out->offsets = p->offsets.as<uint64_t>();
        out->host_offsets = p->h_offsets.as<uint64_t>();
        out->names = p->h_names.as<char>(); out->name_offsets = p->h_name_offsets.as<uint64_t>();
        return MGX_OK;
    };
    if (fmt == 0 || n_bytes == 0) {
        p->h_offsets.as<uint64_t>()[0] = 0; p->h_name_offsets.as<uint64_t>()[0] = 0;
        HIP_TRY(hipMemsetAsync(p->offsets.p, 0, 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        return finish(0, final_chunk ? n_bytes : 0);
    }

    RpChunk c;
    memset(&c, 0, sizeof(c));
    c.text = d_text; c.n = n_bytes; c.mis = (uint32_t)((uintptr_t)d_text & 15u);
    c.n_spans = (uint32_t)((n_bytes + c.mis + RP_SPAN - 1) / RP_SPAN);
    c.format = (uint32_t)fmt; c.final_chunk = final_chunk ? 1u : 0u;
    // ---- line pass ----
    if (int rc = p->mask.ensure((size_t)c.n_spans * 8)) return rc;
    if (int rc = p->span_count.ensure(((size_t)c.n_spans + 1) * 4)) return rc;
    if (int rc = p->span_first.ensure(((size_t)c.n_spans + 1) * 4)) return rc;
    c.mask = p->mask.as<uint64_t>(); c.span_count = p->span_count.as<uint32_t>(); c.span_first = p->span_first.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(c.span_count + c.n_spans, 0, 4, st));
    HIP_TRY((hipError_t)mgx_launch_parse_count(&c, st));
    ++g_parse_counts[RP_CNT_LINE];
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, c.span_count, p->span_first.as<uint32_t>(), (int)(c.n_spans + 1), st));
    if (int rc = p->scan_tmp.ensure(tmp_bytes + 16)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(p->scan_tmp.p, tmp_bytes, c.span_count, p->span_first.as<uint32_t>(), (int)(c.n_spans + 1), st));
    uint32_t n_newlines = 0;
    char last_byte = '\n';
    HIP_TRY(d2h(&n_newlines, c.span_first + c.n_spans, 4));
    if (text_on_device) HIP_TRY(d2h(&last_byte, d_text + n_bytes - 1, 1)); else last_byte = text[n_bytes - 1];
    HIP_TRY(hipStreamSynchronize(st));
    c.n_lines = n_newlines + (final_chunk && last_byte != '\n' ? 1u : 0u);
    if (c.n_lines >= 0x7FFFFFF0u) return fail(MGX_ERR_INVALID, "mgx_parse_reads: %u lines in one chunk", c.n_lines);
    const size_t nl = c.n_lines;
    if (int rc = p->line_begin.ensure(((size_t)n_newlines + 2) * 4)) return rc;
    if (int rc = p->items.ensure((nl + 1) * sizeof(RpSum))) return rc;
    if (int rc = p->sums.ensure((nl + 1) * sizeof(RpSum))) return rc;
    if (int rc = p->ctr.ensure(sizeof(RpCounters))) return rc;
    // (records: one per header line at most — every fourth line of a FASTQ chunk)
    const size_t max_records = fmt == (int)RP_FASTQ ? nl / 4 + 1 : nl;
    if (int rc = p->offsets.ensure((max_records + 2) * 8)) return rc;
    if (int rc = p->name_offsets.ensure((max_records + 2) * 8)) return rc;
    c.line_begin = p->line_begin.as<uint32_t>(); c.items = p->items.as<RpSum>(); c.sums = p->sums.as<RpSum>(); c.ctr = p->ctr.as<RpCounters>();
    c.offsets = p->offsets.as<uint64_t>(); c.name_offsets = p->name_offsets.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(c.ctr, 0, sizeof(RpCounters), st));
    HIP_TRY(hipMemsetAsync(&c.ctr->err_pos, 0xFF, 4, st));
    HIP_TRY((hipError_t)mgx_launch_parse_table(&c, st));
    ++g_parse_counts[RP_CNT_LINE];
    // ---- classify, scan, records ----
    HIP_TRY((hipError_t)mgx_launch_parse_classify(&c, st));
    const RpSum zero = { 0, 0, 0 };
    HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, tmp_bytes, c.items, p->sums.as<RpSum>(), RpAdd(), zero, (int)(nl + 1), st));
    if (int rc = p->scan_tmp.ensure(tmp_bytes + 16)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveScan(p->scan_tmp.p, tmp_bytes, c.items, p->sums.as<RpSum>(), RpAdd(), zero, (int)(nl + 1), st));
    HIP_TRY((hipError_t)mgx_launch_parse_records(&c, st));
    RpCounters k;
    HIP_TRY(d2h(&k, c.ctr, sizeof(k)));
    HIP_TRY(hipStreamSynchronize(st));
    if (const char *what = rp_verdict(c.format, c.n_lines, final_chunk != 0, k, &pos))
        return fail(MGX_ERR_INVALID, "mgx_parse_reads: outside the grammar at the line that begins at byte %llu: %s", (unsigned long long)pos, what);
    // ---- copy ----
    c.seq_bytes = k.seq_bytes; c.name_bytes = k.name_bytes;
    if (int rc = p->seqs.ensure(k.seq_bytes + 16)) return rc;
    if (int rc = p->names.ensure(k.name_bytes + 16)) return rc;
    if (int rc = p->h_names.ensure(k.name_bytes + 1)) return rc;
    if (int rc = p->h_offsets.ensure((k.n_records + 1) * 8)) return rc;
    if (int rc = p->h_name_offsets.ensure((k.n_records + 1) * 8)) return rc;
    c.seqs = p->seqs.as<char>(); c.names = p->names.as<char>();
    HIP_TRY((hipError_t)mgx_launch_parse_copy(&c, 0, st));
    HIP_TRY((hipError_t)mgx_launch_parse_copy(&c, 1, st));
    g_parse_counts[RP_CNT_COPY] += (k.seq_bytes ? 1 : 0) + (k.name_bytes ? 1 : 0);
    if (k.name_bytes) HIP_TRY(d2h(p->h_names.p, c.names, k.name_bytes));
    HIP_TRY(d2h(p->h_name_offsets.p, c.name_offsets, (k.n_records + 1) * 8));
    HIP_TRY(d2h(p->h_offsets.p, c.offsets, (k.n_records + 1) * 8));
    HIP_TRY(hipStreamSynchronize(st));
    if (p->h_offsets.as<uint64_t>()[k.n_records] != k.seq_bytes || p->h_name_offsets.as<uint64_t>()[k.n_records] != k.name_bytes)
        return fail(MGX_ERR_INVALID, "mgx_parse_reads: internal: the offsets do not end at the byte counts");
    const int rc = finish(k.n_records, final_chunk ? n_bytes : k.consumed);
    p->seq_bytes = k.seq_bytes;
    return rc;
}

int mgx_read_parser_slice(mgx_read_parser *p, uint64_t first, uint64_t n, const char **seqs, const uint64_t **offsets) {
    if (!p || !seqs || !offsets) return fail(MGX_ERR_INVALID, "null argument");
    if (first > p->n_records || n > p->n_records - first)
        return fail(MGX_ERR_INVALID, "mgx_read_parser_slice: records %llu .. %llu of %llu", (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)p->n_records);
    *seqs = p->seqs.as<char>() + p->h_offsets.as<uint64_t>()[first];
    *offsets = p->offsets.as<uint64_t>();
    if (first == 0) return MGX_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = p->slice.ensure((n + 1) * 8)) return rc;
    k_parse_rebase<<<blocks_for(n + 1), 256, 0, p->stream>>>(p->offsets.as<uint64_t>(), first, n, p->slice.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    *offsets = p->slice.as<uint64_t>();
    return MGX_OK;
}

int mgx_read_parser_fetch(mgx_read_parser *p, char *seqs_out, uint64_t *offsets_out) {
    if (!p || (!seqs_out && p->seq_bytes) || !offsets_out) return fail(MGX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    memcpy(offsets_out, p->h_offsets.p, (p->n_records + 1) * 8);
    if (p->seq_bytes) {
        HIP_TRY(hipMemcpyAsync(seqs_out, p->seqs.p, p->seq_bytes, hipMemcpyDeviceToHost, p->stream));
        g_parse_counts[RP_CNT_D2H_BYTES] += p->seq_bytes;
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return MGX_OK;
}

}  // extern "C"
