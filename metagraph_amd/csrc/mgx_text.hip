// mgx_text.hip — the output text of a batch: the per-query host formatters (mgx_format_tsv[_labeled], mgx_format_json) and the one
// host sequence (FormatJob, format_on_device) behind the three entry points whose text is written by kernels — mgx_format_tsv_batch
// (mgx_format.hip), mgx_format_map_batch (mgx_mapfmt.hip), mgx_format_json_batch (mgx_jsonfmt.hip).  Host code.
#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>

#include "host_state.hpp"
#include "kernel_units.hpp"
#include "tsv_format.hpp"
#include "map_format.hpp"
#include "json_format.hpp"

using namespace mgx;

extern "C" {

size_t mgx_format_tsv(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                      int32_t min_path_score, char *buf, size_t buf_len) {
    return mgx_format_tsv_labeled(res, qi, header, query, query_len, min_path_score, nullptr, 0, buf, buf_len);
}
size_t mgx_format_tsv_labeled(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                              int32_t min_path_score, const char *const *label_names, uint32_t n_label_names,
                              char *buf, size_t buf_len) {
    // cli/align.cpp:262-285 + alignment.hpp:426-433; the query is printed normalised (AlignmentResults ctor)
    std::string s(header);
    s += '\t';
    for (size_t i = 0; i < query_len; ++i) {
        int8_t c = (int8_t)query[i];
        s += c >= 0 ? (char)toupper(c) : (char)127;
    }
    if (res->aln_begin[qi] == res->aln_begin[qi + 1]) {
        s += "\t*\t*\t" + std::to_string(min_path_score) + "\t*\t*\t*\n";
    } else {
        static const char ops[] = "SX=DIG";
        for (uint64_t ai = res->aln_begin[qi]; ai < res->aln_begin[qi + 1]; ++ai) {
            const mgx_alignment &a = res->alignments[ai];
            s += a.orientation ? "\t-\t" : "\t+\t";
            s.append(res->seqs + a.seq_begin, a.seq_len);
            s += '\t' + std::to_string(a.score) + '\t' + std::to_string(a.num_matches) + '\t';
            for (uint32_t x = 0; x < a.n_cigar; ++x) {
                const mgx_cigar_op &op = res->cigar[a.cigar_begin + x];
                s += std::to_string(op.len) + ops[op.op];
            }
            s += '\t' + std::to_string(a.offset);
            if (res->labels && a.n_labels) {
                // cli/align.cpp:274-281: the label names (LabelEncoder::decode), joined by ';'
                s += '\t';
                for (uint32_t x = 0; x < a.n_labels; ++x) {
                    const uint32_t lbl = res->labels[a.labels_begin + x];
                    if (x) s += ';';
                    if (label_names && lbl < n_label_names) s += label_names[lbl];
                    else s += std::to_string(lbl);
                }
            }
        }
        s += '\n';
    }
    if (buf && buf_len) {
        size_t nc = std::min(buf_len - 1, s.size());
        memcpy(buf, s.data(), nc);
        buf[nc] = 0;
    }
    return s.size();
}

// ---- the text of a batch, written by kernels: the one host sequence behind mgx_format_tsv_batch, mgx_format_map_batch and
// mgx_format_json_batch.  An entry point checks its arguments and describes its job; format_on_device runs it.
struct FormatJob {
    const char *fn;                                  // the entry point's name, for messages
    const char *oom_advice;                          // the end of the two out-of-memory messages ("" or what the caller can do)
    std::atomic<uint64_t> *size_launches, *write_launches, *d2h_bytes, *h2d_bytes, *host_lines;    // its counters; null: it has none
    int (*launch_size)(const void *, void *);        // the two kernels' launchers ...
    int (*launch_write)(const void *, void *);
    const void *params;                              // ... their TfBatch / MfBatch / JfBatch ...
    char **text;                                     // ... and its `text` field (set here, once the size of the text is known)
    const char *headers;                             // header i of the range: headers[header_offsets[i] .. header_offsets[i + 1])
    const uint64_t *header_offsets;
    uint64_t header_from;                            // header_offsets[0] as the kernels see it: the uploaded bytes start there
    uint64_t first, n, n_batch;                      // queries first .. first + n of the staged batch of n_batch
    // Called once tf_headers, tf_header_offsets, tf_len, tf_begin (and tf_cap, with host_line) are large enough and the headers are
    // on the stream: fills *params but for `text`, uploads the entry point's own tables.
    std::function<int()> bind;
    // The text of a query that the host aligned again: (view of that query's results alone, header, query bytes, their count).
    // None: the formatter leaves no query to the host; no tf_cap, no retry.
    std::function<std::string(const mgx_results &, const char *, const char *, size_t)> host_line;
};

// what a per-query host formatter writes, as a string: size the line, fill it, drop the formatter's NUL
static std::string host_formatted(const std::function<size_t(char *, size_t)> &format) {
    std::string line(format(nullptr, 0) + 1, '\0');
    format(&line[0], line.size());
    line.pop_back();
    return line;
}

static int format_on_device(mgx_aligner *A, const FormatJob &job, mgx_text *out) {
    const uint64_t first = job.first, n = job.n;
    auto count = [](std::atomic<uint64_t> *c, uint64_t by) { if (c) *c += by; };
    auto d2h = [&](void *dst, const void *src, size_t bytes) {
        count(job.d2h_bytes, bytes);
        return copy_sync(A, dst, src, bytes, hipMemcpyDeviceToHost);
    };
    auto h2d = [&](void *dst, const void *src, size_t bytes) {
        count(job.h2d_bytes, bytes);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, A->hstream);
    };
    // the range's headers and their offsets (as the caller counts them: uploaded with every call)
    const uint64_t header_bytes = job.header_offsets[n] - job.header_from;
    if (int rc = A->tf_headers.ensure(header_bytes + 16)) return rc;
    if (int rc = A->tf_header_offsets.ensure((n + 1) * 8)) return rc;
    if (int rc = A->tf_len.ensure((n + 1) * 8)) return rc;
    if (int rc = A->tf_begin.ensure((n + 2) * 8)) return rc;
    if (job.host_line) if (int rc = A->tf_cap.ensure((n + 1) * 4)) return rc;
    if (header_bytes) HIP_TRY(h2d(A->tf_headers.p, job.headers + job.header_from, header_bytes));
    HIP_TRY(h2d(A->tf_header_offsets.p, job.header_offsets, (n + 1) * 8));
    if (int rc = job.bind()) return rc;
    uint64_t *d_len = A->tf_len.as<uint64_t>(), *d_begin = A->tf_begin.as<uint64_t>();
    // pass 1: the line lengths (d_len[n] = 0 closes the scan), the capacity-status queries; the scan gives line_begin
    HIP_TRY(hipMemsetAsync(d_len + n, 0, 8, A->hstream));
    HIP_TRY(hipMemsetAsync(d_begin + n + 1, 0, 8, A->hstream));
    HIP_TRY((hipError_t)job.launch_size(job.params, A->hstream));
    count(job.size_launches, 1);
    if (int rc = exclusive_sum(A, d_len, d_begin, n + 1)) return rc;
    uint64_t counters[2] = { 0, 0 };                  // the text's bytes, the capacity-status queries (0 without host_line)
    HIP_TRY(d2h(counters, d_begin + n, 16));
    // the capacity-status queries of the range: aligned again with larger limits, formatted by host_line, their lengths patched in
    std::vector<uint64_t> todo;
    std::vector<std::string> host_lines;
    if (job.host_line && counters[1]) {
        std::vector<uint32_t> cap(counters[1]);
        HIP_TRY(d2h(cap.data(), A->tf_cap.p, cap.size() * 4));
        std::sort(cap.begin(), cap.end());
        for (uint32_t i : cap) todo.push_back(first + i);
        if (!A->retry_capacity)
            return fail(MGX_ERR_CAPACITY, "%s: query %llu (and %llu more) has a capacity status and retry_capacity is off", job.fn,
                        (unsigned long long)todo.front(), (unsigned long long)todo.size() - 1);
        std::vector<HostResults> fixed;
        std::vector<uint8_t> have;
        std::vector<uint64_t> h_off;
        std::vector<char> h_seq;
        if (int rc = realign_capacity_queries(A, A->last_d_seqs, A->last_d_offsets, job.n_batch, todo, fixed, have, h_off, h_seq)) return rc;
        count(job.d2h_bytes, (job.n_batch + 1) * 8 + (h_seq.size() - 1));
        std::vector<uint64_t> patch_len(todo.size());
        host_lines.resize(todo.size());
        for (size_t t = 0; t < todo.size(); ++t) {
            const uint64_t q = todo[t];
            if (!have[t]) return fail(MGX_ERR_CAPACITY, "%s: query %llu keeps its capacity status after the retry", job.fn, (unsigned long long)q);
            mgx_results v;
            fixed[t].view(&v);
            const std::string header(job.headers + job.header_offsets[q - first], job.headers + job.header_offsets[q - first + 1]);
            host_lines[t] = job.host_line(v, header.c_str(), h_seq.data() + (h_off[q] - h_off[todo.front()]), h_off[q + 1] - h_off[q]);
            patch_len[t] = host_lines[t].size();
        }
        A->hstats.n_capacity_retried = todo.size();
        count(job.host_lines, todo.size());
        // (i, length) pairs: the i as 4-byte words behind the 8-byte lengths
        if (int rc = A->tf_patch.ensure(todo.size() * 12 + 16)) return rc;
        uint32_t *d_pq = reinterpret_cast<uint32_t *>(A->tf_patch.as<uint64_t>() + todo.size());
        HIP_TRY(h2d(A->tf_patch.p, patch_len.data(), todo.size() * 8));
        HIP_TRY(h2d(d_pq, cap.data(), todo.size() * 4));
        HIP_TRY((hipError_t)mgx_launch_format_patch(d_len, d_pq, A->tf_patch.as<uint64_t>(), (uint32_t)todo.size(), A->hstream));
        if (int rc = exclusive_sum(A, d_len, d_begin, n + 1)) return rc;
        HIP_TRY(d2h(counters, d_begin + n, 8));
        HIP_TRY(hipStreamSynchronize(A->hstream));   // (patch_len and cap are read by the copies above)
    }
    // pass 2: the text
    const uint64_t text_bytes = counters[0];
    auto no_buffer = [&](const char *which) {
        return fail(MGX_ERR_OOM, "%s: the text of queries %llu .. %llu needs %llu bytes and no %s buffer of that size could be allocated%s", job.fn,
                    (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)text_bytes, which, job.oom_advice);
    };
    if (A->tf_text.ensure(text_bytes + 16) != MGX_OK) return no_buffer("device");
    if (text_bytes + 1 > A->h_text_bytes) {
        if (A->h_text) { (void)hipHostFree(A->h_text); A->h_text = nullptr; A->h_text_bytes = 0; }
        const size_t want = text_bytes + text_bytes / 8 + 4096;
        void *p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            out->text = "";                          // (what it pointed at is freed)
            return no_buffer("pinned host");
        }
        A->h_text = static_cast<char *>(p); A->h_text_bytes = want;
    }
    *job.text = A->tf_text.as<char>();
    HIP_TRY((hipError_t)job.launch_write(job.params, A->hstream));
    count(job.write_launches, 1);
    count(job.d2h_bytes, text_bytes);
    if (text_bytes) HIP_TRY(hipMemcpyAsync(A->h_text, A->tf_text.p, text_bytes, hipMemcpyDeviceToHost, A->hstream));
    HIP_TRY(d2h(A->h_line_begin.data(), d_begin, (n + 1) * 8));
    for (size_t t = 0; t < todo.size(); ++t) memcpy(A->h_text + A->h_line_begin[todo[t] - first], host_lines[t].data(), host_lines[t].size());
    out->text = A->h_text;
    return MGX_OK;
}

// ---- the TSV text of a batch (tsv_format.hpp, mgx_format.hip) ------------------------------------------------------------
enum { TF_CNT_SIZE = 0, TF_CNT_WRITE, TF_CNT_HOST_LINES, TF_CNT_D2H_BYTES };
static std::atomic<uint64_t> g_format_counts[4];        // mgx_format_kernel_launch_counts
void mgx_format_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_format_counts[x].load(); }

int mgx_format_tsv_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, const char *const *label_names,
                         uint32_t n_label_names, mgx_text *out) {
    static_assert(sizeof(TfBatch) == MGX_FORMAT_ARGS_BYTES, "TfBatch differs from what mgx_format.hip takes");
    if (!A || !out || (n_label_names && !label_names)) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = refuse_chainer(A, "mgx_format_tsv_batch")) return rc;
    const uint64_t n = A->n_reads;
    if (n && (!headers || !header_offsets)) return fail(MGX_ERR_INVALID, "null argument");
    if (A->cfg.post_chain_alignments)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_format_tsv_batch: with post_chain_alignments the chained alignments exist on the host only "
                                         "(mgx_fetch_results + mgx_format_tsv print them)");
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    if (!(A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets))
        return fail(MGX_ERR_INVALID, "mgx_format_tsv_batch: no aligned batch on this handle, or another batch was staged after mgx_align_batch_device");
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_tsv_batch: more than 2^31 - 2 queries in a batch");
    HIP_TRY(hipSetDevice(A->graph->device));
    // the label names (uploaded with every call: a few hundred bytes): for the kernels a blob, for the host formatter C strings
    std::string name_blob;
    std::vector<uint32_t> name_begin(1, 0);
    std::vector<const char *> names(n_label_names);
    for (uint32_t j = 0; j < n_label_names; ++j) {
        names[j] = label_names[j] ? label_names[j] : "";
        name_blob += names[j];
        name_begin.push_back((uint32_t)name_blob.size());
    }
    const size_t names_at = (name_blob.size() + 3) & ~(size_t)3;                 // the begins follow the bytes, 4-byte aligned
    TfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_tsv_batch"; job.oom_advice = "";
    job.size_launches = &g_format_counts[TF_CNT_SIZE]; job.write_launches = &g_format_counts[TF_CNT_WRITE];
    job.d2h_bytes = &g_format_counts[TF_CNT_D2H_BYTES]; job.host_lines = &g_format_counts[TF_CNT_HOST_LINES];
    job.launch_size = mgx_launch_format_size; job.launch_write = mgx_launch_format_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets;
    job.n = job.n_batch = n;
    job.bind = [&]() -> int {
        if (int rc = A->tf_names.ensure(names_at + name_begin.size() * 4 + 16)) return rc;
        if (n_label_names) {
            if (!name_blob.empty()) HIP_TRY(hipMemcpyAsync(A->tf_names.p, name_blob.data(), name_blob.size(), hipMemcpyHostToDevice, A->hstream));
            HIP_TRY(hipMemcpyAsync(A->tf_names.as<char>() + names_at, name_begin.data(), name_begin.size() * 4, hipMemcpyHostToDevice, A->hstream));
        }
        memset(&b, 0, sizeof(b));
        b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
        b.seqs = A->last_d_seqs; b.offsets = A->last_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.name_bytes = A->tf_names.as<char>(); b.name_begin = reinterpret_cast<const uint32_t *>(A->tf_names.as<char>() + names_at);
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.cap_list = A->tf_cap.as<uint32_t>(); b.cap_count = reinterpret_cast<unsigned long long *>(A->tf_begin.as<uint64_t>() + n + 1);
        b.n_queries = n; b.n_names = n_label_names; b.min_path_score = A->cfg.min_path_score; b.labeled = A->anno ? 1u : 0u;
        return MGX_OK;
    };
    job.host_line = [&](const mgx_results &v, const char *header, const char *query, size_t qlen) {
        return host_formatted([&](char *buf, size_t buf_len) {
            return mgx_format_tsv_labeled(&v, 0, header, query, qlen, A->cfg.min_path_score, names.data(), n_label_names, buf, buf_len);
        });
    };
    return format_on_device(A, job, out);
}

// ---- the text of `align --map` for a batch (map_format.hpp, mgx_mapfmt.hip) ---------------------------------
enum { MF_CNT_SIZE = 0, MF_CNT_WRITE, MF_CNT_D2H_BYTES, MF_CNT_H2D_BYTES };
static std::atomic<uint64_t> g_mapfmt_counts[4];        // mgx_format_map_kernel_launch_counts
void mgx_format_map_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_mapfmt_counts[x].load(); }

int mgx_format_map_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, int format, double discovery_fraction,
                         mgx_text *out) {
    static_assert(sizeof(MfBatch) == MGX_MAPFMT_ARGS_BYTES, "MfBatch differs from what mgx_mapfmt.hip takes");
    static_assert(MF_NODES == MGX_MAP_FMT_NODES && MF_COUNT_KMERS == MGX_MAP_FMT_COUNT_KMERS && MF_QUERY_PRESENCE == MGX_MAP_FMT_QUERY_PRESENCE
                  && MF_FILTER_PRESENT == MGX_MAP_FMT_FILTER_PRESENT, "map formats");
    if (!A || !out || !headers || !header_offsets) return fail(MGX_ERR_INVALID, "mgx_format_map_batch: null argument");
    if (int rc = refuse_chainer(A, "mgx_format_map_batch")) return rc;
    if (format != MGX_MAP_FMT_NODES && format != MGX_MAP_FMT_COUNT_KMERS && format != MGX_MAP_FMT_QUERY_PRESENCE && format != MGX_MAP_FMT_FILTER_PRESENT)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: unknown format %d", format);
    if (!A->ms_generation)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: no summary batch staged: mgx_map_summary_batch has not run on this handle");
    if (A->ms_generation != A->stage_generation)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: no summary batch staged: mgx_align_batch_device or mgx_map_batch ran on this "
                                     "handle after mgx_map_summary_batch");
    if (format == MGX_MAP_FMT_NODES && !A->ms_have_nodes)
        return fail(MGX_ERR_INVALID, "mgx_format_map_batch: MGX_MAP_FMT_NODES needs the node array: run mgx_map_summary_batch with "
                                     "MGX_MAP_KEEP_NODES (or MGX_MAP_WANT_NODES)");
    const uint64_t n = A->n_reads;
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_map_batch: more than 2^31 - 2 queries in a batch");
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const uint32_t k = A->graph->g.k, map_length = A->ms_map_length;
    const bool sub_k = map_length != 0 && map_length < k;
    const uint32_t window = sub_k ? map_length : k;
    // the presence threshold for every k-mer count a read of this batch can have, by mgx_map_present's own expressions (the same
    // compiler, the same flags, the same doubles): the kernels compare integers
    const uint32_t max_kmers = A->ms_lmax >= window ? A->ms_lmax - window + 1 : 0;
    const bool presence = format == MGX_MAP_FMT_QUERY_PRESENCE || format == MGX_MAP_FMT_FILTER_PRESENT;
    std::vector<uint64_t> &threshold = A->h_mf_threshold;
    HIP_TRY(hipStreamSynchronize(A->hstream));       // (no earlier upload still reads the table)
    threshold.assign(presence ? (size_t)max_kmers + 1 : 1, 0);
    if (presence)
        for (size_t n_kmers = 0; n_kmers <= max_kmers; ++n_kmers)
            threshold[n_kmers] = mf_threshold_host(n_kmers, discovery_fraction, sub_k);
    MfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_map_batch"; job.oom_advice = "";
    job.size_launches = &g_mapfmt_counts[MF_CNT_SIZE]; job.write_launches = &g_mapfmt_counts[MF_CNT_WRITE];
    job.d2h_bytes = &g_mapfmt_counts[MF_CNT_D2H_BYTES]; job.h2d_bytes = &g_mapfmt_counts[MF_CNT_H2D_BYTES];
    job.launch_size = mgx_launch_mapfmt_size; job.launch_write = mgx_launch_mapfmt_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets;
    job.n = job.n_batch = n;
    job.bind = [&]() -> int {
        if (int rc = A->mf_threshold.ensure(threshold.size() * 8)) return rc;
        g_mapfmt_counts[MF_CNT_H2D_BYTES] += threshold.size() * 8;
        HIP_TRY(hipMemcpyAsync(A->mf_threshold.p, threshold.data(), threshold.size() * 8, hipMemcpyHostToDevice, A->hstream));
        memset(&b, 0, sizeof(b));
        b.counts = A->ms_counts.as<uint32_t>(); b.nodes = A->ms_nodes.as<uint64_t>(); b.node_begin = A->node_begin.as<uint64_t>();
        b.seqs = A->ms_d_seqs; b.offsets = A->ms_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.threshold = A->mf_threshold.as<uint64_t>();
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.n_queries = n; b.max_kmers = presence ? max_kmers : 0; b.k = k; b.window = window; b.sub_k = sub_k ? 1u : 0u; b.format = format;
        return MGX_OK;
    };
    return format_on_device(A, job, out);            // (no host_line: this formatter leaves no line to the host)
}

// ---- metagraph align --json (cli/align.cpp:287-305): Alignment::to_json (alignment.cpp:883-963) + path_json (:704-881),
// written the way Json::writeString does with indentation "" (jsoncpp: object keys in lexicographic order, no white
// space, doubles as %.17g with ".0" appended to integral values, strings with the standard escapes).
namespace {
void json_string(std::string &o, const char *p, size_t n) {
    o += '"';
    for (size_t i = 0; i < n; ++i) {
        const unsigned char c = (unsigned char)p[i];
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20 || c >= 0x7F) { char b[8]; snprintf(b, sizeof(b), "\\u%04X", (unsigned)c); o += b; }
                else o += (char)c;
        }
    }
    o += '"';
}
void json_double(std::string &o, double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    o += b;
    if (!strpbrk(b, ".eEn")) o += ".0";
}
// one edit object: keys from_length, sequence, to_length (only those set)
void json_edit(std::string &o, bool &first, long long from_len, const char *seq, size_t seq_len, long long to_len) {
    if (!first) o += ',';
    first = false;
    o += '{';
    bool f2 = true;
    if (from_len >= 0) { o += "\"from_length\":" + std::to_string(from_len); f2 = false; }
    if (seq) { if (!f2) o += ','; o += "\"sequence\":"; json_string(o, seq, seq_len); f2 = false; }
    if (to_len >= 0) { if (!f2) o += ','; o += "\"to_length\":" + std::to_string(to_len); }
    o += '}';
}
}  // namespace

size_t mgx_format_json(const mgx_results *res, uint64_t qi, const char *header, const char *query, size_t query_len,
                       uint32_t k, char *buf, size_t buf_len) {
    // the query as AlignmentResults keeps it (alignment.cpp:1348-1372): upper case, bytes < 0 -> 127; and its reverse
    // complement (COMPL_TAB, reverse_complement.hpp:31-62)
    std::string fwd(query_len, 0), rc(query_len, 0);
    for (size_t i = 0; i < query_len; ++i) {
        const int8_t c = (int8_t)query[i];
        fwd[i] = c >= 0 ? (char)toupper(c) : (char)127;
    }
    for (size_t i = 0; i < query_len; ++i) {
        const unsigned char c = (unsigned char)fwd[query_len - 1 - i];
        static const char up[] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
        rc[i] = (c >= 'A' && c <= 'Z') ? up[c - 'A'] : (c >= 'a' && c <= 'z') ? (char)(up[c - 'a'] + 32) : c == 96 ? (char)64 : (char)c;
    }
    std::string s;
    const size_t hl = strlen(header);
    if (res->aln_begin[qi] == res->aln_begin[qi + 1]) {
        // Alignment().to_json: an empty alignment carries its name and an empty sequence
        s += "{\"name\":"; json_string(s, header, hl); s += ",\"sequence\":\"\"}\n";
    }
    for (uint64_t ai = res->aln_begin[qi]; ai < res->aln_begin[qi + 1]; ++ai) {
        const mgx_alignment &a = res->alignments[ai];
        const bool secondary = ai != res->aln_begin[qi];
        const std::string &full = a.orientation ? rc : fwd;
        const char *qv = full.data() + a.clipping;                     // query_view_
        const size_t qv_len = query_len - a.clipping - a.end_clipping;
        const mgx_cigar_op *cg = res->cigar + a.cigar_begin;
        // mgx_cigar_op.op: 0 clipped, 1 mismatch, 2 match, 3 deletion, 4 insertion, 5 node insertion (aligner_cigar.hpp:19-26)
        static const char opc[] = "SX=DIG";
        s += "{\"annotation\":{\"cigar\":\"";
        for (uint32_t x = 0; x < a.n_cigar; ++x) s += std::to_string(cg[x].len) + opc[cg[x].op];
        s += '"';
        if (a.seq_len) { s += ",\"ref_sequence\":"; json_string(s, res->seqs + a.seq_begin, a.seq_len); }
        s += "},\"identity\":";
        json_double(s, qv_len ? (double)a.num_matches / (double)qv_len : 0.0);
        if (secondary) s += ",\"is_secondary\":true";
        s += ",\"name\":"; json_string(s, header, hl);
        if (a.n_nodes) {
            // path_json: mappings of the first node (may cover up to node_size characters), then one per further node
            const uint64_t *nodes = res->nodes + a.nodes_begin;
            uint32_t ci = 0;
            if (a.n_cigar && cg[0].op == 0) ++ci;
            uint64_t c_off = 0;
            const char *qs = qv;
            s += ",\"path\":{";
            if (nodes[0] == nodes[a.n_nodes - 1]) s += "\"is_circular\":true,";
            s += "\"length\":" + std::to_string(a.n_nodes) + ",\"mapping\":[";
            long long rank = 1;
            size_t cur = a.offset;
            {
                s += "{\"edit\":[";
                bool first = true;
                while (cur < k && ci < a.n_cigar) {
                    size_t next_pos = std::min<size_t>(k, cur + (cg[ci].len - c_off));
                    const size_t next_size = next_pos - cur;
                    const uint32_t op = cg[ci].op;
                    if (op == 0) { ++ci; c_off = 0; continue; }               // trailing clip
                    if (op == 1) { json_edit(s, first, (long long)next_size, qs, next_size, (long long)next_size); qs += next_size; }
                    else if (op == 4) { json_edit(s, first, -1, qs, next_size, (long long)next_size); qs += next_size; next_pos = cur; }
                    else if (op == 3) json_edit(s, first, (long long)next_size, nullptr, 0, -1);
                    else if (op == 2) { json_edit(s, first, (long long)next_size, nullptr, 0, (long long)next_size); qs += next_size; }
                    c_off += next_size;
                    cur = next_pos;
                    if (c_off == cg[ci].len) { ++ci; c_off = 0; }
                }
                s += "],\"position\":{\"node_id\":" + std::to_string(nodes[0]);
                if (a.offset) s += ",\"offset\":" + std::to_string(a.offset);
                s += "},\"rank\":" + std::to_string(rank++) + "}";
            }
            for (uint32_t ni = 1; ni < a.n_nodes && ci < a.n_cigar; ++ni) {
                s += ",{\"edit\":[";
                bool first = true;
                if (cg[ci].op == 4 || cg[ci].op == 0) {
                    const size_t len = cg[ci].len - c_off;
                    json_edit(s, first, -1, qs, len, (long long)len);
                    qs += len;
                    ++ci; c_off = 0;
                }
                if (ci < a.n_cigar) {
                    const uint32_t op = cg[ci].op;
                    if (op == 1) { json_edit(s, first, 1, qs, 1, 1); ++qs; }
                    else if (op == 3) json_edit(s, first, 1, nullptr, 0, -1);
                    else if (op == 2) { json_edit(s, first, 1, nullptr, 0, 1); ++qs; }
                    if (++c_off == cg[ci].len) { c_off = 0; ++ci; }
                }
                s += "],\"position\":{\"node_id\":" + std::to_string(nodes[ni]) + ",\"offset\":" + std::to_string(k - 1);
                s += "},\"rank\":" + std::to_string(rank++) + "}";
            }
            s += "],\"name\":\"\"}";
        }
        if (a.clipping) s += ",\"query_position\":" + std::to_string(a.clipping);
        s += std::string(",\"read_mapped\":") + (qv_len ? "true" : "false");
        if (a.orientation) s += ",\"read_on_reverse_strand\":true";
        s += ",\"score\":" + std::to_string(a.score);
        s += ",\"sequence\":"; json_string(s, full.data(), full.size());
        if (a.clipping) s += ",\"soft_clipped\":true";
        s += "}\n";
    }
    if (buf && buf_len) {
        size_t nc = std::min(buf_len - 1, s.size());
        memcpy(buf, s.data(), nc);
        buf[nc] = 0;
    }
    return s.size();
}

// ---- the `align --json` text of a range of a batch (json_format.hpp, mgx_jsonfmt.hip) -------------------------
enum { JF_CNT_SIZE = 0, JF_CNT_WRITE, JF_CNT_HOST_QUERIES, JF_CNT_D2H_BYTES };
static std::atomic<uint64_t> g_jsonfmt_counts[4];       // mgx_format_json_kernel_launch_counts
void mgx_format_json_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_jsonfmt_counts[x].load(); }

int mgx_format_json_batch(mgx_aligner *A, const char *headers, const uint64_t *header_offsets, uint64_t first, uint64_t n, mgx_text *out) {
    static_assert(sizeof(JfBatch) == MGX_JSONFMT_ARGS_BYTES, "JfBatch differs from what mgx_jsonfmt.hip takes");
    if (!A || !out || (n && (!headers || !header_offsets))) return fail(MGX_ERR_INVALID, "mgx_format_json_batch: null argument");
    if (int rc = refuse_chainer(A, "mgx_format_json_batch")) return rc;
    if (A->cfg.post_chain_alignments)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_format_json_batch: post_chain_alignments is set and JSON output for chains is not supported");
    const uint64_t n_batch = A->n_reads;
    if (first > n_batch || n > n_batch - first)
        return fail(MGX_ERR_INVALID, "mgx_format_json_batch: queries %llu .. %llu are beyond the staged batch of %llu", (unsigned long long)first,
                    (unsigned long long)(first + n), (unsigned long long)n_batch);
    A->h_line_begin.assign(n + 1, 0);
    out->n_queries = n; out->text = A->h_text ? A->h_text : ""; out->line_begin = A->h_line_begin.data();
    if (!n) return MGX_OK;
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    if (!(A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets))
        return fail(MGX_ERR_INVALID, "mgx_format_json_batch: no alignment batch staged: mgx_align_batch_device has not run on this handle, or a "
                                     "map / summary call ran since");
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "mgx_format_json_batch: more than 2^31 - 2 queries in a range");
    HIP_TRY(hipSetDevice(A->graph->device));
    const uint32_t k = A->graph->g.k;
    JfBatch b;
    FormatJob job = {};
    job.fn = "mgx_format_json_batch"; job.oom_advice = ": take a smaller range";
    job.size_launches = &g_jsonfmt_counts[JF_CNT_SIZE]; job.write_launches = &g_jsonfmt_counts[JF_CNT_WRITE];
    job.d2h_bytes = &g_jsonfmt_counts[JF_CNT_D2H_BYTES]; job.host_lines = &g_jsonfmt_counts[JF_CNT_HOST_QUERIES];
    job.launch_size = mgx_launch_jsonfmt_size; job.launch_write = mgx_launch_jsonfmt_write; job.params = &b; job.text = &b.text;
    job.headers = headers; job.header_offsets = header_offsets; job.header_from = header_offsets[0];    // (the kernels subtract it)
    job.first = first; job.n = n; job.n_batch = n_batch;
    job.bind = [&]() -> int {
        memset(&b, 0, sizeof(b));
        b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
        b.seqs = A->last_d_seqs; b.offsets = A->last_d_offsets;
        b.headers = A->tf_headers.as<char>(); b.header_from = job.header_from; b.header_offsets = A->tf_header_offsets.as<uint64_t>();
        b.line_len = A->tf_len.as<uint64_t>(); b.line_begin = A->tf_begin.as<uint64_t>();
        b.cap_list = A->tf_cap.as<uint32_t>(); b.cap_count = reinterpret_cast<unsigned long long *>(A->tf_begin.as<uint64_t>() + n + 1);
        b.first = first; b.n_queries = n; b.k = k; b.labeled = A->anno ? 1u : 0u;
        return MGX_OK;
    };
    job.host_line = [&](const mgx_results &v, const char *header, const char *query, size_t qlen) {
        return host_formatted([&](char *buf, size_t buf_len) { return mgx_format_json(&v, 0, header, query, qlen, k, buf, buf_len); });
    };
    return format_on_device(A, job, out);
}

} // extern "C"
