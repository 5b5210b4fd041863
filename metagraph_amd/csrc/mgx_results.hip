// mgx_results.hip — the results of an aligned batch on their way to the caller: the mgx_results arrays written by kernels
// (decode_on_device, mgx_decode_results_device) or decoded on the host (mgx_fetch_results), the raw records and stream
// (mgx_device_results, mgx_results_from_raw), post-chaining, and the capacity retry (realign_capacity_queries).  Host code: the
// kernels are mgx_decode.hip's.
#include <hip/hip_runtime.h>

#include <atomic>

#include "host_state.hpp"
#include "chain_host.hpp"
#include "kernel_units.hpp"
#include "results_decode.hpp"

using namespace mgx;
// the records the decode kernels write (results_decode.hpp) are the public ones, field by field
static_assert(sizeof(RdBatch) == MGX_DECODE_ARGS_BYTES, "RdBatch differs from what mgx_decode.hip takes");
static_assert(sizeof(RdCigarOp) == sizeof(mgx_cigar_op) && offsetof(RdCigarOp, len) == offsetof(mgx_cigar_op, len)
              && offsetof(RdCigarOp, op) == offsetof(mgx_cigar_op, op) && offsetof(RdCigarOp, pad) == offsetof(mgx_cigar_op, _pad),
              "RdCigarOp is not mgx_cigar_op");
static_assert(sizeof(RdAlignment) == sizeof(mgx_alignment) && offsetof(RdAlignment, score) == offsetof(mgx_alignment, score)
              && offsetof(RdAlignment, offset) == offsetof(mgx_alignment, offset) && offsetof(RdAlignment, clipping) == offsetof(mgx_alignment, clipping)
              && offsetof(RdAlignment, end_clipping) == offsetof(mgx_alignment, end_clipping)
              && offsetof(RdAlignment, num_matches) == offsetof(mgx_alignment, num_matches) && offsetof(RdAlignment, n_nodes) == offsetof(mgx_alignment, n_nodes)
              && offsetof(RdAlignment, n_cigar) == offsetof(mgx_alignment, n_cigar) && offsetof(RdAlignment, seq_len) == offsetof(mgx_alignment, seq_len)
              && offsetof(RdAlignment, nodes_begin) == offsetof(mgx_alignment, nodes_begin)
              && offsetof(RdAlignment, cigar_begin) == offsetof(mgx_alignment, cigar_begin) && offsetof(RdAlignment, seq_begin) == offsetof(mgx_alignment, seq_begin)
              && offsetof(RdAlignment, orientation) == offsetof(mgx_alignment, orientation) && offsetof(RdAlignment, pad) == offsetof(mgx_alignment, _pad)
              && offsetof(RdAlignment, n_labels) == offsetof(mgx_alignment, n_labels) && offsetof(RdAlignment, labels_begin) == offsetof(mgx_alignment, labels_begin),
              "RdAlignment is not mgx_alignment");
static_assert(sizeof(mgx_results_sizes) == RD_ARRAYS * 8, "mgx_results_sizes is the five totals in the order of RdArray");

static int retry_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, mgx_results *out);

extern "C" {

// ---- the mgx_results layout of a batch, written by kernels (results_decode.hpp, mgx_decode.hip): the one host
// sequence behind mgx_decode_results_device (RD_TO_DEVICE: `out` points at the device arrays) and the option decode_on_device of
// mgx_fetch_results (RD_TO_HOST: the seven arrays are copied to the handle's pinned buffers).  The caller has checked that the
// aligned batch is the staged one and that n = A->n_reads > 0.
enum { RD_CNT_SIZE = 0, RD_CNT_WRITE, RD_CNT_D2H_BYTES, RD_CNT_FETCHES };
static std::atomic<uint64_t> g_decode_counts[4];        // mgx_decode_kernel_launch_counts
void mgx_decode_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_decode_counts[x].load(); }

enum RdWhere { RD_TO_DEVICE, RD_TO_HOST };
static int decode_on_device(mgx_aligner *A, RdWhere where, mgx_results *out, mgx_results_sizes *sizes) {
    const char *fn = where == RD_TO_DEVICE ? "mgx_decode_results_device" : "mgx_fetch_results (decode_on_device=1)";
    const uint64_t n = A->n_reads;
    if (n >= 0x7FFFFFFFull) return fail(MGX_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 queries in a batch", fn);
    const uint64_t stride = n + 1;
    if (int rc = A->rd_counts.ensure(RD_ARRAYS * stride * 8)) return rc;
    if (int rc = A->rd_begins.ensure(RD_ARRAYS * stride * 8)) return rc;
    if (int rc = A->rd_totals.ensure(RD_ARRAYS * 8)) return rc;
    if (int rc = A->rd_status.ensure(n * 4 + 16)) return rc;
    uint64_t *d_counts = A->rd_counts.as<uint64_t>(), *d_begins = A->rd_begins.as<uint64_t>();
    RdBatch b;
    memset(&b, 0, sizeof(b));
    b.results = A->results.as<ReadResult>(); b.stream = A->stream.as<uint32_t>();
    b.counts = d_counts; b.begins = d_begins; b.status = A->rd_status.as<int32_t>();
    b.n_queries = n; b.stride = stride; b.labeled = A->anno ? 1u : 0u;
    // pass 1: what every query takes in the five arrays (and the zeros that close the scans); the scans give the begins
    HIP_TRY((hipError_t)mgx_launch_decode_size(&b, A->hstream));
    ++g_decode_counts[RD_CNT_SIZE];
    for (int x = 0; x < RD_ARRAYS; ++x) {
        if (int rc = exclusive_sum(A, d_counts + x * stride, d_begins + x * stride, n + 1)) return rc;
        // the totals side by side, so that one copy of 40 bytes brings them
        HIP_TRY(hipMemcpyAsync(A->rd_totals.as<uint64_t>() + x, d_begins + x * stride + n, 8, hipMemcpyDeviceToDevice, A->hstream));
    }
    uint64_t total[RD_ARRAYS] = { 0, 0, 0, 0, 0 };
    HIP_TRY(copy_sync(A, total, A->rd_totals.p, sizeof(total), hipMemcpyDeviceToHost));
    g_decode_counts[RD_CNT_D2H_BYTES] += sizeof(total);
    // pass 2: the arrays
    const size_t bytes[mgx_aligner::RD_H_N] = { (size_t)(n + 1) * 8, (size_t)total[RD_ALN] * sizeof(mgx_alignment), (size_t)total[RD_NODES] * 8,
                                                (size_t)total[RD_CIGAR] * sizeof(mgx_cigar_op), (size_t)total[RD_SEQ], (size_t)n * 4,
                                                (size_t)total[RD_LABELS] * 4 };
    size_t all_bytes = 0;
    for (size_t x : bytes) all_bytes += x;
    auto no_buffer = [&](const char *which) {
        return fail(MGX_ERR_OOM, "%s: the results of %llu queries need %llu bytes and no %s buffer of that size could be allocated", fn,
                    (unsigned long long)n, (unsigned long long)all_bytes, which);
    };
    // (16 bytes more than needed: an array without elements still has an address)
    if (A->rd_alns.ensure(bytes[mgx_aligner::RD_H_ALNS] + 16) != MGX_OK || A->rd_nodes.ensure(bytes[mgx_aligner::RD_H_NODES] + 16) != MGX_OK
        || A->rd_cigar.ensure(bytes[mgx_aligner::RD_H_CIGAR] + 16) != MGX_OK || A->rd_seqs.ensure(bytes[mgx_aligner::RD_H_SEQS] + 16) != MGX_OK
        || A->rd_labels.ensure(bytes[mgx_aligner::RD_H_LABELS] + 16) != MGX_OK)
        return no_buffer("device");
    b.alignments = A->rd_alns.as<RdAlignment>(); b.nodes = A->rd_nodes.as<uint64_t>(); b.cigar = A->rd_cigar.as<RdCigarOp>();
    b.seqs = A->rd_seqs.as<char>(); b.labels = A->rd_labels.as<uint32_t>();
    HIP_TRY((hipError_t)mgx_launch_decode_write(&b, A->hstream));
    ++g_decode_counts[RD_CNT_WRITE];
    const void *d_arrays[mgx_aligner::RD_H_N] = { d_begins + RD_ALN * stride, A->rd_alns.p, A->rd_nodes.p, A->rd_cigar.p, A->rd_seqs.p, A->rd_status.p,
                                                  A->rd_labels.p };
    const void *arrays[mgx_aligner::RD_H_N];
    if (where == RD_TO_DEVICE) {
        HIP_TRY(hipStreamSynchronize(A->hstream));       // (the arrays are complete when the call returns, whatever stream reads them)
        for (int x = 0; x < mgx_aligner::RD_H_N; ++x) arrays[x] = d_arrays[x];
    } else {
        for (int x = 0; x < mgx_aligner::RD_H_N; ++x) {
            if (bytes[x] + 1 > A->h_rd_bytes[x]) {
                if (A->h_rd[x]) { (void)hipHostFree(A->h_rd[x]); A->h_rd[x] = nullptr; A->h_rd_bytes[x] = 0; }
                const size_t want = bytes[x] + bytes[x] / 8 + 4096;
                void *p = nullptr;
                if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return no_buffer("pinned host"); }
                A->h_rd[x] = p; A->h_rd_bytes[x] = want;
            }
            if (bytes[x]) HIP_TRY(hipMemcpyAsync(A->h_rd[x], d_arrays[x], bytes[x], hipMemcpyDeviceToHost, A->hstream));
            g_decode_counts[RD_CNT_D2H_BYTES] += bytes[x];
            arrays[x] = A->h_rd[x];
        }
        HIP_TRY(hipStreamSynchronize(A->hstream));
    }
    out->n_queries = n;
    out->aln_begin = static_cast<const uint64_t *>(arrays[mgx_aligner::RD_H_ALN_BEGIN]);
    out->alignments = static_cast<const mgx_alignment *>(arrays[mgx_aligner::RD_H_ALNS]);
    out->nodes = static_cast<const uint64_t *>(arrays[mgx_aligner::RD_H_NODES]);
    out->cigar = static_cast<const mgx_cigar_op *>(arrays[mgx_aligner::RD_H_CIGAR]);
    out->seqs = static_cast<const char *>(arrays[mgx_aligner::RD_H_SEQS]);
    out->status = static_cast<const int32_t *>(arrays[mgx_aligner::RD_H_STATUS]);
    out->labels = total[RD_LABELS] ? static_cast<const uint32_t *>(arrays[mgx_aligner::RD_H_LABELS]) : nullptr;     // (as HostResults::view)
    if (sizes) {
        sizes->n_alignments = total[RD_ALN]; sizes->n_nodes = total[RD_NODES]; sizes->n_cigar = total[RD_CIGAR];
        sizes->n_seq_bytes = total[RD_SEQ]; sizes->n_labels = total[RD_LABELS];
    }
    return MGX_OK;
}

int mgx_decode_results_device(mgx_aligner *A, mgx_results *out, mgx_results_sizes *sizes) {
    if (!A || !out || !sizes) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = refuse_chainer(A, "mgx_decode_results_device")) return rc;
    const uint64_t n = A->n_reads;
    memset(sizes, 0, sizeof(*sizes));
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    const bool staged = n ? A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets : A->aligned_empty;
    if (!staged)
        return fail(MGX_ERR_INVALID, "mgx_decode_results_device: no aligned batch on this handle, or another batch was staged after mgx_align_batch_device");
    HIP_TRY(hipSetDevice(A->graph->device));
    if (!n) {
        // no query: aln_begin is its one zero, every other array is empty (and has an address)
        if (int rc = A->rd_begins.ensure(64)) return rc;
        HIP_TRY(hipMemsetAsync(A->rd_begins.p, 0, 64, A->hstream));
        HIP_TRY(hipStreamSynchronize(A->hstream));
        memset(out, 0, sizeof(*out));
        out->aln_begin = A->rd_begins.as<uint64_t>();
        out->alignments = reinterpret_cast<const mgx_alignment *>(A->rd_begins.as<uint64_t>() + 1);
        out->nodes = A->rd_begins.as<uint64_t>() + 1;
        out->cigar = reinterpret_cast<const mgx_cigar_op *>(A->rd_begins.as<uint64_t>() + 1);
        out->seqs = reinterpret_cast<const char *>(A->rd_begins.as<uint64_t>() + 1);
        out->status = reinterpret_cast<const int32_t *>(A->rd_begins.as<uint64_t>() + 1);
        return MGX_OK;
    }
    return decode_on_device(A, RD_TO_DEVICE, out, sizes);
}

int mgx_fetch_results(mgx_aligner *A, mgx_results *out) {
    HostStageTimer t_fetch("fetch_results");
    if (int rc = refuse_chainer(A, "mgx_fetch_results")) return rc;
    const uint64_t n = A->n_reads;
    HIP_TRY(hipSetDevice(A->graph->device));
    // the aligned batch is read back below (post-chaining, the capacity retry): only while the staging buffers still hold it —
    // mgx_map_batch on this aligner re-stages them; a caller's device buffers are the caller's to keep until the fetch
    const bool batch_intact = A->aligned_generation == A->stage_generation && A->last_d_seqs && A->last_d_offsets;
    if (A->opt.decode_on_device && n && batch_intact) {
        // the option decode_on_device: the seven arrays come decoded (no records, no stream, no per-element work here)
        A->h_results.clear();                            // (mgx_fetch_seed_info reads the records itself)
        mgx_results_sizes sizes;
        if (int rc = decode_on_device(A, RD_TO_HOST, out, &sizes)) return rc;
        ++g_decode_counts[RD_CNT_FETCHES];
        // the capacity retry tells a queue overflow (final) from an arena overflow by the record: the rare batch with a capacity
        // status brings its records as well
        if (std::find(out->status, out->status + n, (int32_t)MGX_ERR_CAPACITY) != out->status + n) {
            A->h_results.resize(n);
            HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
            g_decode_counts[RD_CNT_D2H_BYTES] += n * sizeof(ReadResult);
        }
    } else {
        A->h_results.resize(n);
        unsigned long long used = 0;
        if (n) {
            HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
            HIP_TRY(copy_sync(A, &used, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
            used = std::min<unsigned long long>(used, A->out_words);
        }
        A->h_stream.resize(used);
        if (used) HIP_TRY(copy_sync(A, A->h_stream.data(), A->stream.p, used * 4, hipMemcpyDeviceToHost));
        A->host.decode(A->h_results.data(), n, A->h_stream.data(), ~0ull, A->anno != nullptr);
        A->host.view(out);
    }
    if (A->cfg.post_chain_alignments && n) {
        // chain_alignments (dbg_aligner.cpp:328-332) on the host: needs the reads of the queries with two or more alignments once
        // more — one transfer of the span of the batch that holds them (none at all when no query has two)
        uint64_t q_lo = n, q_hi = 0;
        for (uint64_t q = 0; q < n; ++q) if (out->aln_begin[q + 1] - out->aln_begin[q] >= 2) { q_lo = std::min(q_lo, q); q_hi = q + 1; }
        if (!batch_intact)
            return fail(MGX_ERR_INVALID, "post_chain_alignments: another batch was staged on this aligner between mgx_align_batch_device and mgx_fetch_results");
        std::vector<uint64_t> offs(n + 1, 0);
        HIP_TRY(copy_sync(A, offs.data(), A->last_d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
        std::vector<char> reads(1);
        uint64_t b0 = 0;
        if (q_lo < q_hi) {
            b0 = offs[q_lo];
            const uint64_t b1 = offs[q_hi];
            reads.resize(b1 - b0 + 1);
            if (b1 > b0) HIP_TRY(copy_sync(A, reads.data(), A->last_d_seqs + b0, b1 - b0, hipMemcpyDeviceToHost));
        }
        mgx_results plain = *out;
        chain_results(plain, reads.data(), offs.data(), A->cfg, A->graph->g.k, &A->host_chained, b0);
        A->host_chained.view(out);
    }
    // reads the batch's limits were too small for: once more, with larger ones (below)
    if (!batch_intact) return MGX_OK;              // (statuses stay: the reads are no longer where they were)
    return retry_capacity_queries(A, A->last_d_seqs, A->last_d_offsets, n, out);
}

int mgx_device_results(mgx_aligner *A, const void **headers, uint64_t *header_bytes, uint64_t *n_queries,
                       const void **stream, uint64_t *stream_words) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = refuse_chainer(A, "mgx_device_results")) return rc;
    unsigned long long used = 0;
    if (A->n_reads) HIP_TRY(copy_sync(A, &used, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
    used = std::min<unsigned long long>(used, A->out_words);
    *headers = A->results.p; *header_bytes = sizeof(ReadResult); *n_queries = A->n_reads;
    *stream = A->stream.p; *stream_words = used;
    return MGX_OK;
}

uint64_t mgx_device_stream_capacity(const mgx_aligner *A) { return A ? A->out_words : 0; }

struct mgx_raw_store { HostResults host; };

int mgx_results_from_raw(const void *headers, uint64_t n, const uint32_t *stream, uint64_t stream_words,
                         mgx_raw_store **store, mgx_results *out) {
    return mgx_results_from_raw_labeled(headers, n, stream, stream_words, 0, store, out);
}
int mgx_results_from_raw_labeled(const void *headers, uint64_t n, const uint32_t *stream, uint64_t stream_words, int labeled,
                                 mgx_raw_store **store, mgx_results *out) {
    if ((!headers && n) || !store || !out || (!stream && stream_words)) return fail(MGX_ERR_INVALID, "null argument");
    const ReadResult *rr = static_cast<const ReadResult *>(headers);
    auto *S = new mgx_raw_store();
    if (!S->host.decode(rr, n, stream, stream_words, labeled != 0)) {
        delete S;
        return fail(MGX_ERR_INVALID, "a record points outside the stream (%llu words)", (unsigned long long)stream_words);
    }
    S->host.view(out);
    *store = S;
    return MGX_OK;
}

void mgx_raw_store_free(mgx_raw_store *store) { delete store; }

// chain_alignments (aligner_chainer.cpp:555-720) over decoded results — what mgx_fetch_results does itself when the aligner's
// config has post_chain_alignments set; for results decoded elsewhere (mgx_results_from_raw after a gather).  Host code.
int mgx_chain_alignments(const mgx_config *config, uint32_t k, const mgx_results *in, const char *seqs, const uint64_t *offsets,
                         mgx_raw_store **store, mgx_results *out) {
    if (!config || !in || !store || !out || (in->n_queries && (!seqs || !offsets))) return fail(MGX_ERR_INVALID, "null argument");
    if (k < 2) return fail(MGX_ERR_INVALID, "k out of range");
    auto *S = new mgx_raw_store();
    chain_results(*in, seqs, offsets, *config, k, &S->host);
    S->host.view(out);
    *store = S;
    return MGX_OK;
}

} // extern "C"

// Queries whose per-read arenas overflowed (status MGX_ERR_CAPACITY: the reference has no such limit, its tables grow on the
// heap) are aligned again by a temporary aligner with doubled limits, up to six doublings, and take their place in the
// results — what the C++ adapter (host/hip_dbg_aligner.hpp) did for its callers since round 2, now for every caller of
// mgx_fetch_results / mgx_align_batch (the Python binding and the device-resident batches among them).  What doubling cannot cure stays a capacity status: a query with more
// alignments than the post_chain_alignments queue holds.  (Label-aware alignment: the retry also doubles the label arenas —
// alignments per backtracking, aggregator pool, label queues, label sets; derive_limits' label_scale.)
// The re-alignment itself, for the queries `todo` (ascending) of the batch the device holds: fixed[t] = the results of todo[t]
// where have[t]; h_off = the batch's offsets, h_seq = its bytes from h_off[todo.front()] on (mgx_format_tsv_batch prints from them).
int realign_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, const std::vector<uint64_t> &todo,
                             std::vector<HostResults> &fixed, std::vector<uint8_t> &have, std::vector<uint64_t> &h_off,
                             std::vector<char> &h_seq) {
    // the reads in question, from the batch as the device holds it (the caller's buffers, or the upload of a host batch): ONE
    // transfer of the span of the batch between the first and the last of them
    h_off.resize(n + 1);
    HIP_TRY(copy_sync(A, h_off.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t b0 = h_off[todo.front()], b1 = h_off[todo.back() + 1];
    h_seq.resize(b1 - b0 + 1);
    if (b1 > b0) HIP_TRY(copy_sync(A, h_seq.data(), d_seqs + b0, b1 - b0, hipMemcpyDeviceToHost));
    const char *seqs = h_seq.data();
    auto seq_of = [&](uint64_t q) { return seqs + (h_off[q] - b0); };
    const uint64_t *offsets = h_off.data();
    // results so far, query by query (replaced below)
    fixed.assign(todo.size(), HostResults());
    have.assign(todo.size(), 0);
    mgx_limits lim;
    mgx_aligner_get_limits(A, &lim);
    mgx_aligner *tmp = nullptr;
    struct Guard { mgx_aligner *&p; ~Guard() { if (p) mgx_aligner_destroy(p); } } guard{ tmp };
    std::vector<uint64_t> pending(todo.size());
    for (size_t t = 0; t < todo.size(); ++t) pending[t] = t;
    for (int attempt = 0; attempt < 6 && !pending.empty(); ++attempt) {
        lim.max_query_length = 0;                       // the (smaller) batch sets its own
        lim.max_columns = lim.max_columns * 2;
        lim.max_seeds = std::min<uint32_t>(65535u, lim.max_seeds * 2);
        lim.cell_arena_bytes = lim.cell_arena_bytes * 2;
        if (tmp) { mgx_aligner_destroy(tmp); tmp = nullptr; }
        // (an attempt that fails — out of memory at the inflated limits, say — ends the retry: what the batch and the earlier
        // attempts produced stays valid and is what the caller gets, statuses included)
        if (aligner_create(A->graph, &A->cfg, &lim, A->anno, &tmp) != MGX_OK) break;
        tmp->opt = A->opt; tmp->no_fast = A->no_fast;
        tmp->hstream = A->hstream;                        // (borrowed: the retry runs where the batch ran)
        tmp->retry_capacity = false;
        tmp->label_scale = 2u << attempt;
        std::string blob;
        std::vector<uint64_t> offs(pending.size() + 1, 0);
        for (size_t t = 0; t < pending.size(); ++t) {
            const uint64_t q = todo[pending[t]];
            blob.append(seq_of(q), offsets[q + 1] - offsets[q]);
            offs[t + 1] = blob.size();
        }
        mgx_results sub{};
        if (mgx_align_batch(tmp, blob.data(), offs.data(), pending.size(), 0, &sub) != MGX_OK) break;
        std::vector<uint64_t> again;
        for (size_t t = 0; t < pending.size(); ++t) {
            if (sub.status[t] == MGX_ERR_CAPACITY) {
                // (its queue overflowed this time: final)
                if (!(t < tmp->h_results.size() && tmp->h_results[t].orientation == RR_CAUSE_QUEUE)) again.push_back(pending[t]);
                continue;
            }
            fixed[pending[t]].append_query(sub, t);
            have[pending[t]] = 1;
        }
        pending.swap(again);
        mgx_aligner_get_limits(tmp, &lim);
    }
    return MGX_OK;
}

static int retry_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, mgx_results *out) {
    std::vector<uint64_t> todo;
    // (a query whose post_chain_alignments queue overflowed is flagged by the kernel — RR_CAUSE_QUEUE — and stays a status: no
    // limit cures it, and six rounds of ever larger arenas would be paid for nothing)
    for (uint64_t q = 0; q < n; ++q)
        if (out->status[q] == MGX_ERR_CAPACITY && !(q < A->h_results.size() && A->h_results[q].orientation == RR_CAUSE_QUEUE)) todo.push_back(q);
    if (todo.empty() || !A->retry_capacity || !d_seqs || !d_offsets) return MGX_OK;
    std::vector<HostResults> fixed;
    std::vector<uint8_t> have;
    std::vector<uint64_t> h_off;
    std::vector<char> h_seq;
    if (int rc = realign_capacity_queries(A, d_seqs, d_offsets, n, todo, fixed, have, h_off, h_seq)) return rc;
    bool any = false;
    for (uint8_t h : have) any |= h != 0;
    if (!any) return MGX_OK;
    HostResults merged;
    size_t t = 0;
    for (uint64_t q = 0; q < n; ++q) {
        if (t < todo.size() && todo[t] == q) {
            if (have[t]) { mgx_results v; fixed[t].view(&v); merged.append_query(v, 0); }
            else merged.append_query(*out, q);
            ++t;
        } else merged.append_query(*out, q);
    }
    A->host_retried = std::move(merged);
    A->host_retried.view(out);
    A->hstats.n_capacity_retried = (uint64_t)std::count(have.begin(), have.end(), (uint8_t)1);
    return MGX_OK;
}

extern "C" {

int mgx_align_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device, mgx_results *out) {
    if (!out) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = mgx_align_batch_device(A, seqs, offsets, n, on_device)) return rc;
    return mgx_fetch_results(A, out);          // (with the capacity retry)
}

// test hook: keep the per-read seed lists of the next batches (device -> mgx_fetch_seeds)
void mgx_aligner_keep_seeds(mgx_aligner *A, int keep) { A->keep_seeds = keep != 0; }

// per read: num_matches fwd/rc, n_seeds fwd/rc, n_extensions, n_columns (6 x u32), and optionally the seeds
int mgx_fetch_seed_info(mgx_aligner *A, uint32_t *info6, uint32_t *seeds /* [n][2][max_seeds][4] or NULL */, uint32_t *max_seeds_out) {
    if (int rc = refuse_chainer(A, "mgx_fetch_seed_info")) return rc;
    const uint64_t n = A->n_reads;
    if (A->h_results.size() != n || n == 0) {
        A->h_results.resize(n);
        if (n) HIP_TRY(copy_sync(A, A->h_results.data(), A->results.p, n * sizeof(ReadResult), hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < n; ++i) {
        const ReadResult &r = A->h_results[i];
        uint32_t *o = info6 + 6 * i;
        o[0] = r.num_matches_fwd; o[1] = r.num_matches_rc; o[2] = r.n_seeds_fwd; o[3] = r.n_seeds_rc;
        o[4] = r.n_extensions; o[5] = r.n_columns;
    }
    if (max_seeds_out) *max_seeds_out = A->lim.max_seeds;
    if (seeds && A->keep_seeds && n) {
        std::vector<DevSeed> h(n * 2 * (uint64_t)A->lim.max_seeds);
        HIP_TRY(copy_sync(A, h.data(), A->dbg_seeds.p, h.size() * sizeof(DevSeed), hipMemcpyDeviceToHost));
        for (size_t x = 0; x < h.size(); ++x) {
            seeds[4 * x] = h[x].clipping; seeds[4 * x + 1] = h[x].length; seeds[4 * x + 2] = h[x].offset;
            seeds[4 * x + 3] = h[x].offset ? h[x].node : h[x].n_nodes;
        }
    }
    return MGX_OK;
}

} // extern "C"
