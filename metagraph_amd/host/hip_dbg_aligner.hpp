// hip_dbg_aligner.hpp — C++ host adapter: MetaGraph's aligner operator surface over the C-ABI.
//
// Mirrors, name for name, what `metagraph align` consumes from graph/alignment:
//   IDBGAligner::align_batch / align / get_config      (dbg_aligner.hpp:20-39, dbg_aligner.cpp:22-31)
//   Query, AlignmentCallback                            (dbg_aligner.hpp:22-24)
//   AlignmentResults (normalised query + RC + alignments, alignment.hpp:366-406; ctor alignment.cpp:1348-1372)
//   Alignment getters + Cigar::to_string                (alignment.hpp:132-331, aligner_cigar.cpp:86-96)
//   format_alignment TSV                                (cli/align.cpp:254-285)
// Header-only; links against libmgx.so only (include/mgx.h).  Callbacks are invoked once per query, in
// batch order, on the calling thread, like DBGAligner::align_batch (dbg_aligner.cpp:263,353).
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <algorithm>
#include <stdexcept>
#include <cstdlib>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/mgx.h"

namespace mgx {
namespace host {

typedef mgx_config DBGAlignerConfig;      // field-for-field mirror (aligner_config.hpp:18-94)
typedef uint64_t node_index;

class Cigar {
  public:
    typedef std::pair<uint8_t, uint32_t> value_type;
    const std::vector<value_type> &data() const { return cigar_; }
    std::vector<value_type> &data() { return cigar_; }
    std::string to_string() const {
        static const char op_str[] = "SX=DIG";
        std::string s;
        for (const auto &p : cigar_) s += std::to_string(p.second) + op_str[p.first];
        return s;
    }
    size_t get_num_matches() const {
        size_t n = 0;
        for (const auto &p : cigar_) n += (p.first == MGX_OP_MATCH) * p.second;
        return n;
    }
    uint32_t get_clipping() const { return cigar_.size() && cigar_.front().first == MGX_OP_CLIPPED ? cigar_.front().second : 0; }
    uint32_t get_end_clipping() const { return cigar_.size() && cigar_.back().first == MGX_OP_CLIPPED ? cigar_.back().second : 0; }
  private:
    std::vector<value_type> cigar_;
};

class Alignment {
  public:
    std::string_view get_query_view() const { return query_view_; }
    const std::vector<node_index> &get_nodes() const { return nodes_; }
    std::string_view get_sequence() const { return sequence_; }
    size_t get_offset() const { return offset_; }
    size_t size() const { return nodes_.size(); }
    bool empty() const { return nodes_.empty(); }
    bool get_orientation() const { return orientation_; }
    int32_t get_score() const { return score_; }
    const Cigar &get_cigar() const { return cigar_; }
    uint32_t get_clipping() const { return cigar_.get_clipping(); }
    uint32_t get_end_clipping() const { return cigar_.get_end_clipping(); }
    // Alignment::label_columns (alignment.hpp:285): the labels of a label-aware aligner's alignment, ascending; else empty
    const std::vector<uint64_t> &get_label_columns() const { return label_columns_; }
    // fmt formatter of the reference (alignment.hpp:426-433)
    std::string to_tsv_fields() const {
        return std::string(orientation_ ? "-" : "+") + "\t" + sequence_ + "\t" + std::to_string(score_) + "\t"
            + std::to_string(cigar_.get_num_matches()) + "\t" + cigar_.to_string() + "\t" + std::to_string(offset_);
    }
  private:
    friend class HipDBGAligner;
    std::string_view query_view_;
    std::vector<node_index> nodes_;
    bool orientation_ = false;
    size_t offset_ = 0;
    std::string sequence_;
    int32_t score_ = 0;
    Cigar cigar_;
    std::vector<uint64_t> label_columns_;
};

class AlignmentResults {
  public:
    explicit AlignmentResults(std::string_view query = {}) {
        // alignment.cpp:1348-1372: upper-case, bytes < 0 -> 127, SSO disabled, reverse complement
        query_.reserve(std::max<size_t>(query.size(), 32) + 8);
        for (char ch : query) {
            int8_t c = (int8_t)ch;
            query_.push_back(c >= 0 ? (char)toupper(c) : (char)127);
        }
        query_rc_.reserve(query_.capacity());
        query_rc_.assign(query_.rbegin(), query_.rend());
        for (char &c : query_rc_) c = complement(c);
    }
    AlignmentResults(const AlignmentResults &) = delete;
    AlignmentResults &operator=(const AlignmentResults &) = delete;
    AlignmentResults(AlignmentResults &&) = default;
    AlignmentResults &operator=(AlignmentResults &&) = default;
    const std::string &get_query(bool reverse_complement = false) const { return reverse_complement ? query_rc_ : query_; }
    size_t size() const { return alignments_.size(); }
    bool empty() const { return alignments_.empty(); }
    const Alignment &operator[](size_t i) const { return alignments_[i]; }
    auto begin() const { return alignments_.begin(); }
    auto end() const { return alignments_.end(); }
  private:
    friend class HipDBGAligner;
    static char complement(char c) {      // COMPL_TAB (common/seq_tools/reverse_complement.hpp:31-48)
        static const char up[] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
        unsigned char u = (unsigned char)c;
        if (u >= 'A' && u <= 'Z') return up[u - 'A'];
        if (u >= 'a' && u <= 'z') return (char)(up[u - 'a'] + 32);
        if (u == 96) return 64;
        return c;
    }
    std::string query_, query_rc_;
    std::vector<Alignment> alignments_;
};

// The graph handle the aligner holds a reference to (DBGSuccinct's role for this path)
class HipBOSSGraph {
  public:
    // W/last: one byte per edge, n_edges + 1 entries; valid may be null (reset_mask(), cli/align.cpp:337-339)
    HipBOSSGraph(uint32_t k, uint64_t n_edges, const uint8_t *W, const uint8_t *last, const uint64_t F[5],
                 const uint8_t *valid = nullptr, int device = 0, uint32_t mode = MGX_MODE_BASIC) {
        mgx_boss_view v{};
        v.k = k; v.sigma = 5; v.n_edges = n_edges; v.W = W; v.last = last; v.F = F; v.valid = valid;
        v.mode = mode; v.on_device = 0;          // DeBruijnGraph::get_mode(); PRIMARY graphs are aligned through CanonicalDBG
        if (int rc = mgx_graph_create(&v, device, &g_)) throw std::runtime_error(std::string("mgx_graph_create: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    // a `.dbg` file written by the reference (DBGSuccinct::load); load_on_device: its payloads are decoded by kernels
    // (mgx_graph_load_dbg_device) instead of on this thread — the same graph
    explicit HipBOSSGraph(const std::string &dbg_path, int device = 0, bool load_on_device = false) {
        const int rc = load_on_device ? mgx_graph_load_dbg_device(dbg_path.c_str(), device, &g_) : mgx_graph_load_dbg(dbg_path.c_str(), device, &g_);
        if (rc) throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
    }
    ~HipBOSSGraph() { mgx_graph_destroy(g_); }
    HipBOSSGraph(const HipBOSSGraph &) = delete;
    size_t get_k() const { return mgx_graph_k(g_); }
    uint64_t max_index() const { return mgx_graph_max_index(g_); }
    mgx_graph *handle() const { return g_; }
  private:
    mgx_graph *g_ = nullptr;
};

// In-process multi-GPU (the natural drop-in for `metagraph align`, which is ONE process with a pool of batch tasks,
// cli/align.cpp:440-475): one replica of the graph per device; worker w of the pool aligns its batches on device w % D.  Reads
// shard by batch, the graph is replicated, nothing is exchanged between devices — results come back per batch on the host.
class HipGraphSet {
  public:
    HipGraphSet(int n_devices, uint32_t k, uint64_t n_edges, const uint8_t *W, const uint8_t *last, const uint64_t F[5],
                const uint8_t *valid = nullptr, uint32_t mode = MGX_MODE_BASIC) {
        if (n_devices < 1) throw std::runtime_error("HipGraphSet: at least one device");
        for (int d = 0; d < n_devices; ++d) replicas_.emplace_back(new HipBOSSGraph(k, n_edges, W, last, F, valid, d, mode));
    }
    HipGraphSet(int n_devices, const std::string &dbg_path, bool load_on_device = false) {
        if (n_devices < 1) throw std::runtime_error("HipGraphSet: at least one device");
        for (int d = 0; d < n_devices; ++d) replicas_.emplace_back(new HipBOSSGraph(dbg_path, d, load_on_device));
    }
    size_t size() const { return replicas_.size(); }
    static size_t device_of_worker(size_t worker, size_t n_devices) { return worker % n_devices; }
    const HipBOSSGraph &for_worker(size_t worker) const { return *replicas_[device_of_worker(worker, replicas_.size())]; }
  private:
    std::vector<std::unique_ptr<HipBOSSGraph>> replicas_;
};

// what the format_batch* methods of the two handle classes below share (no part of the interface)
namespace detail {
constexpr uint64_t ANY_BATCH = ~0ull;
// the view of the text a mgx_format_*_batch call (`fn`) returned with `rc`; n_queries: the size the handle's batch must have
inline std::string_view text_view(int rc, const mgx_text &text, const char *fn, uint64_t n_queries = ANY_BATCH) {
    if (rc) throw std::runtime_error(std::string(fn) + ": " + mgx_last_error() + " (" + std::to_string(rc) + ")");
    if (n_queries != ANY_BATCH && text.n_queries != n_queries) throw std::runtime_error(std::string(fn) + ": the handle's batch is not this one");
    return std::string_view(text.text, (size_t)text.line_begin[text.n_queries]);
}
// name_offsets[0 .. n] counted from name_offsets[0]
inline std::vector<uint64_t> rebased(const uint64_t *name_offsets, uint64_t n) {
    std::vector<uint64_t> offsets(n + 1);
    for (uint64_t t = 0; t <= n; ++t) offsets[t] = name_offsets[t] - name_offsets[0];
    return offsets;
}
}  // namespace detail

// DeBruijnGraph::map_to_nodes / DeBruijnGraph::find on the device graph — the graph-side calls behind `metagraph align --map`
// (map_sequences_in_file, cli/align.cpp:71-179).  Holds a device handle of its own; one per worker thread.  The batched form is
// the one to use: a single sequence pays a whole launch.
class HipGraphMapper {
  public:
    explicit HipGraphMapper(const HipBOSSGraph &graph) : graph_(graph) {
        mgx_config cfg;
        mgx_config_init_cli(&cfg, (uint32_t)graph.get_k());
        if (int rc = mgx_aligner_create(graph.handle(), &cfg, nullptr, &a_))
            throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
    }
    ~HipGraphMapper() { mgx_aligner_destroy(a_); }
    HipGraphMapper(const HipGraphMapper &) = delete;
    // The view of the whole batch (valid until the next call): counts per sequence and, with want_nodes, the node arrays.
    // map_length: 0 = k; L < k = the windows of --align-length L (BASIC and CANONICAL graphs).  keep_nodes: the node array stays in
    // device memory for format_batch(.., MGX_MAP_FMT_NODES) and nothing more comes to the host.
    mgx_map_summary map_batch(const std::vector<std::string_view> &seqs, uint32_t map_length = 0, bool want_nodes = false, bool keep_nodes = false) const {
        std::string blob;
        std::vector<uint64_t> offsets(seqs.size() + 1, 0);
        for (size_t t = 0; t < seqs.size(); ++t) { blob.append(seqs[t].data(), seqs[t].size()); offsets[t + 1] = blob.size(); }
        if (blob.empty()) blob.push_back('\0');
        mgx_map_summary out{};
        if (int rc = mgx_map_summary_batch(a_, blob.data(), offsets.data(), seqs.size(), 0, map_length,
                                           (want_nodes ? MGX_MAP_WANT_NODES : 0u) | (keep_nodes ? MGX_MAP_KEEP_NODES : 0u), &out))
            throw std::runtime_error(std::string("mgx_map_summary_batch: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
        return out;
    }
    // ... over reads that are in device memory already (HipReadParser::slice): n reads, offsets from 0
    mgx_map_summary map_batch_device(const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t map_length, bool keep_nodes) const {
        mgx_map_summary out{};
        if (int rc = mgx_map_summary_batch(a_, d_seqs, d_offsets, n, 1, map_length, keep_nodes ? MGX_MAP_KEEP_NODES : 0, &out))
            throw std::runtime_error(std::string("mgx_map_summary_batch: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
        return out;
    }
    // The text map_sequences_in_file prints for the batch mapped last, written on the device (mgx_format_map_batch): what
    // mgx_format_map gives for every query, in query order.  names / name_offsets: the headers as flat arrays, `name_offsets`
    // points at the batch's first record (n + 1 entries).  The view is the handle's and stays valid until its next batch.
    std::string_view format_batch(const char *names, const uint64_t *name_offsets, uint64_t n, int format, double discovery_fraction) const {
        const std::vector<uint64_t> offsets = detail::rebased(name_offsets, n);
        mgx_text text{};
        const int rc = mgx_format_map_batch(a_, names + name_offsets[0], offsets.data(), format, discovery_fraction, &text);
        return detail::text_view(rc, text, "mgx_format_map_batch", n);
    }
    // std::vector<node_index> map_to_nodes(const DeBruijnGraph &, std::string_view) (sequence_graph.cpp)
    std::vector<uint64_t> map_to_nodes(std::string_view sequence) const {
        const mgx_map_summary s = map_batch({ sequence }, 0, true);
        return std::vector<uint64_t>(s.nodes + s.node_begin[0], s.nodes + s.node_begin[1]);
    }
    // bool DeBruijnGraph::find(std::string_view sequence, double discovery_fraction = 1) (sequence_graph.cpp:65-89)
    bool find(std::string_view sequence, double discovery_fraction = 1) const {
        const mgx_map_summary s = map_batch({ sequence });
        return mgx_map_present(&s.counts[0], sequence.size(), (uint32_t)graph_.get_k(), 0, discovery_fraction) != 0;
    }
    void set_kernel_option(const std::string &opt) {
        if (int rc = mgx_aligner_set_pipeline(a_, opt.c_str()))
            throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
    }
    const HipBOSSGraph &get_graph() const { return graph_; }
  private:
    const HipBOSSGraph &graph_;
    mgx_aligner *a_ = nullptr;
};

class IDBGAligner {
  public:
    typedef std::pair<std::string /* header */, std::string /* seq */> Query;
    typedef std::function<void(const std::string & /* header */, AlignmentResults && /* alignments */)> AlignmentCallback;
    virtual ~IDBGAligner() {}
    virtual const HipBOSSGraph &get_graph() const = 0;
    virtual const DBGAlignerConfig &get_config() const = 0;
    virtual void align_batch(const std::vector<Query> &seq_batch, const AlignmentCallback &callback) const = 0;
    AlignmentResults align(std::string_view query) const {          // dbg_aligner.cpp:22-31
        AlignmentResults result;
        align_batch({ Query{ std::string{}, std::string(query) } },
                    [&](const std::string &, AlignmentResults &&alignment) { std::swap(result, alignment); });
        return result;
    }
    virtual bool has_coordinates() const = 0;
};

// The annotator argument of LabeledAligner<> (aligner_labeled.hpp:125-127): the label matrix on the graph's device, from the
// set rows of every column (what a ColumnCompressed annotation stores; row = AnnotatedDBG::graph_to_anno_index(node) = node - 1)
class HipAnnotation {
  public:
    HipAnnotation(uint64_t n_rows, const std::vector<uint64_t> &col_begin, const std::vector<uint64_t> &rows, int device = 0) {
        if (col_begin.empty()) throw std::runtime_error("HipAnnotation: col_begin needs n_labels + 1 entries");
        if (int rc = mgx_annotation_create_sparse(n_rows, (uint32_t)(col_begin.size() - 1), col_begin.data(), rows.data(), 0, device, &a_))
            throw std::runtime_error(std::string("mgx_annotation_create_sparse: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    // `.column.annodbg` files decoded by kernels (mgx_annotation_load_columns_device); label_names: the labels in column order
    HipAnnotation(const std::vector<const char *> &paths, int device, uint64_t *n_rows, std::vector<std::string> *label_names) {
        mgx_column_file *names = nullptr;
        if (mgx_annotation_load_columns_device(paths.data(), (uint32_t)paths.size(), device, &a_, &names) != MGX_OK) throw std::runtime_error(mgx_last_error());
        *n_rows = mgx_column_file_num_rows(names);
        for (uint32_t j = 0, nl = mgx_column_file_num_labels(names); j < nl; ++j) label_names->emplace_back(mgx_column_file_label(names, j));
        mgx_column_file_free(names);
    }
    ~HipAnnotation() { mgx_annotation_destroy(a_); }
    HipAnnotation(const HipAnnotation &) = delete;
    uint32_t num_labels() const { return mgx_annotation_num_labels(a_); }
    mgx_annotation *handle() const { return a_; }
  private:
    mgx_annotation *a_ = nullptr;
};

// FASTA / FASTQ text to read batches on the device (mgx_read_parser: csrc/reads_parse.hpp).  parse() returns the handle's view:
// seqs / offsets in device memory, names / name_offsets / host_offsets on the host; valid until the next parse.  A file outside
// the grammar throws ParseRefused with the message of the C-ABI (it names the byte position).
struct ParseRefused : std::runtime_error { using std::runtime_error::runtime_error; };
class HipReadParser {
  public:
    explicit HipReadParser(int device = 0) {
        if (int rc = mgx_read_parser_create(device, &p_))
            throw std::runtime_error(std::string("mgx_read_parser_create: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    ~HipReadParser() { mgx_read_parser_destroy(p_); }
    HipReadParser(const HipReadParser &) = delete;
    HipReadParser &operator=(const HipReadParser &) = delete;
    // flags: 0, or the format of the file's first chunk for the later ones (mgx_reads::format)
    mgx_reads parse(const char *text, uint64_t n_bytes, bool final_chunk, uint32_t flags = 0, bool text_on_device = false) {
        mgx_reads r{};
        if (int rc = mgx_parse_reads(p_, text, n_bytes, text_on_device ? 1 : 0, final_chunk ? 1 : 0, flags, &r)) {
            if (rc == MGX_ERR_INVALID) throw ParseRefused(mgx_last_error());
            throw std::runtime_error(std::string("mgx_parse_reads: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
        }
        return r;
    }
    // device pointers of records first .. first + n, offsets from 0; valid until the next slice or parse
    void slice(uint64_t first, uint64_t n, const char **seqs, const uint64_t **offsets) {
        if (int rc = mgx_read_parser_slice(p_, first, n, seqs, offsets))
            throw std::runtime_error(std::string("mgx_read_parser_slice: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    mgx_read_parser *handle() const { return p_; }

  private:
    mgx_read_parser *p_ = nullptr;
};

class HipDBGAligner : public IDBGAligner {
  public:
    // throws std::runtime_error like the reference when check_config_scores() fails (dbg_aligner.cpp:55-56)
    HipDBGAligner(const HipBOSSGraph &graph, const DBGAlignerConfig &config, const mgx_limits *limits = nullptr)
          : graph_(graph) {
        if (int rc = mgx_aligner_create(graph.handle(), &config, limits, &a_))
            throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
        mgx_aligner_get_config(a_, &config_);
        own_stream();
    }
    // LabeledAligner<>(graph, config, annotator): every alignment of the results carries its label_columns
    HipDBGAligner(const HipBOSSGraph &graph, const DBGAlignerConfig &config, const HipAnnotation &annotation,
                  const mgx_limits *limits = nullptr)
          : graph_(graph), annotation_(&annotation) {
        if (int rc = mgx_labeled_aligner_create(graph.handle(), &config, limits, annotation.handle(), &a_))
            throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
        mgx_aligner_get_config(a_, &config_);
        own_stream();
    }
    // `workers` aligners are at work on this device at the same time (cli/align.cpp's thread pool): each sizes its arenas for its share
    void set_device_share(unsigned workers) {
        const std::string opt = "device_share=" + std::to_string(workers ? workers : 1);
        mgx_aligner_set_pipeline(a_, opt.c_str());
    }
    // a result-preserving kernel-selection switch of the library ("key=value", mgx_aligner_set_pipeline): A/B runs
    void set_kernel_option(const std::string &opt) {
        if (int rc = mgx_aligner_set_pipeline(a_, opt.c_str()))
            throw std::runtime_error(std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")");
    }
    ~HipDBGAligner() override { mgx_aligner_destroy(a_); }
    const HipBOSSGraph &get_graph() const override { return graph_; }
    const DBGAlignerConfig &get_config() const override { return config_; }
    bool has_coordinates() const override { return false; }

    void align_batch(const std::vector<Query> &seq_batch, const AlignmentCallback &callback) const override {
        // One call: mgx_align_batch itself re-aligns queries whose per-read device arenas overflowed (MGX_ERR_CAPACITY: the
        // reference has no such limit, its tables grow on the heap) with doubled limits, up to six doublings.  A status that is
        // left after that is an error of this call, as nothing in the reference's interface could carry it.
        std::string blob;
        std::vector<uint64_t> offsets(seq_batch.size() + 1, 0);
        for (size_t t = 0; t < seq_batch.size(); ++t) {
            blob += seq_batch[t].second;
            offsets[t + 1] = blob.size();
        }
        mgx_results res{};
        if (int rc = mgx_align_batch(a_, blob.data(), offsets.data(), seq_batch.size(), 0, &res))
            throw std::runtime_error(std::string("mgx_align_batch: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
        deliver(res, seq_batch, callback);
    }

    // The two halves for a host that gathers the results of several devices over RCCL (mgx_gather_*, mgx_align --rccl-gather):
    // the kernels of a batch with the results left in HBM — mgx_gather_start(g, handle()) takes them from there — and, on the
    // root, the decoded records of any rank (mgx_results_from_raw) handed to the callback like align_batch does.
    void align_batch_device(const std::vector<Query> &seq_batch) const {
        std::string blob;
        std::vector<uint64_t> offsets(seq_batch.size() + 1, 0);
        for (size_t t = 0; t < seq_batch.size(); ++t) {
            blob += seq_batch[t].second;
            offsets[t + 1] = blob.size();
        }
        if (blob.empty()) blob.push_back('\0');                      // (an empty batch still needs a pointer)
        if (int rc = mgx_align_batch_device(a_, blob.data(), offsets.data(), seq_batch.size(), 0))
            throw std::runtime_error(std::string("mgx_align_batch_device: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    // The TSV text of the batch align_batch_device ran last, written on the device (mgx_format_tsv_batch): what format_alignment
    // gives for every query, in query order.  label_names: as for format_alignment (null: labels print as numbers).  The view
    // is the handle's and stays valid until its next batch.  Throws for post_chain_alignments (the chained alignments exist
    // on the host only: align_batch with a callback remains the path) and for capacity statuses no retry cures.
    std::string_view format_batch_tsv(const std::vector<Query> &seq_batch, const std::vector<std::string> *label_names = nullptr) const {
        std::string headers;
        const std::vector<uint64_t> offsets = pack_headers(seq_batch, 0, seq_batch.size(), headers);
        return format_tsv(headers.data(), offsets.data(), seq_batch.size(), label_names);
    }
    // The results of the batch align_batch_device ran last in the mgx_results layout, decoded on the device and left there
    // (mgx_decode_results_device): every pointer of the view is DEVICE memory of the handle, valid until its next batch, fetch,
    // decode or format call; *sizes (optional) receives the arrays' element counts.  Pre-retry (a capacity-status query has
    // its status and no alignments) and, with post_chain_alignments, unchained.
    mgx_results decode_batch_device(mgx_results_sizes *sizes = nullptr) const {
        mgx_results res{};
        mgx_results_sizes s{};
        if (int rc = mgx_decode_results_device(a_, &res, &s))
            throw std::runtime_error(std::string("mgx_decode_results_device: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
        if (sizes) *sizes = s;
        return res;
    }
    // ... over reads that are in device memory already (HipReadParser::slice): n reads, offsets from 0
    void align_batch_device(const char *d_seqs, const uint64_t *d_offsets, uint64_t n) const {
        if (int rc = mgx_align_batch_device(a_, d_seqs, d_offsets, n, 1))
            throw std::runtime_error(std::string("mgx_align_batch_device: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
    }
    // ... with the names as flat arrays (mgx_reads::names / name_offsets; `name_offsets` points at the batch's first record: n + 1 entries)
    std::string_view format_batch_tsv(const char *names, const uint64_t *name_offsets, uint64_t n, const std::vector<std::string> *label_names = nullptr) const {
        return format_tsv(names + name_offsets[0], detail::rebased(name_offsets, n).data(), n, label_names);
    }
    // The `align --json` lines of queries first .. first + n of the batch align_batch_device ran last, written on the device
    // (mgx_format_json_batch): what mgx_format_json gives for those queries, in query order.  JSON text is large (about 60 bytes
    // per path node), so a caller formats a batch in slices: the slices' texts concatenated are the batch's.  The view is the
    // handle's and stays valid until its next batch or format call.  Throws for post_chain_alignments (the reference has no JSON
    // for chains) and for capacity statuses no retry cures.
    std::string_view format_batch_json(const std::vector<Query> &seq_batch, uint64_t first, uint64_t n) const {
        if (first > seq_batch.size() || n > seq_batch.size() - first) throw std::runtime_error("format_batch_json: the range is beyond the batch");
        std::string headers;
        const std::vector<uint64_t> offsets = pack_headers(seq_batch, first, n, headers);
        return format_json_range(headers.data(), offsets.data(), first, n);
    }
    // ... with the names as flat arrays (mgx_reads::names / name_offsets; `name_offsets` points at the BATCH's first record)
    std::string_view format_batch_json(const char *names, const uint64_t *name_offsets, uint64_t first, uint64_t n) const {
        return format_json_range(names, name_offsets + first, first, n);
    }
    mgx_aligner *handle() const { return a_; }
    static void deliver(const mgx_results &res, const std::vector<Query> &seq_batch, const AlignmentCallback &callback) {
        std::vector<AlignmentResults> results;
        results.reserve(seq_batch.size());
        for (const auto &q : seq_batch) results.emplace_back(q.second);
        for (size_t t = 0; t < seq_batch.size(); ++t) {
            if (res.status[t] != MGX_OK)
                throw std::runtime_error("query " + std::to_string(t) + " (" + seq_batch[t].first + "): status "
                                         + std::to_string(res.status[t]) + " (after the capacity retry, where the call has one)");
            AlignmentResults &paths = results[t];
            for (uint64_t ai = res.aln_begin[t]; ai < res.aln_begin[t + 1]; ++ai) {
                const mgx_alignment &m = res.alignments[ai];
                Alignment a;
                a.orientation_ = m.orientation;
                a.offset_ = m.offset;
                a.score_ = m.score;
                a.sequence_.assign(res.seqs + m.seq_begin, m.seq_len);
                a.nodes_.assign(res.nodes + m.nodes_begin, res.nodes + m.nodes_begin + m.n_nodes);
                for (uint32_t x = 0; x < m.n_cigar; ++x)
                    a.cigar_.data().emplace_back(res.cigar[m.cigar_begin + x].op, res.cigar[m.cigar_begin + x].len);
                const std::string &q = paths.get_query(m.orientation);
                a.query_view_ = std::string_view(q).substr(m.clipping, q.size() - m.clipping - m.end_clipping);
                if (res.labels && m.n_labels)
                    a.label_columns_.assign(res.labels + m.labels_begin, res.labels + m.labels_begin + m.n_labels);
                paths.alignments_.push_back(std::move(a));
            }
        }
        for (size_t i = 0; i < seq_batch.size(); ++i) callback(seq_batch[i].first, std::move(results[i]));
    }

  private:
    // the reference builds one aligner per thread-pool task (cli/align.cpp:440-475): every handle works on a stream of its own, so
    // that the tasks of one device overlap instead of taking turns on the default stream (batches arrive from host memory: nothing
    // of the caller's is ordered against it)
    std::string_view format_json_range(const char *headers, const uint64_t *header_offsets, uint64_t first, uint64_t n) const {
        mgx_text text{};
        const int rc = mgx_format_json_batch(a_, headers, header_offsets, first, n, &text);
        return detail::text_view(rc, text, "mgx_format_json_batch");
    }
    std::string_view format_tsv(const char *headers, const uint64_t *header_offsets, uint64_t n, const std::vector<std::string> *label_names) const {
        std::vector<const char *> names;
        if (label_names) for (const std::string &nm : *label_names) names.push_back(nm.c_str());
        mgx_text text{};
        const int rc = mgx_format_tsv_batch(a_, headers, header_offsets, names.empty() ? nullptr : names.data(), (uint32_t)names.size(), &text);
        return detail::text_view(rc, text, "mgx_format_tsv_batch", n);
    }
    // the headers of seq_batch[first .. first + n) end to end in `blob` -> their n + 1 offsets
    static std::vector<uint64_t> pack_headers(const std::vector<Query> &seq_batch, uint64_t first, uint64_t n, std::string &blob) {
        std::vector<uint64_t> offsets(n + 1, 0);
        for (uint64_t t = 0; t < n; ++t) {
            blob += seq_batch[first + t].first;
            offsets[t + 1] = blob.size();
        }
        if (blob.empty()) blob.push_back('\0');                     // (a range of empty headers still needs a pointer)
        return offsets;
    }
    void own_stream() {
        if (getenv("MGX_ADAPTER_DEFAULT_STREAM")) return;          // (A/B switch: every handle on the legacy default stream, as before round 6)
        if (int rc = mgx_aligner_create_stream(a_)) {
            const std::string msg = std::string(mgx_last_error()) + " (" + std::to_string(rc) + ")";
            mgx_aligner_destroy(a_);
            a_ = nullptr;
            throw std::runtime_error(msg);
        }
    }
    const HipBOSSGraph &graph_;
    const HipAnnotation *annotation_ = nullptr;
    DBGAlignerConfig config_;
    mgx_aligner *a_ = nullptr;
};

// format_alignment (cli/align.cpp:254-285), TSV branch; label_names: LabelEncoder::decode for label-aware results (:274-281)
inline std::string format_alignment(const std::string &header, const AlignmentResults &paths, int32_t min_path_score,
                                    const std::vector<std::string> *label_names = nullptr) {
    std::string s = header + "\t" + paths.get_query();
    if (paths.empty()) {
        s += "\t*\t*\t" + std::to_string(min_path_score) + "\t*\t*\t*\n";
    } else {
        for (const auto &p : paths) {
            s += "\t" + p.to_tsv_fields();
            if (p.get_label_columns().size()) {
                s += "\t";
                bool first = true;
                for (uint64_t c : p.get_label_columns()) {
                    if (!first) s += ";";
                    first = false;
                    s += (label_names && c < label_names->size()) ? (*label_names)[c] : std::to_string(c);
                }
            }
        }
        s += "\n";
    }
    return s;
}

} // namespace host
} // namespace mgx
