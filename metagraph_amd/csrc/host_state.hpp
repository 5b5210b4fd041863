// host_state.hpp — what the host units of libmgx.so share (mgx.hip, mgx_graph.hip, mgx_map.hip, mgx_results.hip, mgx_text.hip):
// the error message, the device block pool, the two handle types, the cursor words, the environment switches, and the entry
// points that one host unit calls in another.  Declarations and small inlines only; host code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mgx.h"
#include "host_common.hpp"

#define MGX_INTERNAL __attribute__((visibility("hidden")))      // shared by the units of the library, not exported from it

// mgx.hip: sets the thread-local message behind mgx_last_error() and returns `code`
MGX_INTERNAL int fail(int code, const char *fmt, ...);
MGX_INTERNAL int hip_fail(hipError_t e, const char *expr, const char *file, int line);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return hip_fail(e_, #expr, __FILE__, __LINE__);                      \
    } while (0)

// Device blocks of destroyed aligners, kept for the next aligner on the same device.  The reference builds one aligner per
// thread-pool task (cli/align.cpp:440-475); with hipMalloc / hipFree per handle every task paid for fresh multi-GB arenas
// (first-touch of a new 20 - 40 GB block: seconds, `profiles/r06_workers_one_device.txt`) and every hipFree synchronised the
// whole device under the other workers.  A block returns here when its aligner is destroyed (its stream has been
// synchronised by then) and is handed out best-fit; the pool is emptied when an allocation fails and by mgx_device_trim().
struct DevPool {
    enum { MAX_DEV = 16 };
    std::mutex mu;
    std::multimap<size_t, void *> blocks[MAX_DEV];
    size_t held[MAX_DEV] = { 0 };
    static int dev() { int d = 0; (void)hipGetDevice(&d); return d >= 0 && d < MAX_DEV ? d : -1; }
    void *take(size_t want, size_t *got) {
        const int d = dev();
        if (d < 0) return nullptr;
        std::lock_guard<std::mutex> lock(mu);
        auto it = blocks[d].lower_bound(want);
        if (it == blocks[d].end() || it->first > want + want / 2 + (1u << 20)) return nullptr;       // (a much larger block stays for who needs it)
        void *p = it->second;
        *got = it->first;
        held[d] -= it->first;
        blocks[d].erase(it);
        return p;
    }
    void give(void *p, size_t bytes) {
        const int d = dev();
        if (d < 0) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> lock(mu);
        blocks[d].emplace(bytes, p);
        held[d] += bytes;
    }
    size_t held_bytes() {
        const int d = dev();
        if (d < 0) return 0;
        std::lock_guard<std::mutex> lock(mu);
        return held[d];
    }
    void flush() {
        const int d = dev();
        if (d < 0) return;
        std::lock_guard<std::mutex> lock(mu);
        for (auto &e : blocks[d]) (void)hipFree(e.second);
        blocks[d].clear();
        held[d] = 0;
    }
};
MGX_INTERNAL extern DevPool g_pool;       // mgx.hip

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pooled = false;              // an aligner's buffer: comes from / returns to g_pool (the graph's own tables do not)
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        if (pooled) g_pool.give(p, bytes); else (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
    // headroom: 1/8 on top for buffers that grow with the batch; none for the arena, which is sized from the free memory.
    // (A block from the pool holds whatever its last owner left: like a fresh hipMalloc block, its contents are undefined —
    // every owner initialises what it reads, keyed on `bytes` having changed.)
    int ensure(size_t n, bool exact = false) {
        if (n <= bytes) return MGX_OK;
        release();
        size_t want = exact ? n : n + n / 8 + 256;
        if (pooled) {
            size_t got = 0;
            if (void *q = g_pool.take(want, &got)) { p = q; bytes = got; return MGX_OK; }
        }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && g_pool.held_bytes()) {      // what the pool holds is free memory: give it back and try again
            (void)hipGetLastError();
            g_pool.flush();
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) { p = nullptr; return fail(MGX_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        bytes = want;
        return MGX_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct mgx_graph {
    int device = 0;
    mgx::DevGraph g;
    DevBuf blocks, last_hint, w_hint[4], sel_anchor, firstc, terminus, valid, prefix_tbl;
    uint64_t bytes = 0;
    uint32_t mode = MGX_MODE_BASIC;
    bool primary_tables = false;      // PRIMARY: reverse-complement tables built (default; MGX_PRIMARY_TABLES=0 turns them off)
    // What label-aware aligners derive from the whole graph, computed once per graph (and annotation) instead of once per
    // aligner — the host adapters build one aligner per batch and worker thread; mgx_graph.hip, graph_*() below:
    mutable std::mutex label_mu;
    mutable DevBuf canon_repr;        // CANONICAL-mode graphs: node -> the representative of its k-mer (k_canon_repr, 4 B per node)
    mutable bool canon_repr_ready = false;
    mutable std::map<uint64_t, bool> dummy_clean;   // per annotation, by its process-unique id (mgx_annotation_uid: never reused, unlike the handle's address)
};

// Environment variables: every read of the environment in the host units goes through this block.
// (a) Measurement probes — occupancy scans, LDS caps, prints, ablations that give WRONG results — are read in -DMGX_PROBES builds
// (tools/build_variant.py TAG host -DMGX_PROBES) only; the product library ignores them: MGX_MAP_BYTES, MGX_DEBUG_SLOTS, MGX_ABLATE,
// MGX_EXT_GROUPS_PCT, MGX_EXT_LDS_CAP, MGX_SEED_LDS_CAP, MGX_SEED_LDS_PRINT, MGX_SEED_WAVES_PCT, MGX_HOST_TIMERS.
#ifdef MGX_PROBES
static inline bool probe_env_set(const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; }
static inline uint32_t probe_env_u32(const char *name, uint32_t dflt) { const char *e = getenv(name); return e ? (uint32_t)atoi(e) : dflt; }
static inline uint32_t probe_env_pct(const char *name) { const char *e = getenv(name); return e ? (uint32_t)std::min(100, std::max(1, atoi(e))) : 100u; }
#else
static inline bool probe_env_set(const char *) { return false; }
static inline uint32_t probe_env_u32(const char *, uint32_t dflt) { return dflt; }
static inline uint32_t probe_env_pct(const char *) { return 100u; }
#endif
// (b) Read by the product library too (the tools/pmc_*.sh flows and the variant builds run against it); none changes a result:
//   MGX_PREFIX_LEN_MAX=m    graph load: the suffix-range table covers at most m characters (2 .. 15)
//   MGX_PRIMARY_TABLES=0    graph load: no reverse-complement tables for a PRIMARY graph
//   MGX_LANE_HASH_MULT=f    k_lane: f times the node-table slots per lane
//   MGX_LANE_BLOCKS_PCT=p   k_lane: p % of the resident wavefronts (is the kernel bound by the latency of its own dependent
//                           accesses, or by what the memory system serves per second?)
//   MGX_LANE_TIMERS / MGX_SL_TIMERS   print the section timers of a -DMGX_LANE_TIMERS / -DMGX_SL_TIMERS build of the lane kernels
static inline bool env_int(const char *name, int *v) {
    const char *e = getenv(name);
    if (e) *v = atoi(e);
    return e != nullptr;
}

// MGX_HOST_TIMERS=1: host-side wall time per stage of a batch on stderr (where does a one-read batch spend its 2 ms?)
struct HostStageTimer {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    static bool on() { static const bool v = probe_env_set("MGX_HOST_TIMERS"); return v; }
    explicit HostStageTimer(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostStageTimer() {
        if (on()) fprintf(stderr, "mgx host stage %-14s %8.1f us\n", name,
                          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// The words of mgx_aligner::cursors (16 x 8 B): what the kernels count, through the pointers the host hands them.
enum CursorSlot {
    CUR_OUT = 0,              // output-stream words handed out (keeps counting past the capacity: mgx_align_batch_device)
    CUR_READ = 1,             // next work item of a persistent kernel: rewound before every launch that takes items from it
    CUR_SEED = 2,             // seeds in the seed stream (keeps counting past the capacity)
    CUR_LMAX = CUR_SEED,      // ... and, while a batch is staged, the length of its longest read (k_kmer_counts)
    CUR_RETRY = 3,            // multi-pass extension: reads listed for the next pass (CUR_OUT .. CUR_RETRY: cleared when run_align starts)
    CUR_MAP = 4,              // next chain of the mapping kernels
    CUR_LANE_BAIL = 5,        // k_lane: reads passed on to the extension kernel ...
    CUR_LANE_DONE = 6,        // ... and reads finished (the host reads the two with one copy)
    CUR_SL_BAIL = 8,          // lane-per-read seeder, first pass: reads left, listed from the front ...
    CUR_SL_DONE = 9,          // (both passes: reads seeded)
    CUR_SL_BAIL2 = 10,        // second pass: reads left for the wave-per-read seeding kernel
    CUR_SL_BAIL_BACK = 11,    // ... first pass: reads left, listed from the back
    CUR_WORDS = 16
};

// mgx_aligner::ev: the stream positions mgx_stats' times are measured between (collect_stats)
enum AlignEvent {
    EV_MAP_BEGIN, EV_MAP_END,         // run_map
    EV_ALIGN_BEGIN, EV_ALIGN_END,     // run_align, from the first seeding launch
    EV_SEEDED,                        // both seeders are through
    EV_SORTED,                        // the work sort is through: the extension starts
    EV_LANE_END,                      // the lane-per-read kernel is through (= the extension's start when it does not run)
    EV_SEED_LANE_END,                 // the lane-per-read seeder is through
    EV_COUNT
};

// What a seed-chainer handle (mgx_seed_chainer_create, mgx_chaintab.hip) keeps between calls: the scratch of the chain stage, the
// tables of its last batch in device memory, and their host copies (mgx_chain_tables_batch without MGX_CHAIN_TABLES_ON_DEVICE,
// mgx_chain_tables_fetch).  Counts and their exclusive sums: CT_ARRAYS arrays of 2 n + 1 words each.
struct ChainTabState {
    enum { CT_PAIRS = 0, CT_SEEDS, CT_NODES, CT_ANCHORS, CT_ARRAYS };
    DevBuf counts, begins;                                   // per list: (seed, label) pairs seen, kept seeds, their nodes, anchors
    DevBuf pair_key, pair_key_alt, pair_val, pair_val_alt;   // (label, first covered position) -> end of the covered range, per pair
    DevBuf kept, n_kept;                                     // per list: the labels at or above the cut-off, ascending
    DevBuf seeds, nodes, num_matching, status, qsize, penalty;
    DevBuf anchors, anchors_alt, backtrace, perm, perm_alt, k32, k32_alt, k64, k64_alt, sort_tmp, sort_tmp_anchors;     // (one scratch per sort: what a call allocates does not depend on which sort wants more)
    std::vector<int32_t> h_penalty;
    uint64_t n = 0, n_seeds = 0, n_nodes = 0, n_anchors = 0;
    bool have = false;                                       // the device arrays hold a batch
    std::vector<uint64_t> h_seed_begin, h_nodes, h_num_matching, h_list_begin;
    std::vector<mgx_chain_seed> h_seeds;
    std::vector<mgx_chain_anchor> h_anchors;
    std::vector<uint32_t> h_backtrace;
    std::vector<int32_t> h_status;
};

struct mgx_aligner {
    const mgx_graph *graph = nullptr;
    const mgx_annotation *anno = nullptr;      // label-aware alignment (mgx_labeled_aligner_create)
    bool anno_dummy_clean = false;             // no row of a dummy node holds a label (k_anno_dummy_rows)
    bool chainer = false;                      // mgx_seed_chainer_create: the handle answers mgx_chain_tables_batch / _fetch only
    ChainTabState ct;
    mgx_config cfg;
    mgx::DevConfig dcfg;
    mgx_limits user_lim;
    bool have_user_lim = false;
    DevBuf mlen_fwd, mlen_rc;     // k_map's index() match lengths, one byte per k-mer position
    DevBuf pk_fwd, pk_rc, iv_fwd, iv_rc;      // 2-bit packed reads + invalid flags of the mapping kernel (k <= 32)
    DevBuf rng_fwd, rng_rc;       // and the (rl, ru) of matches >= min_seed_length (8 B per position; optional)
    bool have_rng = false;
    DevBuf score_matrix, seqs, offsets, counts, node_begin, nodes_fwd, nodes_rc, arena, results, stream, cursors, d_stats, d_stats_map, scan_tmp, dbg_seeds;
    DevBuf seed_hdr, seed_stream, work_key, work_key_sorted, order_in, order, sort_tmp, retry_list;    // seeds from the seeding to the extension kernels, the work sort
    DevBuf resume_pool[2], retry_list2, retry_key[2];      // multi-pass extension: resume records, retry lists and keys (ping-pong)
    DevBuf lane_scratch, lane_params, lane_bail, lane_hist;           // lane-per-read kernel: per-lane scratch, its parameter block, the reads it passes on
    bool packed_valid = false;    // pk_* / iv_* hold this batch's strands (k <= 32 and the batch was mapped)
    uint32_t lane_epoch = 0;
    uint64_t lane_done = 0;
    uint64_t lane_exact = 0;      // ... of them through the exact exit (k_lane_exact) with a first seed that spans the query
    uint64_t lane_exact_path = 0; // ... and through its path class (level 2: every k-mer a node, the first seed shorter)
    uint64_t lane_exact_sub = 0;  // ... and through its substitution class (level 3: one run of zeros, walked; counted in neither of the two above)
    unsigned long long lane_hist_h[32] = { 0 };
    DevBuf seedlane_scratch, seedlane_params, seedlane_bail, seedlane_hist;   // lane-per-read seeder: seed buffers, parameter block, the reads it leaves, why
    uint64_t seedlane_launched = 0;    // the last batch ran it (its counters are read back by collect_stats)
    uint32_t n_passes = 0;
    mgx::DevLimits lim;
    uint64_t n_reads = 0, total_kmers = 0;
    uint32_t n_slots = 0;
    bool keep_seeds = false;
    // host copies
    std::vector<mgx::ReadResult> h_results;
    std::vector<uint32_t> h_stream;
    mgx::HostResults host;
    mgx::HostResults host_chained;     // post_chain_alignments: `host` after chain_host.hpp
    mgx::HostResults host_retried;     // mgx_align_batch: the results with the re-aligned capacity queries in place
    bool retry_capacity = true;        // (mgx_aligner_set_pipeline "retry_capacity=0": statuses are handed to the caller)
    uint32_t label_scale = 1;          // the label arenas' multiplier (derive_limits; doubled per attempt of the capacity retry)
    const char *last_d_seqs = nullptr;           // the batch mgx_align_batch_device ran last (device pointers)
    const uint64_t *last_d_offsets = nullptr;
    // Every launch, asynchronous copy and hipcub call of this aligner goes to this stream, and its blocking copies synchronise
    // this stream only (copy_sync).  0 = the legacy default stream (what rounds 1-5 used throughout): ordered with everything
    // else the process does on blocking streams.  mgx_aligner_set_stream() gives a handle its own stream, so that the handles
    // of several worker threads on one device (cli/align.cpp:440-475: one aligner per thread-pool task) overlap instead of
    // serialising on the default stream.
    hipStream_t hstream = nullptr;
    int device = 0;                    // the graph's device
    bool own_stream = false;           // mgx_aligner_create_stream: destroyed with the aligner
    uint64_t stage_generation = 0;               // counts stage_batch calls (mgx_map_batch re-stages the same buffers) ...
    uint64_t aligned_generation = 0;             // ... and which of them mgx_align_batch_device aligned: post-chaining and the
                                                 // capacity retry read the batch back only while it is still the staged one
    std::vector<uint64_t> m_node_begin, m_fwd, m_rc;
    DevBuf ms_counts, ms_nodes, ms_sorted;       // mgx_map_summary_batch: the 12-byte records, the merged node array, the long form's scratch
    std::vector<mgx_map_counts> h_ms_counts;
    std::vector<uint64_t> h_ms_nodes;
    // the batch mgx_map_summary_batch ran last, for mgx_format_map_batch: the stage_batch call it was (0: none, or the call failed —
    // every other batch call stages again and so ends it), its reads (device pointers), map_length, longest read, and whether
    // ms_nodes holds its node array
    uint64_t ms_generation = 0;
    const char *ms_d_seqs = nullptr;
    const uint64_t *ms_d_offsets = nullptr;
    uint32_t ms_map_length = 0, ms_lmax = 0;
    bool ms_have_nodes = false;
    DevBuf mf_threshold;                         // mgx_format_map_batch: the presence threshold per k-mer count
    std::vector<uint64_t> h_mf_threshold;        // ... its host copy (the handle's: an asynchronous upload may outlive the call that failed)
    // mgx_format_tsv_batch: headers, their offsets, label names (bytes, then the n + 1 begins), line lengths, line_begin (n + 1, then
    // the capacity counter), the text, the capacity list, the host-formatted lines' (query, length) pairs
    DevBuf tf_headers, tf_header_offsets, tf_names, tf_len, tf_begin, tf_text, tf_cap, tf_patch;
    char *h_text = nullptr;                      // the text on the host: pinned memory, grown as needed
    size_t h_text_bytes = 0;
    std::vector<uint64_t> h_line_begin;
    // decode_on_device (mgx_decode_results_device, the option decode_on_device): the five count arrays and their exclusive sums
    // (RD_ARRAYS x (n + 1) words each; the first of the sums is aln_begin), the five totals, and the other six output arrays
    DevBuf rd_counts, rd_begins, rd_totals, rd_alns, rd_nodes, rd_cigar, rd_seqs, rd_status, rd_labels;
    enum { RD_H_ALN_BEGIN = 0, RD_H_ALNS, RD_H_NODES, RD_H_CIGAR, RD_H_SEQS, RD_H_STATUS, RD_H_LABELS, RD_H_N };
    void *h_rd[RD_H_N] = {};                     // the seven arrays on the host: pinned memory, grown as needed (like h_text)
    size_t h_rd_bytes[RD_H_N] = {};
    bool aligned_empty = false;                  // the last mgx_align_batch_device call had no query (it stages nothing)
    mgx_stats hstats;
    hipEvent_t ev[EV_COUNT] = {};
    uint64_t kernels_ran = 0;     // MGX_KERNEL_* bits of the extension kernels the last batch launched
    uint64_t seed_scale = 1, seed_cap = 0;
    uint64_t arena_stride = 0;
    uint64_t out_words = 0;       // capacity of `stream` for the current batch shape
    uint64_t out_min_words = 0;   // raised when a batch overflowed the heuristic size
    bool no_fast = false;         // test hook: extension through the general path only
    // Result-preserving kernel-selection switches (mgx_aligner_set_pipeline "key=value"; INTEGRATION.md "run-time switches").
    // Every combination gives the same alignments; the parity suite runs the kernels the automatic choice would not pick for
    // its small batches through them.  -1 = automatic.
    struct Options {
        int ext64 = 1;            // 0: never the 64-lane one-read-per-wavefront kernel (small batches run the 8-lane groups)
        int groups_per_wave = -1; // 0 = all 8 groups of a wavefront take reads, 1 .. 8 = that many
        int multi_pass = -1;      // multi-pass extension on / off
        int resume_cap = -1;      // ... resume records a pass may write at most (-1: as many as reads, memory permitting); a read
                                  // that finds no room goes on without a seed limit in the same launch
        int no_compact = 0, no_alias = 0, no_bt_runs = 0, no_flat = 0;
        int lane = -1;            // the lane-per-read kernel in front of the extension kernel: -1 auto, 0 off, 1 forced
        int exact = -1;           // the lane kernel's exact exit (k_lane_exact, no DP): -1 auto (level 3 for the batches the lane kernel
                                  // takes of its own accord), 0 off, 1 / 2 / 3 that level wherever the lane kernel runs (1: reads whose
                                  // first seed spans the query; 2: also reads whose every k-mer is a node, the path class; 3: also
                                  // reads with one substitution, the substitution class);
                                  // label-aware batches included (the reads that keep one label all along)
        int seed_lane = -1;       // the lane-per-read seeder in front of the seeding kernel (seed_lane.hpp): -1 auto, 0 off, 1 forced
        int seed_wps = 8;         // wavefronts per SIMD of the short-read seeding kernel: 8 (64 VGPRs, spills) or 4 (102 VGPRs, tables in LDS)
        int device_share = 1;     // handles expected to run on this device at the same time (worker threads, -p N): the per-slot
                                  // arenas of this handle are sized for 1 / device_share of the machine instead of all of it
        int decode_on_device = 0; // mgx_fetch_results: the mgx_results arrays written by kernels (mgx_results.hip) instead of HostResults::decode
        int map_pipe = 1;         // k_map as the request / response machine (map_pipe.hpp): 1 = for batches of >= 65536 chains, 2 = always,
                                  // 0 = never (one chain step per lane and iteration: rounds 1-4)
    } opt;
};

static inline unsigned long long *cursor(const mgx_aligner *A, CursorSlot s) { return A->cursors.as<unsigned long long>() + s; }
// zero the slots first .. last
static inline hipError_t clear_cursors(mgx_aligner *A, CursorSlot first, CursorSlot last) {
    return hipMemsetAsync(cursor(A, first), 0, (size_t)(last - first + 1) * 8, A->hstream);
}
// a blocking copy that synchronises the aligner's stream only (hipMemcpy would synchronise the whole device's default stream)
static inline hipError_t copy_sync(mgx_aligner *A, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, A->hstream)) return e;
    return hipStreamSynchronize(A->hstream);
}

// ---- what one host unit calls in another ---------------------------------------------------------------------------------------
// mgx.hip
MGX_INTERNAL int aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *anno,
                                mgx_aligner **out);
MGX_INTERNAL int collect_stats(mgx_aligner *A, bool mapped, bool aligned);
// the seeding stage of run_align alone, for a staged and mapped batch: SeedHdr / DevSeed in A->seed_hdr / A->seed_stream (the
// events collect_stats reads behind the seeding are recorded at its end).  *seeds_wanted: what the seed stream was asked for;
// more than A->seed_cap: the caller raises A->seed_scale and runs the stage again, as mgx_align_batch_device does
MGX_INTERNAL int run_seeding(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax, uint64_t *seeds_wanted);
// every align / fetch / format entry point starts with this: a seed-chainer handle runs none of them
MGX_INTERNAL int refuse_chainer(const mgx_aligner *A, const char *call);
// out[0 .. n) = the exclusive sums of in[0 .. n) (device arrays) on the aligner's stream; the scratch is A->scan_tmp
MGX_INTERNAL int exclusive_sum(mgx_aligner *A, uint64_t *in, uint64_t *out, uint64_t n);
// The HIP runtime loads a unit's code object onto a device at the first use of one of its kernels.  mgx_graph_create brings those
// of the mapping kernels (load_map_kernels, mgx_map.hip), the plain seeding kernel (mgx_seed_load) and the work sort and scan
// (load_sort_kernels, mgx.hip) onto the graph's device — as when they were one code object with the index builders — so that
// the first batch, and the worker threads that run their first batches at once, do not load them.  No launch, nothing on a stream.
MGX_INTERNAL hipError_t load_sort_kernels();
MGX_INTERNAL hipError_t load_map_kernels();

// mgx_graph.hip: the two label tables an aligner derives from the whole graph, each computed once and kept under label_mu —
// does no row of a dummy node hold a label of `anno` (k_anno_dummy_rows); CANONICAL-mode graphs: g->canon_repr (k_canon_repr)
MGX_INTERNAL int graph_dummy_rows_clean(const mgx_graph *g, const mgx_annotation *anno, bool *clean);
MGX_INTERNAL int graph_canon_repr(const mgx_graph *g);

// mgx_map.hip: stage inputs, compute k-mer slot offsets and Lmax on the device (window: the characters per node slot — the
// graph's k, or mgx_map_summary_batch's map_length < k); map the staged batch (raw_edges: BOSS::map_to_edges, the node mask not
// applied — mgx_map_summary_batch on CANONICAL graphs applies it after the minimum)
MGX_INTERNAL int stage_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device,
                             const char **d_seqs, const uint64_t **d_offsets, uint32_t *Lmax_out, uint32_t window = 0);
MGX_INTERNAL int run_map(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, bool do_rc, bool mapped, uint32_t Lmax,
                         bool raw_edges = false);

// mgx_results.hip: the capacity-status queries `todo` (ascending) of the batch the device holds, aligned again with larger limits:
// fixed[t] = the results of todo[t] where have[t]; h_off = the batch's offsets, h_seq = its bytes from h_off[todo.front()] on
MGX_INTERNAL int realign_capacity_queries(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n,
                                          const std::vector<uint64_t> &todo, std::vector<mgx::HostResults> &fixed,
                                          std::vector<uint8_t> &have, std::vector<uint64_t> &h_off, std::vector<char> &h_seq);
