/*
 * mgx.h — C-ABI of the MI355X-native sequence-to-graph aligner (libmgx.so).
 *
 * This is the drop-in boundary for MetaGraph's `DBGAligner` hot path.  Every entry point
 * cites the reference interface it stands in for (paths are into ratschlab/metagraph,
 * `metagraph/src/...`).  Plain C types only: pointers + sizes, no C++/torch types.
 *
 * Ownership: inputs are caller-owned and only read during the call.  Results live in a
 * library-owned arena attached to the aligner handle and stay valid until the next
 * mgx_align_batch() on the same handle or mgx_aligner_destroy().
 * Threading: one in-flight batch per aligner handle; several handles may share one graph
 * (graph is immutable after creation), mirroring `DBGAligner` instances sharing a
 * `const DeBruijnGraph&` (graph/alignment/dbg_aligner.hpp:63-64).
 * Errors: every function returns MGX_OK (0) or a negative code; mgx_last_error() gives text.
 * There is NO CPU fallback: without a HIP device every compute entry point fails with
 * MGX_ERR_NO_DEVICE.
 */
#ifndef MGX_H_
#define MGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 6      /* still 6: symbols added only: mgx_column_coord_file_read / mgx_column_file_coord_begin / mgx_column_file_coords /
                                * mgx_annotation_set_coordinates_device / mgx_annotation_load_coord_columns_device / mgx_column_coord_file_decode_device
                                * (k-mer coordinates read from files, on the host and on the device); before that mgx_annotation_load_columns_device / mgx_column_file_decode_device / mgx_column_decode_kernel_launch_counts
                                * (`.column.annodbg` files decoded by kernels); before that mgx_stats::n_lane_exact_reads and (later) n_lane_exact_path_reads, n_lane_exact_sub_reads appended (mgx_aligner_stats fills sizeof(mgx_stats): rebuild callers with this
                                * header) and the option exact; before that, symbols added only: mgx_decode_results_device / mgx_decode_kernel_launch_counts / the option decode_on_device
                                * (the mgx_results layout of a batch, written by kernels); before that mgx_format_json_batch / mgx_format_json_kernel_launch_counts (the `align --json` text of a
                                * batch, written by kernels); before that mgx_format_map_batch / mgx_format_map_kernel_launch_counts / MGX_MAP_KEEP_NODES (the text of
                                * `align --map`, written by kernels); before that mgx_read_parser_* / mgx_parse_reads / mgx_parse_kernel_launch_counts (FASTA / FASTQ text to
                                * read batches on the device); before that mgx_format_tsv_batch / mgx_format_kernel_launch_counts (the TSV text of a batch, written
                                * by kernels); before that mgx_map_summary_batch / mgx_map_present / mgx_format_map / mgx_map_kernel_launch_counts
                                * (`align --map`: per-read k-mer counts, presence, --align-length < k);
                                * 6 (round 6, late): mgx_gather_* (RCCL gather of the device results); 5 (round 6): mgx_stats::n_seed_lane_reads / seed_lane_ms / seed_lane_left_reads, streams, coordinates,
                                * mgx_chain_seeds; 4 (round 5): mgx_stats::n_capacity_retried, mgx_chain_alignments, post_chain_alignments accepted;
                                * 3 (round 4): mgx_alignment::n_labels / labels_begin, mgx_results::labels (label-aware alignment),
                                * mgx_stats::extend_kernels / n_lane_reads / lane_ms, "key=value" options of mgx_aligner_set_pipeline;
                                * 2 (round 3): mgx_annotation_*; mgx_stats / mgx_config grew in round 2 without a bump (callers built
                                * against 1 must be rebuilt: mgx_aligner_stats writes the larger struct) */

enum {
    MGX_OK = 0,
    MGX_ERR_INVALID = -1,      /* bad argument / malformed BOSS view */
    MGX_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime failure */
    MGX_ERR_UNSUPPORTED = -3,  /* config outside the implemented path */
    MGX_ERR_CONFIG = -4,       /* check_config_scores() failed (aligner_config.cpp:39-66);
                                  the reference throws std::runtime_error (dbg_aligner.cpp:55-56) */
    MGX_ERR_CAPACITY = -5,     /* a per-read device arena overflowed; see mgx_limits */
    MGX_ERR_OOM = -6
};

/* Graph modes (graph/representation/base/sequence_graph.hpp:160). */
enum { MGX_MODE_BASIC = 0, MGX_MODE_CANONICAL = 1, MGX_MODE_PRIMARY = 2 };

/* CIGAR operators, numeric values identical to Cigar::Operator
 * (graph/alignment/aligner_cigar.hpp:18-25); printed with "SX=DIG" (:107). */
enum { MGX_OP_CLIPPED = 0, MGX_OP_MISMATCH = 1, MGX_OP_MATCH = 2,
       MGX_OP_DELETION = 3, MGX_OP_INSERTION = 4, MGX_OP_NODE_INSERTION = 5 };

/*
 * A read-only view of a BOSS table — what `boss::BOSS` holds after load
 * (graph/representation/succinct/boss.hpp:28-631; fields W_, last_, F_, k_).
 * Edge indices are 1..n_edges; slot 0 of W/last is the unused sentinel slot
 * (boss.cpp:74-83).  A DBG node IS a BOSS edge index (dbg_succinct.cpp:43-45).
 */
typedef struct mgx_boss_view {
    uint32_t k;              /* DBG k-mer length = BOSS node length + 1 (dbg_succinct.cpp:44) */
    uint32_t sigma;          /* alphabet size incl. '$'; must be 5 ("$ACGT", kmer/alphabets.hpp:64) */
    uint64_t n_edges;        /* W/last have n_edges+1 entries */
    const uint8_t *W;        /* one byte per edge, values 0..2*sigma-1 (boss.cpp:62) */
    const uint8_t *last;     /* one byte per edge, 0/1 */
    const uint64_t *F;       /* sigma entries (boss.hpp:506-510) */
    const uint8_t *valid;    /* optional node mask, one byte per edge (dbg_succinct.cpp:934-936);
                                NULL = every edge is a node, as after reset_mask() (cli/align.cpp:337-339) */
    uint32_t mode;           /* MGX_MODE_* = DeBruijnGraph::get_mode() of the DBGSuccinct.  CANONICAL (both strands stored): the
                              * aligner always seeds both strands, runs the backward pass on the same graph and reports
                              * reverse-strand alignments as the forward alignments they mirror (dbg_aligner.cpp:225,644-655).
                              * PRIMARY (one k-mer of every pair stored): aligned through the CanonicalDBG wrapper as the reference
                              * does (dbg_aligner.cpp:52-53, canonical_dbg.cpp): node ids above n_edges are reverse complements
                              * (id - n_edges is the stored node), mgx_graph_max_index reports 2 * n_edges.  PRIMARY needs
                              * k <= 64 and 2 * n_edges < 2^32 (MGX_ERR_UNSUPPORTED otherwise). */
    uint32_t on_device;      /* 0: W/last/valid are host pointers; 1: device pointers (F always host) */
} mgx_boss_view;

/* Field-for-field mirror of DBGAlignerConfig (graph/alignment/aligner_config.hpp:18-94): same members in the same order
 * (explicit padding where the C++ struct has implicit padding), so a reference-side adapter copies member-wise. */
typedef struct mgx_config {
    uint64_t num_alternative_paths;    /* :23 */
    uint64_t min_seed_length;          /* :24  (0 -> k, dbg_aligner.cpp:37-38) */
    uint64_t max_seed_length;          /* :25  (0 -> k, dbg_aligner.cpp:43-44) */
    uint64_t max_num_seeds_per_locus;  /* :26 */
    int32_t min_cell_score;            /* :34 */
    int32_t min_path_score;            /* :35 */
    int32_t xdrop;                     /* :36 */
    int32_t _pad0;
    double min_exact_match;            /* :38 */
    double max_nodes_per_seq_char;     /* :39 */
    double max_ram_per_alignment;      /* :40 */
    double rel_score_cutoff;           /* :41 */
    int8_t gap_opening_penalty;        /* :43 */
    int8_t gap_extension_penalty;      /* :44 */
    int8_t left_end_bonus;             /* :45 */
    int8_t right_end_bonus;            /* :46 */
    uint8_t forward_and_reverse_complement; /* :48 */
    uint8_t chain_alignments;          /* :49 (must be 0.  The reference never lets a caller set it either: it exits without coordinates,
                                        * dbg_aligner.cpp:546-550, and LabeledAligner switches it on itself for an annotation with
                                        * coordinates, aligner_labeled.cpp:457-462 — such annotations are refused at
                                        * mgx_labeled_aligner_create.  Of seed chaining, aligner_chainer.cpp:47-542, the device has
                                        * k-mer coordinates, mgx_annotation_set_coordinates, the chainer's DP on its own,
                                        * mgx_chain_seeds, and the whole chain stage of a read batch — seeds, their coordinate-aware
                                        * filter, the anchors, the chainer's tables —, mgx_chain_tables_batch on a handle of
                                        * mgx_seed_chainer_create; the extension between chained seeds is not built: DESIGN 3.9) */
    uint8_t post_chain_alignments;     /* :50: chain_alignments (aligner_chainer.cpp:555-720) over every query's alignments.  The
                                        * device then keeps EVERY alignment of a query (aligner_aggregator.hpp:88-96; at most
                                        * 4 x MGX_MAX_ALTERNATIVE_PATHS - 3 x num_alternative_paths = 13 with the default of
                                        * one alternative path — a query with more has status MGX_ERR_CAPACITY) and the
                                        * chaining runs on the host inside mgx_fetch_results / mgx_align_batch; results left
                                        * on the device (mgx_device_results) are the un-chained ones: decode them and call
                                        * mgx_chain_alignments.  Not with an annotation. */
    uint8_t global_xdrop;              /* :51; 0 = per-branch x-drop: label-aware aligners only (mgx_labeled_aligner_create), a plain
                                          aligner gives MGX_ERR_UNSUPPORTED as the reference's DBGAligner throws */
    uint8_t allow_left_trim;           /* :52 */
    uint8_t no_backtrack;              /* :53 (must be 0) */
    uint8_t seed_complexity_filter;    /* :54 */
    uint8_t alignment_edit_distance;          /* :56  read by mgx_config_set_scoring_matrix only, like the reference's */
    int8_t alignment_match_score;             /* :57  set_scoring_matrix(); the aligner itself reads score_matrix       */
    int8_t alignment_mm_transition_score;     /* :58  (a positive penalty, negated when the matrix is built)            */
    int8_t alignment_mm_transversion_score;   /* :59 */
    uint8_t _pad1[1];
    int8_t score_matrix[128][128];     /* :61 ScoreMatrix, [graph char][query char] */
} mgx_config;

/* Fill `c` with DBGAlignerConfig{} defaults (aligner_config.hpp:23-54); score matrix zeroed. */
void mgx_config_init_default(mgx_config *c);
/* Fill `c` with the `metagraph align` CLI defaults (cli/config/config.hpp:114-145 through
 * cli/align.cpp:33-69), for a graph with k-mer length k. */
void mgx_config_init_cli(mgx_config *c, uint32_t k);
/* DBGAlignerConfig::dna_scoring_matrix (aligner_config.cpp:164-183); penalties are negative. */
void mgx_config_set_dna_matrix(mgx_config *c, int8_t match, int8_t mm_transition, int8_t mm_transversion);
/* DBGAlignerConfig::unit_scoring_matrix over "ACGT" (aligner_config.cpp:185-204). */
void mgx_config_set_unit_matrix(mgx_config *c, int8_t match);
/* DBGAlignerConfig::set_scoring_matrix (aligner_config.cpp:128-162, DNA alphabet): from alignment_edit_distance /
 * alignment_match_score / alignment_mm_*_score; edit distance also zeroes the end bonuses. */
void mgx_config_set_scoring_matrix(mgx_config *c);

/* Largest DBGAlignerConfig::num_alternative_paths the device path keeps per query (a second instantiation of the
 * extension kernel with room for that many alignments runs when it is > 1).  More: MGX_ERR_UNSUPPORTED. */
#define MGX_MAX_ALTERNATIVE_PATHS 4u

/* Longest query the device path accepts (seed coordinates are 16-bit on the device; per-strand seed lists hold up to
 * 2 L + 64 entries).  Longer queries: MGX_ERR_UNSUPPORTED for the batch.  The reference has no such limit. */
#define MGX_MAX_QUERY_LENGTH 32704u

/* Per-read device arena limits (no reference counterpart; the reference uses the heap). */
typedef struct mgx_limits {
    uint32_t max_query_length;   /* longest read accepted in a batch (<= MGX_MAX_QUERY_LENGTH) */
    uint32_t max_columns;        /* DP-table columns per extension  */
    uint32_t max_seeds;          /* seeds per read and strand       */
    uint64_t cell_arena_bytes;   /* S/E/F storage per in-flight read */
} mgx_limits;
void mgx_limits_init_default(mgx_limits *l, uint32_t max_query_length);
/* The limits the last batch actually ran with (user limits, or what was derived from the config and the batch's
 * longest read).  A caller that sees MGX_ERR_CAPACITY statuses re-runs those reads with larger values. */
int mgx_aligner_get_limits(const struct mgx_aligner *a, mgx_limits *out);

typedef struct mgx_graph mgx_graph;
typedef struct mgx_aligner mgx_aligner;

/* One CIGAR run: Cigar::value_type (aligner_cigar.hpp:28). */
typedef struct mgx_cigar_op { uint32_t len; uint8_t op; uint8_t _pad[3]; } mgx_cigar_op;

/* One alignment: the observable state of `Alignment` (graph/alignment/alignment.hpp:132-331). */
typedef struct mgx_alignment {
    int32_t score;            /* get_score() */
    uint32_t offset;          /* get_offset() */
    uint32_t clipping;        /* get_clipping() */
    uint32_t end_clipping;    /* get_end_clipping() */
    uint32_t num_matches;     /* get_cigar().get_num_matches() */
    uint32_t n_nodes;         /* size() */
    uint32_t n_cigar;
    uint32_t seq_len;         /* get_sequence().size() */
    uint64_t nodes_begin;     /* index into mgx_results.nodes */
    uint64_t cigar_begin;     /* index into mgx_results.cigar */
    uint64_t seq_begin;       /* index into mgx_results.seqs  */
    uint8_t orientation;      /* get_orientation(): 1 = reverse complement of the query matched */
    uint8_t _pad[3];
    uint32_t n_labels;        /* label_columns.size() (alignment.hpp:327; 0 without an annotation) */
    uint64_t labels_begin;    /* index into mgx_results.labels: the alignment's label columns, ascending */
} mgx_alignment;

/* Results of one batch: AlignmentResults per query (alignment.hpp:366-406), in batch order. */
typedef struct mgx_results {
    uint64_t n_queries;
    const uint64_t *aln_begin;        /* n_queries+1 prefix offsets into `alignments` */
    const mgx_alignment *alignments;
    const uint64_t *nodes;
    const mgx_cigar_op *cigar;
    const char *seqs;
    const int32_t *status;            /* per query: MGX_OK or MGX_ERR_CAPACITY */
    const uint32_t *labels;           /* Alignment::label_columns of all alignments (label-aware alignment; else NULL) */
} mgx_results;

/* Seeding-only output (DeBruijnGraph::map_to_nodes_sequentially for both strands). */
typedef struct mgx_mapping {
    uint64_t n_queries;
    const uint64_t *node_begin;       /* n_queries+1 prefix offsets (per strand array) */
    const uint64_t *nodes_fwd;        /* BOSS::map_to_edges of the query (boss.cpp:996-1045) */
    const uint64_t *nodes_rc;         /* ... of its reverse complement (sequence_graph.cpp:563-573) */
} mgx_mapping;

/* Counters for roofline accounting: BOSS primitives actually executed. */
typedef struct mgx_stats {
    uint64_t n_reads;
    uint64_t n_rank_lines;      /* 64-B block reads issued for rank_W / W / last        */
    uint64_t n_select_lines;    /* 64-B block reads issued for select_last / select_W  */
    uint64_t n_bit_lines;       /* side-table reads (MEM terminus bits, first chars)   */
    uint64_t n_columns;         /* DP columns computed (none for a read of n_lane_exact_reads) */
    uint64_t n_extensions;      /* DefaultColumnExtender::extend calls (none for a read of n_lane_exact_reads: no DP ran) */
    uint64_t n_seeds;
    uint64_t n_map_lines;       /* part of n_rank_lines + n_select_lines issued by the k-mer mapping kernel */
    uint64_t n_capacity_errors; /* reads whose status is MGX_ERR_CAPACITY */
    uint64_t phase_cycles[8];   /* k_align shader cycles summed over waves: query prep, seeding, extend,
                                   backtrack, driver rest, output (profiling aid) */
    uint64_t extend_cycles[8];  /* extend() breakdown: pop, stage+band, outgoing, column, scan, commit, conv, push */
    double seed_kernel_ms, align_kernel_ms;   /* HIP-event time of the k-mer mapping kernel and of the whole
                                                 alignment stage (seeding + sort + extension), last batch */
    double seeding_ms, sort_ms, extend_ms;    /* split pipeline only (0 otherwise): seeding kernel, work sort (with the lane
                                                 kernel's exact exit, k_lane_exact, which runs in front of it), extension kernel */
    uint64_t n_seed_lines;      /* split pipeline: part of the line counters issued by the seeding kernel */
    uint64_t n_fast_columns;    /* part of n_columns computed by the register-resident chain path */
    uint64_t extend_kernels;    /* which extension kernels the last batch launched (MGX_KERNEL_* bits): what a parity test
                                   asserts so that it is known to have exercised the kernel it means to */
    uint64_t n_lane_reads;      /* reads the lane-per-read kernel finished on its own (the rest went on to the group kernel) */
    double lane_ms;             /* HIP-event time of the lane-per-read kernel (part of extend_ms) */
    uint64_t n_lane_lines;      /* part of the line counters issued by the lane-per-read kernel */
    uint64_t n_lane_columns;    /* part of n_columns computed by it (for the reads it passes on too) */
    uint64_t lane_bail_reads[32]; /* reads the lane-per-read kernel passed on to the group kernel, by reason (the LANE_BAIL codes of
                                   csrc/lane_read.hpp: 3 second strand, 4 many seeds, 5 invalid characters, 10 fork, 14 / 16 wide band,
                                   15 node seen before, 19 a later seed survives, 26 backward extension, 27 an equal-score batch of columns on the query,
                                   28 more parked columns than frontier slots, ...) */
    uint64_t n_capacity_retried; /* queries the last mgx_fetch_results / mgx_align_batch re-aligned with doubled limits after an
                                   MGX_ERR_CAPACITY status (they are in its results like any other query; n_capacity_errors counts
                                   them too) */
    uint64_t n_seed_lane_reads; /* reads the lane-per-read seeder (round 6, csrc/seed_lane.hpp) seeded on its own; the rest went on to the
                                   wave-per-read seeding kernel */
    double seed_lane_ms;        /* HIP-event time of the lane-per-read seeder (part of seeding_ms) */
    uint64_t seed_lane_left_reads[16]; /* reads it left to the seeding kernel, by reason (seed_lane.hpp: 1 read length, 2 k-mer positions,
                                   3 characters outside ACGT, 4 the DUST scan could mask something, 5 alternative nodes, 6 / 7 seeds) */
    uint64_t n_lane_exact_reads; /* part of n_lane_reads: reads finished through the lane kernel's exact exit (k_lane_exact, csrc/lane_read.hpp
                                   lane_exact(): the first seed of the strand aligned first spans the query, so the result is the all-match
                                   alignment over the seed's nodes and no DP runs; n_lane_reads + sum(lane_bail_reads) == reads still holds) */
    uint64_t n_lane_exact_path_reads; /* part of n_lane_reads, none of them in n_lane_exact_reads: reads finished through the exit's path
                                   class (exact level 2): the first seed starts at the query's first character and ends at a fork or a
                                   merge, every k-mer of the strand is a node; the same closed form over the strand's mapped nodes.
                                   Both counters count label-aware reads too (k_lane_exact_labeled: one label all along) */
    uint64_t n_lane_exact_sub_reads; /* part of n_lane_reads, none of them in the two counters above: reads finished through the exit's
                                   substitution class (exact level 3; k_lane_exact_sub, label-aware batches k_lane_exact_sub_labeled):
                                   the strand's node array has one run of zeros behind its first entry, the graph walk across it
                                   succeeds, and the result is the alignment with one mismatch over the mapped and the walked nodes;
                                   label-aware: the read keeps one label L along the mapped and the walked nodes, label list [L] */
} mgx_stats;
enum { MGX_KERNEL_GRP8 = 1, MGX_KERNEL_GRP8_PRIM = 2, MGX_KERNEL_GRP8_ALT = 4, MGX_KERNEL_EXT64 = 8, MGX_KERNEL_LANE = 16,
       MGX_KERNEL_LAB64 = 32, MGX_KERNEL_GRP8_LAB = 64, /* the label-aware builds of the 64-lane and the 8-lane kernel */
       MGX_KERNEL_LAB64_BX = 128, MGX_KERNEL_GRP8_LAB_BX = 256 /* ... and their builds with per-branch x-drop (global_xdrop = 0) */ };

int mgx_device_count(void);                 /* number of visible HIP devices (0 without a GPU) */
const char *mgx_last_error(void);
uint32_t mgx_abi_version(void);

/* Upload a BOSS table and build the device index.  Replaces BOSS::load + DBGSuccinct::load
 * (boss.cpp:338-394, dbg_succinct.cpp:690-785) as the source of W/last/F.  `device` is the HIP ordinal. */
int mgx_graph_create(const mgx_boss_view *view, int device, mgx_graph **out);
void mgx_graph_destroy(mgx_graph *g);
uint32_t mgx_graph_k(const mgx_graph *g);            /* DeBruijnGraph::get_k  (sequence_graph.hpp:176) */
uint64_t mgx_graph_max_index(const mgx_graph *g);    /* DeBruijnGraph::max_index (dbg_succinct.cpp:686-688); PRIMARY: 2 x that,
                                                      * as CanonicalDBG::max_index (canonical_dbg.hpp:96) */
uint64_t mgx_graph_device_bytes(const mgx_graph *g);
uint64_t mgx_graph_num_edges(const mgx_graph *g);    /* boss::BOSS::num_edges: the edges of the stored table (PRIMARY: not doubled) */
uint32_t mgx_graph_mode(const mgx_graph *g);         /* MGX_MODE_* the graph was created (or loaded) with */

/* DBGAligner<>::DBGAligner(graph, config) (dbg_aligner.cpp:33-61): clamps seed lengths,
 * validates scores.  `limits` may be NULL (defaults for 512-bp reads). */
int mgx_aligner_create(const mgx_graph *g, const mgx_config *config,
                       const mgx_limits *limits, mgx_aligner **out);
void mgx_aligner_destroy(mgx_aligner *a);
/* IDBGAligner::get_config() after clamping. */
int mgx_aligner_get_config(const mgx_aligner *a, mgx_config *out);

/* IDBGAligner::align_batch (dbg_aligner.hpp:32-33, dbg_aligner.cpp:251-355).
 * `seqs` holds the concatenated raw query bytes, query i = seqs[offsets[i] .. offsets[i+1]).
 * With seqs_on_device != 0, `seqs` and `offsets` are device pointers (reads already in HBM). */
int mgx_align_batch(mgx_aligner *a, const char *seqs, const uint64_t *offsets, uint64_t n_queries,
                    int seqs_on_device, mgx_results *out);

/* The two halves of mgx_align_batch: run the kernels and leave the results in HBM / copy them out.
 * mgx_align_batch(a, ...) == mgx_align_batch_device(a, ...) followed by mgx_fetch_results(a, out).
 * mgx_fetch_results re-aligns the queries whose per-read arenas overflowed (MGX_ERR_CAPACITY: the reference's tables grow on
 * the heap, it has no such status) with doubled limits, up to six times, and reads them from the batch's device buffers:
 * with seqs_on_device != 0 the caller's `seqs` / `offsets` must stay valid until it returns.  The raw device results
 * (mgx_device_results, the RCCL gather path) are what the kernels wrote: statuses included. */
int mgx_align_batch_device(mgx_aligner *a, const char *seqs, const uint64_t *offsets, uint64_t n_queries,
                           int seqs_on_device);
int mgx_fetch_results(mgx_aligner *a, mgx_results *out);
/* Device-resident results of the last batch, for gathering over RCCL without a host round trip:
 * `headers` = n_queries fixed-size records of `header_bytes` bytes each (status, n_alignments, score,
 * offset, n_nodes, n_cigar, seq_len, orientation, stream offset, ...), `stream` = `stream_words`
 * 32-bit words holding nodes / packed CIGAR runs (len << 3 | op) / path characters. */
int mgx_device_results(mgx_aligner *a, const void **headers, uint64_t *header_bytes, uint64_t *n_queries,
                       const void **stream, uint64_t *stream_words);
/* The results of the last batch in the layout of mgx_results, decoded by kernels and LEFT IN DEVICE MEMORY — what a consumer on
 * the device can read (mgx_device_results exposes the kernels' private record and stream encoding).  Every pointer of `out`
 * is device memory owned by the aligner, valid until its next batch, fetch, decode or format call; `sizes` holds the element
 * counts of alignments, nodes, cigar, seqs and labels (aln_begin has n_queries + 1 elements, status n_queries); out->labels is
 * NULL when sizes->n_labels is 0.  Only the five totals (40 bytes) travel to the host.
 *   - Array by array and byte for byte, padding included, `out` holds what mgx_results_from_raw_labeled gives for the records
 *     and the stream of mgx_device_results.  That is, the results are PRE-RETRY: a query whose per-read arenas overflowed has
 *     status MGX_ERR_CAPACITY and no alignments (mgx_fetch_results re-aligns those; this call does not).
 *   - With post_chain_alignments the arrays hold the UNCHAINED alignments (chaining runs on the host inside mgx_fetch_results).
 *   - Call it after mgx_align_batch_device or mgx_align_batch, while that batch is still the staged one: without an aligned
 *     batch on the handle, or after another batch call (mgx_map_batch, mgx_map_summary_batch) staged again, MGX_ERR_INVALID.
 *     With seqs_on_device != 0 the reads are not needed.  A batch of 0 queries: MGX_OK, all sizes 0.
 *   - 2^31 - 1 queries or more: MGX_ERR_UNSUPPORTED.  An output buffer that cannot be allocated: MGX_ERR_OOM, naming the bytes.
 * The same two kernels serve mgx_fetch_results / mgx_align_batch under the pipeline option decode_on_device=1
 * (mgx_aligner_set_pipeline): the seven arrays then come to pinned host memory of the handle instead of records and stream to
 * pageable vectors and a one-thread decode; the view returned is equal to the option-off view in every configuration. */
typedef struct mgx_results_sizes { uint64_t n_alignments, n_nodes, n_cigar, n_seq_bytes, n_labels; } mgx_results_sizes;
int mgx_decode_results_device(mgx_aligner *a, mgx_results *out, mgx_results_sizes *sizes);
/* Test hook: out4 = launches of k_decode_size, launches of k_decode_write, bytes copied device-to-host by the decode,
 * mgx_fetch_results calls the option decode_on_device served — since the library was loaded. */
void mgx_decode_kernel_launch_counts(uint64_t *out4);
/* Capacity (32-bit words) of the device stream buffer behind mgx_device_results: a function of the batch shape only,
 * so equal on all ranks that run equally shaped batches — the padded RCCL gather relies on it. */
uint64_t mgx_device_stream_capacity(const mgx_aligner *a);
/* Host-only decode of raw result records (one rank's `headers` / `stream` as mgx_device_results exposes them, e.g.
 * after an RCCL gather on the root) into the mgx_results view that mgx_format_tsv prints from — the root's side of
 * cli/align.cpp:469-473.  Needs no GPU.  `*store` owns the memory behind `out`; release with mgx_raw_store_free. */
typedef struct mgx_raw_store mgx_raw_store;
int mgx_results_from_raw(const void *headers, uint64_t n_queries, const uint32_t *stream, uint64_t stream_words,
                         mgx_raw_store **store, mgx_results *out);
void mgx_raw_store_free(mgx_raw_store *store);
/* chain_alignments<LocalAlignmentLess> (aligner_chainer.cpp:555-720, called at dbg_aligner.cpp:328-332) over the decoded
 * results of a batch whose aligner had post_chain_alignments set: queries seqs[offsets[q] .. offsets[q + 1]) as they were
 * aligned, k = the graph's k (node_overlap = k - 1).  Host code, needs no GPU.  A chain's nodes hold 0 where the path has no
 * graph node, its spelling '$' at a gap, its CIGAR MGX_OP_NODE_INSERTION runs and clipping runs inside. */
int mgx_chain_alignments(const mgx_config *config, uint32_t k, const mgx_results *in, const char *seqs, const uint64_t *offsets,
                         mgx_raw_store **store, mgx_results *out);
/* Test hooks: keep and fetch the per-read seed lists (DBGAligner::build_seeders products). */
void mgx_aligner_keep_seeds(mgx_aligner *a, int keep);
int mgx_fetch_seed_info(mgx_aligner *a, uint32_t *info6, uint32_t *seeds, uint32_t *max_seeds_out);

/* Hot loop #1 only: map both strands to nodes (dbg_aligner.cpp:210,227-231): DeBruijnGraph::map_to_nodes_sequentially of the
 * query and of its reverse complement — what the ALIGNER seeds from; on a PRIMARY graph those of the CanonicalDBG wrapper
 * (canonical_dbg.cpp:55-146,551-560).  Both node arrays travel to the host.  This is not DeBruijnGraph::map_to_nodes (they
 * differ on CANONICAL and PRIMARY graphs): for that, and for the counts of `align --map`, see mgx_map_summary_batch. */
int mgx_map_batch(mgx_aligner *a, const char *seqs, const uint64_t *offsets, uint64_t n_queries,
                  int seqs_on_device, mgx_mapping *out);

/*
 * `metagraph align --map` (map_sequences_in_file, cli/align.cpp:71-179): DeBruijnGraph::map_to_nodes of every query, summarised
 * on the device.  Node of k-mer i of a query with n k-mers (a query shorter than k has none):
 *   BASIC      the forward mapping, node mask applied (dbg_succinct.cpp:484-497)
 *   CANONICAL  min(forward[i], reverse-complement[n - 1 - i]) over BOSS indexes, 0 if either is missing; the mask after the minimum
 *              (dbg_succinct.cpp:436-482)
 *   PRIMARY    the CanonicalDBG wrapper's path (what mgx_map_batch gives) as base nodes: id > n_edges ? id - n_edges : id
 *              (cli/align.cpp:345-348, canonical_dbg.cpp:148-154)
 * Counts per query (cli/align.cpp:134-164): non-zero nodes, k-mers, distinct non-zero nodes.
 * map_length: 0 or k = whole k-mers.  0 < L < k (--align-length L): the query's len - L + 1 windows of the FORWARD strand only,
 * node = the first one call_nodes_with_suffix_matching_longest_prefix(window, ., L) reports (dbg_succinct.cpp:307-393), 0 if none
 * or if the window holds a character outside ACGT — BASIC and CANONICAL graphs.  On a PRIMARY graph the reference casts the
 * CanonicalDBG wrapper it has just built to a DBGSuccinct there (cli/align.cpp:117 after :347), which is undefined behaviour:
 * MGX_ERR_UNSUPPORTED.  map_length > k: MGX_ERR_INVALID.
 * Without MGX_MAP_WANT_NODES the only device-to-host traffic of a batch is the 12-byte records (node_begin and nodes are NULL).
 * Runs on the aligner's stream and honours the graph's mask and the map_pipe= switch like mgx_map_batch.  The views stay valid
 * until the next batch call on this aligner.
 */
typedef struct mgx_map_counts { uint32_t n_discovered, n_kmers, n_unique; } mgx_map_counts;
typedef struct mgx_map_summary {
    uint64_t n_queries;
    const mgx_map_counts *counts;     /* n_queries */
    const uint64_t *node_begin;       /* n_queries + 1; NULL unless MGX_MAP_WANT_NODES */
    const uint64_t *nodes;            /* the map_to_nodes result, rules above */
} mgx_map_summary;
/* MGX_MAP_KEEP_NODES: k_map_summary writes the 64-bit node array to device memory, where mgx_format_map_batch reads it; nothing
 * more is copied to the host than without a flag (node_begin and nodes stay NULL, out4[3] of mgx_map_kernel_launch_counts does
 * not move).  MGX_MAP_WANT_NODES leaves the array on the device as well. */
enum { MGX_MAP_WANT_NODES = 1, MGX_MAP_KEEP_NODES = 2 };
int mgx_map_summary_batch(mgx_aligner *a, const char *seqs, const uint64_t *offsets, uint64_t n_queries,
                          int seqs_on_device, uint32_t map_length /* 0 = k; > k: MGX_ERR_INVALID */,
                          uint32_t flags, mgx_map_summary *out);
/* --query-presence, in double exactly as the reference writes it.  map_length 0 or k: DeBruijnGraph::find
 * (sequence_graph.cpp:65-89): absent if query_len < k, else present iff n_kmers - n_discovered <= (size_t)(n_kmers * (1 - f)).
 * map_length < k (cli/align.cpp:139-149): present iff n_discovered >= (size_t)(n_kmers - n_kmers * (1 - f)) — a query without a
 * window is present.  Returns 1 / 0.  Host code, needs no GPU. */
int mgx_map_present(const mgx_map_counts *c, uint64_t query_len, uint32_t k, uint32_t map_length, double discovery_fraction);
/* The bytes map_sequences_in_file prints for one query (cli/align.cpp:91-173): MGX_MAP_FMT_NODES "{window}: {node}\n" per window
 * (needs MGX_MAP_WANT_NODES), _COUNT_KMERS "{header}\t{discovered}/{kmers}/{unique}\n", _QUERY_PRESENCE "0\n" / "1\n",
 * _FILTER_PRESENT ">{header}\n{query}\n" or nothing.  Same return convention as mgx_format_tsv.  Host code, needs no GPU. */
enum { MGX_MAP_FMT_NODES = 0, MGX_MAP_FMT_COUNT_KMERS = 1, MGX_MAP_FMT_QUERY_PRESENCE = 2, MGX_MAP_FMT_FILTER_PRESENT = 3 };
size_t mgx_format_map(const mgx_map_summary *s, uint64_t query_index, const char *header, const char *query, size_t query_len,
                      uint32_t k, uint32_t map_length, int format, double discovery_fraction, char *buf, size_t buf_len);
/* Test hook: since the library was loaded, out4[0 .. 2] = launches of k_map_summary's short-read form, of its long-read form and
 * of k_map_subk; out4[3] = bytes of node arrays mgx_map_summary_batch has copied to the host (0 in counts mode). */
void mgx_map_kernel_launch_counts(uint64_t *out4);

int mgx_aligner_stats(const mgx_aligner *a, mgx_stats *out);
/* Test hook: launches of each extension kernel since the library was loaded, out5[b] = the kernel of bit b of MGX_KERNEL_*
 * (8-lane groups, its PRIMARY build, its alternative-paths build, the 64-lane kernel, the lane-per-read kernel). */
void mgx_kernel_launch_counts(uint64_t *out5);

/* Kernel-selection switches; every setting gives the same alignments (the parity suite runs them all).  "split8" names the
 * (only) pipeline: seeding kernel with one wavefront per read, radix sort of the reads by predicted extension work, extension
 * kernel(s).  "general" / "chain": the extension's register-resident chain path off / on.  "key=value" (-1 = automatic):
 *   ext64=0|1|2          small batches on the one-read-per-wavefront 64-lane kernel (default 1) or on the 8-lane groups;
 *                        label-aware aligners: 2 = every batch on the 64-lane labeled kernel
 *   groups_per_wave=n    8-lane kernel: n = 1 .. 8 groups of a wavefront take reads, 0 = all (default: from the batch size)
 *   multi_pass=0|1       the multi-pass extension: a launch extends a limited number of seeds per read (1, then 4, then 16, from
 *                        pass 24 on all), unfinished reads go on in the next launch from a resume record (default: automatic
 *                        from the seeds per read)
 *   resume_cap=n         multi-pass extension: at most n resume records per pass (default -1: one per read, memory permitting);
 *                        a read that finds no room for a record goes on without a seed limit in the same launch
 *   lane=0|1             the lane-per-read kernel in front of the group kernel (default: automatic).  1 means "where the configuration
 *                        allows it": an aligner with global_xdrop = 0 (per-branch x-drop) never runs it, nor its exact exit below —
 *                        the lane kernels encode the global rule (mgx_stats: n_lane_reads and both exact counters stay 0)
 *   exact=0|1|2|3        the lane kernel's exact exit: reads whose result is known when seeding ends are finished in closed form,
 *                        without DP.  1: reads whose first seed spans the query; 2: also reads whose first seed starts at the query's
 *                        first character and whose every k-mer is a node (perfect reads that cross a fork or a merge); 3: also reads
 *                        with one substitution behind their first k characters, where the graph walk across it succeeds
 *                        (batches whose scores make that alignment the strict optimum; elsewhere 3 means 2).  Default:
 *                        automatic — level 3 for the batches the lane kernel takes of its own accord, label-aware ones included;
 *                        1 / 2 / 3: wherever the lane kernel runs and the configuration allows it.  Label-aware batches (wherever the lane kernel takes them:
 *                        no dummy node's row holds a label) are included, at every level and in the automatic default: there
 *                        the exit takes the reads that keep one label all along — the label filter leaves the seeds one label L
 *                        and every node of the path (at level 3: the nodes walked across the substitution too) has the row { L }
 *                        — and the label list of the alignment is [L]; with one
 *                        seed per k-mer the first class is the reads of k characters.  Results never depend on the option
 *   device_share=n       n handles are at work on this device at the same time (worker threads): this handle sizes its per-slot
 *                        arenas for 1 / n of the machine (default 1: all of it)
 *   seed_lane=0|1        the lane-per-read seeder in front of the seeding kernel (default: automatic)
 *   seed_wps=4|8         wavefronts per SIMD of the short-read seeding kernel (default 8)
 *   map_pipe=0|1|2       the mapping kernel as a request / response machine: never / from 65536 chains on (default) / always
 *   retry_capacity=0     capacity statuses are handed to the caller instead of re-aligning those queries with larger limits
 *   decode_on_device=0|1 mgx_fetch_results / mgx_align_batch decode the batch into the mgx_results layout by kernels and copy the
 *                        seven arrays to pinned host memory (default 0: records and stream are copied, one host thread decodes);
 *                        the view is the same.  Ignored (host decode) once the aligned batch is no longer the staged one
 *   no_compact / no_alias / no_bt_runs / no_flat = 1   A/B forms of the column records and loops
 * Unknown name: MGX_ERR_INVALID.  (Measurement probes that change results or occupancy exist only in -DMGX_PROBES builds.) */
int mgx_aligner_set_pipeline(mgx_aligner *a, const char *name);
/* The HIP stream (a hipStream_t, passed as void * so that this header needs no HIP header) every kernel launch, asynchronous
 * copy and device-library call of this aligner goes to; its blocking copies synchronise that stream only.  NULL (the state
 * after creation) = the legacy default stream.  With a stream of its own per handle, the aligners of several worker threads on
 * one device — the reference builds one aligner per thread-pool task, cli/align.cpp:440-475 — run side by side instead of
 * serialising on the default stream.  The stream stays the caller's (not destroyed with the aligner); device buffers handed to
 * mgx_align_batch_device / mgx_map_batch must be ready on it.  mgx_aligner_create_stream gives the aligner a non-blocking
 * stream that it owns (destroyed with it) — what host/mgx_align -p N does per worker. */
/* Device memory of destroyed aligners is kept per device for the next aligner (one aligner per task is the reference's model:
 * without this every task paid for fresh multi-GB arenas); it is released when an allocation of the library fails and by this
 * call — for a host that wants the memory back for something else. */
int mgx_device_trim(int device);
int mgx_aligner_set_stream(mgx_aligner *a, void *hip_stream);
int mgx_aligner_create_stream(mgx_aligner *a);
void *mgx_aligner_get_stream(const mgx_aligner *a);

/*
 * The gather of complete alignments over RCCL (north_star: "RCCL-over-xGMI used only to gather alignment results").
 * Replaces, for one aligner per device, the reference's output loop (cli/align.cpp:469-473: every task prints its queries under a
 * mutex): every rank's device results of a batch (mgx_device_results: n_queries records + the used words of its stream) travel to
 * `root`, which decodes them with mgx_results_from_raw[_labeled] and prints.  Two phases: an all-gather of (n_queries, used words),
 * then one group of send / receive pairs (xGMI is point-to-point).  librccl.so is opened at the first call (dlopen: libmgx does not
 * link it); without it every mgx_gather_create* returns MGX_ERR_UNSUPPORTED.  No other call of this library communicates.
 *   one process per device:  rank 0 calls mgx_gather_unique_id and hands the bytes to the other ranks (a file, MPI, a socket: the
 *                            host's business), every rank calls mgx_gather_create_rank; or mgx_gather_create_comm over an ncclComm_t
 *                            the host has already (not destroyed with the handle);
 *   one process, D devices:  mgx_gather_create_local (ncclCommInitAll) fills out[0 .. D); worker thread r uses out[r] — the calls
 *                            below are collective and block, so every device needs its own thread (host/mgx_align --rccl-gather).
 */
typedef struct mgx_gather mgx_gather;
uint64_t mgx_gather_unique_id_bytes(void);
int mgx_gather_unique_id(void *id_out, uint64_t id_bytes);
int mgx_gather_create_rank(const void *unique_id, uint64_t id_bytes, int rank, int world, int root, int device, mgx_gather **out);
int mgx_gather_create_comm(void *nccl_comm, int rank, int world, int root, int device, mgx_gather **out);
int mgx_gather_create_local(const int *devices, int n_devices, int root, mgx_gather **out /* [n_devices] */);
void mgx_gather_destroy(mgx_gather *g);
int mgx_gather_world(const mgx_gather *g);
int mgx_gather_rank(const mgx_gather *g);
/* Collective: every rank, after mgx_align_batch_device on ITS aligner (same device as the handle).  Returns when this rank's
 * transfers are enqueued on the handle's own stream; the aligner's device results must stay untouched until mgx_gather_finish. */
int mgx_gather_start(mgx_gather *g, mgx_aligner *a);
/* Waits for this rank's transfers.  On the root the caller's arrays of `world` entries receive, per rank r, the number of
 * queries, host pointers to its records and stream (valid until the next mgx_gather_start / mgx_gather_destroy) and the
 * stream's words — the arguments of mgx_results_from_raw.  On the other ranks the arrays are ignored (may be NULL). */
int mgx_gather_finish(mgx_gather *g, uint64_t *n_queries, const void **headers, const uint32_t **streams, uint64_t *stream_words);

/* Format one query's results exactly like format_alignment() (cli/align.cpp:254-285):
 * "header\tquery\t(+|-)\tpath\tscore\tnum_matches\tcigar\toffset\n", or the "*" line.
 * Returns the number of bytes needed (excluding NUL); writes at most buf_len bytes. */
size_t mgx_format_tsv(const mgx_results *res, uint64_t query_index, const char *header,
                      const char *query, size_t query_len, int32_t min_path_score,
                      char *buf, size_t buf_len);

/* Format one query's results like `metagraph align --json` (cli/align.cpp:287-305): one line per alignment, the JSON of
 * Alignment::to_json / path_json (alignment.cpp:704-963) as Json::writeString emits it with indentation "" (keys in
 * lexicographic order, no white space); a query without alignments yields {"name":...,"sequence":""}.  `k` is the graph's
 * node length (DeBruijnGraph::get_k()).  Returns the number of bytes needed (excluding NUL); writes at most buf_len bytes. */
size_t mgx_format_json(const mgx_results *res, uint64_t query_index, const char *header,
                       const char *query, size_t query_len, uint32_t k, char *buf, size_t buf_len);

/*
 * Label-aware alignment (graph/alignment/aligner_labeled.{hpp,cpp}, annotation_buffer.{hpp,cpp}; BASELINE config 3).
 * On the device: the whole LabeledAligner — filter_seeds, LabeledExtender's per-column label sets (flush / call_outgoing / the
 * label-bounded backtracking), the per-label aggregator (mgx_labeled_aligner_create below) — over a row-major label matrix
 * whose rows ARE the label sets AnnotationBuffer would fetch, plus the batched BinaryMatrix::get_rows of
 * AnnotationBuffer::fetch_queued_annotations as an entry point of its own (annotation_buffer.cpp:182; ColumnMajor::get_rows,
 * annotation/binary_matrix/column_sparse/column_major.cpp:27-44 — 1000 columns x |rows| random bit tests in the reference).
 * Label coordinates: read from `.column.annodbg.coords` / `.column_coord.annodbg` files on the host and on the device
 * (mgx_column_coord_file_read, mgx_annotation_load_coord_columns_device, "files" below), kept row-major on the device and answered by
 * mgx_annotation_get_row_tuples; the anchor DP of seed chaining is mgx_chain_seeds, and the chain stage of coordinate mode for a
 * whole read batch — both strands' seeds, filter_seeds with coordinates, the anchors, the sort and the DP, left in device memory —
 * is mgx_chain_tables_batch (mgx_seed_chainer_create).  Not built: the rest of LabeledAligner's coordinate mode, i.e. the extension
 * half of chaining (aligner_labeled.cpp:361-448, aligner_chainer.cpp:47-339, dbg_aligner.cpp:155-250,388-529) — an annotation
 * with coordinates is refused by mgx_labeled_aligner_create.
 *
 * mgx_annotation_create stands in for the annotator argument of LabeledAligner<>(graph, config, annotator)
 * (aligner_labeled.hpp:125-127): the binary matrix as column bit vectors, columns[j] = ceil(n_rows / 64) words, bit r =
 * row r carries label j; row = AnnotatedDBG::graph_to_anno_index(node) = node - 1 (graph/annotated_dbg.hpp:50-52).
 * The device keeps it row-major (one 8-byte word per row; rows with several labels point into a label list).
 */
typedef struct mgx_annotation mgx_annotation;
int mgx_annotation_create(uint64_t n_rows, uint32_t n_labels, const uint64_t *const *columns, int device, mgx_annotation **out);
/* The same from the columns' set rows, the content of a ColumnCompressed annotation (one sd_vector of row indices per label):
 * rows[col_begin[j] .. col_begin[j + 1]) = the rows with label j (any order, no duplicates); col_begin: host array of
 * n_labels + 1 entries; rows: host or (on_device != 0) device pointer.  One sort on the device instead of n_labels bit vectors
 * of n_rows bits each on the host. */
int mgx_annotation_create_sparse(uint64_t n_rows, uint32_t n_labels, const uint64_t *col_begin, const uint64_t *rows,
                                 int on_device, int device, mgx_annotation **out);
void mgx_annotation_destroy(mgx_annotation *a);
uint64_t mgx_annotation_device_bytes(const mgx_annotation *a);
uint64_t mgx_annotation_num_rows(const mgx_annotation *a);
uint32_t mgx_annotation_num_labels(const mgx_annotation *a);
/* BinaryMatrix::get_rows for a batch of rows, as CSR: labels of rows[i] = out_labels[out_begin[i] .. out_begin[i + 1]),
 * ascending (what annotation_buffer.cpp:185 sorts into).  Calls on one handle are serialised inside (the handle owns the scratch
 * buffers); they run on the null stream.  out_begin has n + 1 entries; `cap` = entries out_labels holds: a
 * batch with more returns MGX_ERR_CAPACITY with the needed count in *n_labels_out (out_begin is complete, out_labels
 * untouched).  rows_on_device / out_on_device != 0: device pointers (rows already in HBM / results left in HBM). */
int mgx_annotation_get_rows(mgx_annotation *a, const uint64_t *rows, uint64_t n, int rows_on_device,
                            uint64_t *out_begin, uint32_t *out_labels, uint64_t cap, int out_on_device, uint64_t *n_labels_out);

/* k-mer coordinates (annot::ColumnCoordAnnotator: a MultiIntMatrix next to the binary matrix; AnnotationBuffer::has_coordinates,
 * annotation_buffer.cpp:26-33) for an annotation created from the same n_labels / col_begin / rows with
 * mgx_annotation_create_sparse: pair x (label j = the column whose range holds x, row rows[x]) has the ascending coordinates
 * coords[coord_begin[x] .. coord_begin[x + 1]).  Host arrays.  Round 6: the annotation and its batched lookup
 * (mgx_annotation_get_row_tuples = MultiIntMatrix::get_row_tuples, what AnnotationBuffer::fetch_queued_annotations calls,
 * annotation_buffer.cpp:166-181) are on the device, and so is the chain stage of LabeledAligner's coordinate mode (seed chaining,
 * aligner_labeled.cpp:457-462): mgx_seed_chainer_create / mgx_chain_tables_batch below.  The mode as a whole is not —
 * mgx_labeled_aligner_create refuses such an annotation (MGX_ERR_UNSUPPORTED). */
int mgx_annotation_set_coordinates(mgx_annotation *a, uint32_t n_labels, const uint64_t *col_begin, const uint64_t *rows,
                                   const uint64_t *coord_begin, const int64_t *coords);
/* The same with rows, coord_begin and coords in device memory (col_begin stays a host array); the row-major form is built by
 * kernels: the same tables, and for a row outside the matrix or a descending tuple the same code and message.  The
 * number of launches and allocations does not depend on n_labels. */
int mgx_annotation_set_coordinates_device(mgx_annotation *a, uint32_t n_labels, const uint64_t *col_begin, const uint64_t *rows,
                                          const uint64_t *coord_begin, const int64_t *coords);
int mgx_annotation_has_coordinates(const mgx_annotation *a);
int mgx_annotation_get_row_tuples(mgx_annotation *a, const uint64_t *rows, uint64_t n, uint64_t *out_begin, uint32_t *out_labels,
                                  uint64_t label_cap, uint64_t *out_coord_begin, int64_t *out_coords, uint64_t coord_cap,
                                  uint64_t *n_labels_out, uint64_t *n_coords_out);

/* chain_seeds (aligner_chainer.cpp:341-542) — the anchor DP of seed chaining, on the device.  An anchor is one (seed, label,
 * coordinate) of a (query, strand): the reference's TableElem (aligner_chainer.cpp:23-36, same 32 bytes).  Input: the anchors of
 * n_lists lists (list l = anchors[list_begin[l] .. list_begin[l + 1])) in any order, chain_score = the seed's length
 * (seed_end - seed_clipping), query_size[l] = the length of the list's query; config->min_seed_length sets the gap cost.  Output:
 * every list sorted as the reference sorts it — (label, coordinate, seed_clipping, seed_end) descending — with the final
 * chain_score of every anchor, and backtrace_out[x] = the anchor (index relative to its list's begin, in the sorted order)
 * anchor x's best chain continues with, 0xFFFFFFFF for none.  Bit-identical to the reference's AVX2 loop incl. the float gap
 * cost (tabulated on the host with the host's libm).  At most 6144 anchors per list.  Host arrays. */
typedef struct mgx_chain_anchor {
    uint64_t label;
    int64_t coordinate;
    int32_t seed_clipping, seed_end;
    int32_t chain_score;
    uint32_t seed_index;
} mgx_chain_anchor;
int mgx_chain_seeds(const mgx_config *config, int device, const mgx_chain_anchor *anchors, const uint64_t *list_begin,
                    const uint32_t *query_size, uint64_t n_lists, mgx_chain_anchor *sorted_out, uint32_t *backtrace_out);

/* The chain stage of LabeledAligner's coordinate mode as one device pipeline: the data-parallel half of what the reference does
 * for a query when its annotation carries k-mer coordinates (dbg_aligner.cpp:545-550, aligner_labeled.cpp:594-721,
 * aligner_chainer.cpp:341-542).  Reads go in; per (query, strand) the seeds filter_seeds keeps and the finished tables of
 * chain_seeds come out and stay in device memory for the stage that consumes them.  The sequential half — backtracking the
 * chains, extend_chain / align_connect, the aggregator — is not built.
 *
 * mgx_seed_chainer_create: a handle for that stage.  graph: BASIC mode (the reference has coordinates on BASIC graphs only);
 * annotation: mgx_annotation_has_coordinates() != 0, on the graph's device, outliving the handle;
 * config->forward_and_reverse_complement != 0 (the reference chains only where it seeds both strands,
 * dbg_aligner.cpp:290-297,545-550); config->chain_alignments = 0 as everywhere.  The handle's config is what LabeledAligner's
 * constructor leaves: DBGAligner's clamps, min / max_seed_length <= k, global_xdrop = 0, chain_alignments = 1
 * (mgx_aligner_get_config shows it).  Anything else: MGX_ERR_UNSUPPORTED / MGX_ERR_INVALID with the field named in
 * mgx_last_error.  mgx_labeled_aligner_create keeps refusing such an annotation; on this handle every align / fetch / format call
 * (mgx_align_batch, mgx_align_batch_device, mgx_fetch_results, mgx_device_results, mgx_decode_results_device,
 * mgx_fetch_seed_info, mgx_format_*_batch, mgx_gather_start) returns MGX_ERR_UNSUPPORTED.  Destroyed with mgx_aligner_destroy;
 * options, streams and statistics (mgx_aligner_set_pipeline "seed_lane=..", mgx_aligner_stats: the seeding fields) as on any
 * aligner.
 *
 * mgx_chain_tables_batch, per (query, strand) — list 2q = query q, list 2q + 1 = its reverse complement:
 *   1. seeding as a label-aware aligner seeds (the same kernels);
 *   2. filter_seeds with coordinates: every seed gives each label on the row of its first node (rows of dummy nodes are empty)
 *      the query positions [clipping, clipping + k - offset); labels covering fewer than min_exact_match x |query| positions go;
 *      a seed keeps the remaining labels of that row with the row's coordinates, each shifted by the seed's offset; seeds left
 *      without a label go; num_matching = get_num_char_matches_in_seeds of what is left (what the seeder left for a strand
 *      without seeds);
 *   3. the kept seeds in reversed order (chain_seeds reverses them; seed_index counts in that order), and per label of a seed one
 *      anchor per coordinate, at most max_num_seeds_per_locus of them from the largest down: (label, coordinate, clipping,
 *      clipping + length, chain_score = length, seed_index);
 *   4. the sort and the DP of mgx_chain_seeds (query_size = |query|, the gap cost tabulated on the host), without its limit of
 *      6144 anchors per list: lists are bounded by memory alone, a call by 2^31 - 17 (seed, label) pairs and as many anchors
 *      (more: MGX_ERR_UNSUPPORTED; run the batch in parts).
 * Every array is sized exactly (a size pass, a scan, a write pass); kernel launches, allocations and synchronising copies per
 * call do not depend on the number of reads, seeds or labels, and with MGX_CHAIN_TABLES_ON_DEVICE the only device-to-host
 * traffic is a handful of totals.  The arrays belong to the handle until its next batch call.  A query whose seeding ran out of
 * a per-read arena has status MGX_ERR_CAPACITY and two empty lists (no retry here; mgx_limits raises the arenas).  n = 0: empty
 * tables.  seqs / offsets as in mgx_align_batch. */
int mgx_seed_chainer_create(const mgx_graph *graph, const mgx_config *config, const mgx_limits *limits,
                            const struct mgx_annotation *annotation, mgx_aligner **out);
typedef struct mgx_chain_seed { uint32_t clipping, length, offset, n_nodes; uint64_t nodes_begin; } mgx_chain_seed;
typedef struct mgx_chain_tables {
    uint64_t n_queries;                 /* list 2q = query q, list 2q + 1 = its reverse complement */
    const uint64_t *seed_begin;         /* 2n + 1 */
    const mgx_chain_seed *seeds;        /* the seeds filter_seeds kept, in the order chain_seeds leaves them (reversed) */
    const uint64_t *nodes;              /* seed s: nodes[nodes_begin .. nodes_begin + n_nodes) */
    const uint64_t *num_matching;       /* 2n: filter_seeds' return value */
    const uint64_t *list_begin;         /* 2n + 1 */
    const mgx_chain_anchor *anchors;    /* sorted as the reference sorts, final chain_score, seed_index relative to seed_begin[list] */
    const uint32_t *backtrace;          /* relative to list_begin[list]; 0xFFFFFFFF: none */
    const int32_t *status;              /* n: MGX_OK, or MGX_ERR_CAPACITY from the seeding stage (lists empty; no retry here) */
} mgx_chain_tables;
#define MGX_CHAIN_TABLES_ON_DEVICE 1u   /* all arrays stay in device memory (pointers are device pointers), only sizes travel */
int mgx_chain_tables_batch(mgx_aligner *a, const char *seqs, const uint64_t *offsets, uint64_t n, int seqs_on_device,
                           uint32_t flags, mgx_chain_tables *out);
/* the last MGX_CHAIN_TABLES_ON_DEVICE result of the handle copied to host arrays (the handle's, until its next batch call) */
int mgx_chain_tables_fetch(mgx_aligner *a, mgx_chain_tables *out_host);
/* test hook, like its siblings: [kernel launches and device-library calls of the chain stage (the seeding stage's are not
 * counted), device buffers it took or grew, bytes host-to-device, bytes device-to-host] since the library was loaded */
void mgx_chain_tables_kernel_launch_counts(uint64_t *out4);

/* LabeledAligner<>(graph, config, annotator) (aligner_labeled.hpp:125-127; ctor aligner_labeled.cpp:450-466: DBGAligner's
 * clamps, then min / max_seed_length <= k): an aligner whose batches run label-aware — seeds filtered by label
 * (filter_seeds, aligner_labeled.cpp:612-721), every DP column carries the labels shared along its path
 * (LabeledExtender::call_outgoing / flush, :81-137,176-302), backtracking reports one alignment per label subset of the seed
 * (:304-448), the aggregator keeps num_alternative_paths alignments per label (aligner_aggregator.hpp:68-206).  Every
 * mgx_alignment of its results carries its labels (n_labels, labels_begin into mgx_results.labels, ascending).  Used with
 * mgx_align_batch / mgx_align_batch_device / mgx_fetch_results like any aligner; `annotation` must outlive it and live on
 * the graph's device, with at least as many rows as the graph has nodes (row = node - 1).
 * This round: BASIC-, PRIMARY- and CANONICAL-mode graphs (PRIMARY: through the CanonicalDBG wrapper, labels looked up by base
 * node; CANONICAL: by the k-mer's representative, the smaller BOSS index of the k-mer and its reverse complement — as
 * annotation_buffer.cpp:41-63 does), annotations without coordinates (ColumnCompressed), num_alternative_paths <= MGX_MAX_ALTERNATIVE_PATHS;
 * anything else: MGX_ERR_UNSUPPORTED.  A read whose label bookkeeping outgrows the arenas of a first run (64 labels with
 * alignments, 8 alignments per backtracking, ...) gets MGX_ERR_CAPACITY from mgx_align_batch_device; mgx_align_batch re-runs it
 * with the arenas doubled (up to 8 x) like any other capacity status (mgx_stats.n_capacity_retried).
 * One case the reference leaves UNDEFINED on CANONICAL-mode graphs: the reversed alignment that seeds a backward pass holds
 * reverse-complement nodes its AnnotationBuffer was never asked to fetch; set_seed / flush assert on them
 * (aligner_labeled.cpp:110,143-146) and a release build reads through a null pointer.  The library answers such a look-up
 * with the labels of the node's representative — what a fetch would have found; the oracle does the same and counts them
 * (orc_unfetched_label_lookups: 0 on the reference's own label tests, which is what pins this path; reads that do need
 * such a look-up agree between library and oracle but have no reference behaviour to agree with).
 * config->global_xdrop = 0 is accepted here (and only here): per-branch x-drop (aligner_extender_methods.cpp:429-441,511-536,
 * 577-603,635-663) — every child of a fork gets an x-drop cut-off of its own, max_nodes_per_seq_char counts a branch's depth and
 * ends that branch only, and a cell keeps an extension going only within rel_score_cutoff of the best score reached at its query
 * position (scores_reached_).  Such an aligner extends on builds of the two label-aware kernels with that rule compiled in
 * (MGX_KERNEL_LAB64_BX / MGX_KERNEL_GRP8_LAB_BX) and never on the lane-per-read kernels; the table of an extension is then no longer
 * bounded by max_nodes_per_seq_char x query length, so a read may outgrow max_columns and is re-run by the capacity retry.  The
 * reference sets this together with seed chaining for annotations with coordinates; chaining itself stays refused (above). */
int mgx_labeled_aligner_create(const mgx_graph *graph, const mgx_config *config, const mgx_limits *limits,
                               const mgx_annotation *annotation, mgx_aligner **out);
/* mgx_format_tsv for label-aware results: every alignment's fields are followed by its labels' names joined by ';'
 * (cli/align.cpp:274-281; label_names[j] = LabelEncoder::decode(j); a label without a name prints its number). */
size_t mgx_format_tsv_labeled(const mgx_results *res, uint64_t query_index, const char *header,
                              const char *query, size_t query_len, int32_t min_path_score,
                              const char *const *label_names, uint32_t n_label_names, char *buf, size_t buf_len);
/*
 * The TSV text of a whole batch, written on the device (csrc/tsv_format.hpp, csrc/mgx_format.hip).
 * After mgx_align_batch_device (or mgx_align_batch) on this handle: what format_alignment (cli/align.cpp:254-285) prints for
 * every query of the batch, byte for byte what mgx_format_tsv_labeled gives query by query.  headers: the concatenated header
 * bytes, header i = headers[header_offsets[i] .. header_offsets[i + 1]) (host arrays, n_queries + 1 offsets).  label_names /
 * n_label_names as in mgx_format_tsv_labeled (NULL / 0: numbers; only a label-aware aligner prints labels); the names are
 * uploaded with every call.  min_path_score is the aligner's config's.  The views are host memory owned by the handle and stay
 * valid until the next batch or format call on it.
 *   - Runs on the aligner's stream.  Device-to-host copies: the text, the n_queries + 1 offsets and 16 bytes of counters
 *     (the text's size, the number of capacity-status records); the result records and the stream do not travel.
 *   - Capacity statuses (the device records are pre-retry): those queries alone go through the retry mgx_fetch_results
 *     performs; their lines come from mgx_format_tsv_labeled on the retried results and stand at their place in the text.
 *     The query numbers and the reads of those queries travel in addition.  The text is complete or the call fails:
 *     MGX_ERR_CAPACITY, naming the first such query in mgx_last_error, with retry_capacity=0 or when the retry cures none.
 *   - post_chain_alignments: MGX_ERR_UNSUPPORTED (the chained alignments exist on the host only: mgx_fetch_results +
 *     mgx_format_tsv remain the path for that configuration).
 *   - The batch must still be the staged one (no mgx_map_batch / mgx_map_summary_batch on the handle in between), and with
 *     seqs_on_device != 0 the caller's seqs / offsets must stay valid until the call returns — as for mgx_fetch_results.
 */
typedef struct mgx_text {
    uint64_t n_queries;
    const char *text;            /* all lines, query order, no NUL */
    const uint64_t *line_begin;  /* n_queries + 1 byte offsets into text */
} mgx_text;
int mgx_format_tsv_batch(mgx_aligner *a, const char *headers, const uint64_t *header_offsets,
                         const char *const *label_names, uint32_t n_label_names, mgx_text *out);
/* Test hook: out4 = launches of the size kernel, launches of the write kernel, queries whose line was formatted on the host
 * (capacity retries), bytes copied device-to-host by mgx_format_tsv_batch — since the library was loaded. */
void mgx_format_kernel_launch_counts(uint64_t *out4);
/*
 * The text of `align --map` for a whole batch, written on the device (csrc/map_format.hpp, csrc/mgx_mapfmt.hip):
 * byte for byte what mgx_format_map gives query by query, for the batch mgx_map_summary_batch ran last on this handle, with that
 * call's map_length, n_queries and reads.  format: MGX_MAP_FMT_*; MGX_MAP_FMT_NODES needs a summary run with MGX_MAP_KEEP_NODES
 * (or _WANT_NODES).  headers / header_offsets: host arrays as for mgx_format_tsv_batch (n_queries + 1 offsets; header bytes are
 * copied as they are, up to the offset — no NUL ends one).  Query bytes are printed as they came: nothing is normalised.
 * discovery_fraction: as for mgx_map_present; the host tabulates that function's double expressions per k-mer count and the
 * kernels compare integers, so presence is mgx_map_present's for every query.
 * The views are pinned host memory owned by the handle, valid until the next batch or format call on it.  With seqs_on_device
 * != 0 in the summary call the caller's seqs / offsets must still be valid.
 *   - Device-to-host copies: the text, the n_queries + 1 offsets and 16 bytes of counters (the text's size and a reserved
 *     word, in one copy).  Counts and nodes do not travel.
 *   - MGX_ERR_INVALID, named in mgx_last_error: a null argument; an unknown format; no summary batch staged — never run, or
 *     mgx_align_batch_device / mgx_map_batch (any other batch call) ran since; MGX_MAP_FMT_NODES when the summary kept no nodes.
 */
int mgx_format_map_batch(mgx_aligner *a, const char *headers, const uint64_t *header_offsets, int format,
                         double discovery_fraction, mgx_text *out);
/* Test hook: out4 = launches of k_mapfmt_size, launches of k_mapfmt_write, bytes copied device-to-host, bytes copied
 * host-to-device (headers, header offsets, the threshold table) by mgx_format_map_batch — since the library was loaded. */
void mgx_format_map_kernel_launch_counts(uint64_t *out4);
/*
 * The `align --json` text of a range of a batch, written on the device (csrc/json_format.hpp, csrc/mgx_jsonfmt.hip).
 * After mgx_align_batch_device (or mgx_align_batch) on this handle, under the rules of mgx_format_tsv_batch (the batch must still
 * be the staged one; with seqs_on_device != 0 the caller's seqs / offsets must stay valid): the lines of queries first ..
 * first + n of the staged batch, byte for byte what mgx_format_json gives for those queries in order with k = mgx_graph_k of the
 * aligner's graph.  A query prints one line per alignment, a query without alignments the {"name":...,"sequence":""} line;
 * out->line_begin[i] .. line_begin[i + 1] covers all lines of query first + i, out->n_queries = n.  headers / header_offsets: host
 * arrays FOR THE RANGE, n + 1 offsets (header of query first + i = headers[header_offsets[i] .. header_offsets[i + 1]); no NUL ends
 * one).  The range exists because JSON text is large (one mapping object per path node: 11.5 KB per 150-bp read measured on the
 * benchmark graph, against ~350 bytes of TSV): a caller bounds
 * the text of one call by formatting a staged batch in slices, and the slices' texts concatenated are the whole batch's.
 * n == 0: MGX_OK, an empty text.  The views are pinned host memory owned by the handle, valid until the next batch or format call.
 *   - Runs on the aligner's stream.  Device-to-host copies: the text, the n + 1 offsets and 16 bytes of counters; the result
 *     records and the stream do not travel.
 *   - Capacity statuses: as in mgx_format_tsv_batch — those queries alone are aligned again, their lines come from mgx_format_json
 *     on the retried results and stand at their place; MGX_ERR_CAPACITY, naming the first such query, with retry_capacity=0 or
 *     when the retry cures none.
 *   - post_chain_alignments: MGX_ERR_UNSUPPORTED, naming post_chain_alignments (the reference throws "JSON output for chains not
 *     supported").  A label-aware aligner is accepted: JSON carries no labels.
 *   - MGX_ERR_INVALID, named in mgx_last_error: a null argument; first + n beyond the staged batch; no alignment batch staged
 *     (never run, or a map / summary call ran since).
 *   - "Byte for byte" holds for records as the extension kernels write them (csrc/json_format.hpp lists what the lanes take for
 *     granted: offset < k; no insertion / clip run directly behind another one while nodes are left; num_matches <= the aligned
 *     length; n_nodes no more than the CIGAR's node-consuming positions pay for).  The call formats the handle's own batch, so a
 *     caller cannot hand it any other kind of record.
 *   - MGX_ERR_OOM when the text buffer cannot be allocated; the message says how many bytes the range needs, so that the
 *     caller can take a smaller range.
 */
int mgx_format_json_batch(mgx_aligner *a, const char *headers, const uint64_t *header_offsets,
                          uint64_t first, uint64_t n, mgx_text *out);
/* Test hook: out4 = launches of k_jsonfmt_size, launches of k_jsonfmt_write, queries whose lines were formatted on the host
 * (capacity retries), bytes copied device-to-host by mgx_format_json_batch — since the library was loaded. */
void mgx_format_json_kernel_launch_counts(uint64_t *out4);

/* ---- FASTA / FASTQ text to read batches, parsed on the device --------------------------------------------
 * mgx_parse_reads turns the bytes of a FASTA / FASTQ file (plain text: gzip stays with the caller) into the arrays the calls
 * above take, without a per-record step on the host: `seqs` / `offsets` in DEVICE memory are the arguments of
 * mgx_align_batch_device(..., seqs_on_device = 1); `names` / `name_offsets` in HOST memory are the arguments of
 * mgx_format_tsv_batch; `host_offsets` is a host copy of `offsets` (batching by bases, cli/align.cpp:429-438).  The sequences
 * themselves do not travel back (mgx_read_parser_fetch copies them for who wants them).
 *
 * Grammar: kseq's kseq_read restricted to files where it is unambiguous; anything outside it is MGX_ERR_INVALID — never parsed
 * differently — with the byte position of the offending line in mgx_last_error(), and `out` untouched.
 *   - format: the first byte of the chunk's first non-empty line: '>' FASTA, '@' FASTQ (flags = MGX_READS_FASTA / MGX_READS_FASTQ
 *     forces one; a caller that feeds chunks passes the first chunk's out->format for the later ones).
 *   - name: the bytes behind the marker up to the first isspace() byte or the end of the line; the comment is dropped; empty
 *     names are kept.  A line excludes its '\n' and a '\r' directly in front of it.
 *   - FASTA: every line up to the next header line is a sequence line, copied verbatim; empty lines add nothing; a sequence line
 *     that begins with '@' or '+' is refused.
 *   - FASTQ: records are strictly four lines counted from the start of the chunk, empty lines count: line 0 begins with '@', line 2
 *     with '+', line 1 with none of "@+>", lines 1 and 3 have the same length (multi-line FASTQ is refused).  Empty lines behind
 *     the last record are ignored.
 *   - final == 0: only complete records are consumed (FASTQ: four lines, the fourth ended by '\n'; FASTA: another header line
 *     follows); out->consumed = their bytes, where the caller's next chunk starts; n_records == 0 with MGX_OK asks for a longer
 *     chunk.  final != 0: an unterminated last line ends at the end of the buffer and consumed = n_bytes.
 *   - chunks of 2^32 - 1 bytes or more: MGX_ERR_INVALID.  Offsets are 64-bit.
 * The views are owned by the handle: valid until its next parse or its destruction; the device arrays must not be in use by
 * another stream's work when the next parse starts (mgx_fetch_results / mgx_format_tsv_batch have synchronised by then).
 * A parse that fails or is refused ends the previous parse's views all the same (their buffers may have been reused): the handle
 * then holds no records, mgx_read_parser_slice accepts only the empty range and mgx_read_parser_fetch copies nothing.
 * text_on_device != 0: the text is read by kernels on the parser's own non-blocking stream, which waits for no other stream —
 * the work that produces the text must have completed (a stream or device synchronise by the caller) before the call.
 * `seqs` has 16 bytes of room behind the last sequence, like the staged copy of host reads.
 * A sub-batch (records first .. first + n): mgx_read_parser_slice returns the device pointers to pass on — offsets that start at
 * 0, as the aligner's kernels expect; valid until the next slice or parse.  Names of a sub-batch: names + name_offsets[first]
 * with the offsets rebased by the caller. */
#define MGX_READS_FASTA 1u
#define MGX_READS_FASTQ 2u
typedef struct mgx_read_parser mgx_read_parser;
typedef struct mgx_reads {
    uint64_t n_records, consumed;
    uint32_t format;                /* MGX_READS_FASTA / MGX_READS_FASTQ; 0: no non-empty line seen */
    const char *seqs;               /* DEVICE */
    const uint64_t *offsets;        /* DEVICE, n_records + 1 */
    const uint64_t *host_offsets;   /* HOST copy of offsets */
    const char *names;              /* HOST */
    const uint64_t *name_offsets;   /* HOST, n_records + 1 */
} mgx_reads;
int mgx_read_parser_create(int device, mgx_read_parser **out);
void mgx_read_parser_destroy(mgx_read_parser *p);
int mgx_parse_reads(mgx_read_parser *p, const char *text, uint64_t n_bytes, int text_on_device, int final, uint32_t flags,
                    mgx_reads *out);
int mgx_read_parser_slice(mgx_read_parser *p, uint64_t first, uint64_t n, const char **seqs, const uint64_t **offsets);
/* device -> host copy of the last parse: seqs_out takes host_offsets[n_records] bytes, offsets_out n_records + 1 entries */
int mgx_read_parser_fetch(mgx_read_parser *p, char *seqs_out, uint64_t *offsets_out);
/* Test hook: out4 = launches of the line-pass kernels, launches of the copy-pass kernels, bytes copied host-to-device, bytes
 * copied device-to-host by the parser — since the library was loaded. */
void mgx_parse_kernel_launch_counts(uint64_t *out4);
/* Page-locked host memory for the text handed to mgx_parse_reads (a copy from pageable memory is staged by the runtime and runs at
 * a fraction of the link's rate).  NULL on failure (mgx_last_error). */
void *mgx_pinned_alloc(size_t bytes);
void mgx_pinned_free(void *p);

/* mgx_results_from_raw for the records of a label-aware aligner (labeled != 0: every alignment's arrays are followed by
 * its label list in the stream). */
int mgx_results_from_raw_labeled(const void *headers, uint64_t n_queries, const uint32_t *stream, uint64_t stream_words,
                                 int labeled, mgx_raw_store **store, mgx_results *out);

/*
 * Files: the graph and annotation files the reference writes, read on the host and handed to
 * mgx_graph_create / mgx_annotation_create_sparse.  What a stand-alone caller (host/mgx_align) needs in place of
 * DBGSuccinct::load (dbg_succinct.cpp:690-785 over BOSS::load, boss.cpp:338-394) and ColumnCompressed::load / merge_load
 * (annotate_column_compressed.cpp:436-481,493-640); inside MetaGraph the adapter takes both from the loaded objects
 * (INTEGRATION.md 2).  Read: BOSS states SMALL, STAT and FAST (DYN: MGX_ERR_UNSUPPORTED), any alphabet in
 * mgx_boss_file_read (the device index itself is DNA only); columns stored as sd_vector, bit_vector_stat or rrr_vector<63>
 * (bit_vector_smart writes the first two), both label-encoder formats.  The `.edgemask` next
 * to a `.dbg`: mgx_edgemask_read.  Which layouts are pinned on reference-written files:
 * csrc/boss_files.hpp.  Malformed file: MGX_ERR_INVALID with the field named in mgx_last_error; the *_read calls need no GPU.
 */
typedef struct mgx_boss_file {
    uint32_t k;              /* DBG k (BOSS k + 1) */
    uint32_t sigma;          /* alphabet size incl. '$' (F's length): 5 = DNA */
    uint32_t mode;           /* MGX_MODE_* as stored behind the BOSS table (dbg_succinct.cpp:701) */
    uint32_t state;          /* BOSS::State of the file (boss.hpp:325): 1 SMALL, 3 STAT, 4 FAST */
    uint64_t n_edges;
    const uint64_t *F;       /* sigma entries */
    const uint8_t *W;        /* n_edges + 1 bytes, the layout of mgx_boss_view */
    const uint8_t *last;
    void *owner;             /* private */
} mgx_boss_file;
int mgx_boss_file_read(const char *path, mgx_boss_file *out);
void mgx_boss_file_free(mgx_boss_file *f);
/* The `.edgemask` file next to a `.dbg` (dbg_succinct.cpp:719-752) as mgx_boss_view.valid bytes: valid_out has n_edges + 1
 * entries; `state` = mgx_boss_file.state of the graph (it decides the mask's vector type).  mgx_graph_load_dbg does not apply
 * it — `metagraph align` resets the mask after loading (cli/align.cpp:337-339); a caller that keeps the mask builds the view
 * from mgx_boss_file_read + this. */
int mgx_edgemask_read(const char *path, uint32_t state, uint64_t n_edges, uint8_t *valid_out);
/* mgx_boss_file_read + mgx_graph_create: DBGSuccinct::load for the device */
int mgx_graph_load_dbg(const char *path, int device, mgx_graph **out);
/* mgx_graph_load_dbg with the payloads decoded by kernels: same contract, same graph, same error codes, and a
 * malformed file's message names the same field.  The host reads the file and walks the container headers (sizes, widths, the
 * tree's <= 511 nodes, F, k, state, mode); the rrr_vector<63> blocks, the wavelet tree of W, the int_vector of FAST-state graphs
 * and `last` (rrr, bit_vector_stat or sd_vector) go to the device as they stand in the file and are decoded there into the
 * W / last byte arrays, which mgx_graph_create takes with on_device = 1 and which are released on return.  Nothing of W or last
 * is copied back to the host.  Refused as by the host reader: DYN state, bit_vector_il.  (A wavelet tree whose node table is
 * not a tree, which no writer produces, is decoded by the host reader and uploaded.) */
int mgx_graph_load_dbg_device(const char *path, int device, mgx_graph **out);
/* Test hook: the same kernels, then W / last copied back into a host-owned mgx_boss_file (mgx_boss_file_free) — what
 * mgx_boss_file_read returns, byte for byte.  Like it, and unlike the two load calls, it accepts any alphabet. */
int mgx_boss_file_decode_device(const char *path, int device, mgx_boss_file *out);
/* Test hook: out4 = launches of the rrr kernels, launches of the wavelet-tree / unpack / last kernels, bytes copied
 * host-to-device, bytes copied device-to-host by the two calls above — since the library was loaded. */
void mgx_dbg_decode_kernel_launch_counts(uint64_t *out4);

typedef struct mgx_column_file mgx_column_file;
/* One or several `.column.annodbg` files over the same rows, their columns side by side in argument order (merge_load;
 * a label occurring in two files: MGX_ERR_UNSUPPORTED). */
int mgx_column_file_read(const char *const *paths, uint32_t n_paths, mgx_column_file **out);
void mgx_column_file_free(mgx_column_file *f);
uint64_t mgx_column_file_num_rows(const mgx_column_file *f);
uint32_t mgx_column_file_num_labels(const mgx_column_file *f);
const char *mgx_column_file_label(const mgx_column_file *f, uint32_t j);      /* LabelEncoder::decode(j) */
const uint64_t *mgx_column_file_col_begin(const mgx_column_file *f);          /* num_labels + 1 entries */
const uint64_t *mgx_column_file_rows(const mgx_column_file *f);               /* the arguments of mgx_annotation_create_sparse */
/* An object of mgx_column_coord_file_read: mgx_annotation_set_coordinates is called with its coordinates as well. */
int mgx_annotation_create_from_file(const mgx_column_file *f, int device, mgx_annotation **out);
/* Column annotations with k-mer coordinates (annot::ColumnCoordAnnotator), in either of the two forms the reference writes:
 *   (a) `X.column.annodbg` + the side file `X.column.annodbg.coords` next to it (`metagraph annotate --coordinates`; the side file:
 *       per column a bit_vector_smart of delimiters and an sdsl::int_vector<> of values, TupleCSCMatrix::serialize_tuples); several
 *       such pairs side by side as in mgx_column_file_read, a label in two files: MGX_ERR_UNSUPPORTED; a missing side file:
 *       MGX_ERR_INVALID naming its path;
 *   (b) one `X.column_coord.annodbg` (a path with that ending; it must be the only path): label encoder, ColumnMajor (bit_vector_sd
 *       columns without a representation code; the row count is the columns' common size), then the same tuple section.
 * Checked per column, in this order: the delimiter vector (values + set rows + 1 bits, set rows + 1 of them set, the first and the
 * last among them), every value below 2^63, every tuple ascending; then that no bytes follow the last column.  Each fault:
 * MGX_ERR_INVALID with the field named in mgx_last_error.  The object answers the accessors above and the two below: coords of
 * matrix entry x (rows[x]) = coords[coord_begin[x] .. coord_begin[x + 1]), the arguments of mgx_annotation_set_coordinates.
 * Both return NULL on an object of mgx_column_file_read (which ignores side files) and on a names_out. */
int mgx_column_coord_file_read(const char *const *paths, uint32_t n_paths, mgx_column_file **out);
const uint64_t *mgx_column_file_coord_begin(const mgx_column_file *f);        /* col_begin[num_labels] + 1 entries */
const int64_t *mgx_column_file_coords(const mgx_column_file *f);
/* mgx_column_file_read + mgx_annotation_create_from_file with the columns decoded by kernels: same contract, the
 * same annotation (mgx_annotation_get_rows answers alike), the same error codes and messages for the same files.  The host reads
 * the files and walks their headers (num_rows, the label encoder, per column the representation code and the container headers);
 * the payloads of all columns (sd_vector low / high, bit_vector_stat bits, rrr_vector<63> bt / btnr) go to the device as they
 * stand in the files, in one copy, and are decoded there into the columns' set rows, which mgx_annotation_create_sparse takes
 * with on_device = 1.  The number of kernel launches and device allocations does not depend on the number of columns, and no row
 * index is copied to the host: n_labels counts, the error record and nothing else.  Whenever the header walk or a kernel's check
 * finds fault with a file, the host reader is run on it and ITS code and message are returned (bit_vector_il: MGX_ERR_UNSUPPORTED).
 * names_out (may be NULL) receives a mgx_column_file with num_rows, num_labels, the labels and col_begin: its rows live on the
 * device only, so mgx_column_file_rows returns NULL on it and mgx_annotation_create_from_file refuses it (MGX_ERR_INVALID); free
 * it with mgx_column_file_free. */
int mgx_annotation_load_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out);
/* Test hook: the same kernels, then the rows copied back into a host-owned mgx_column_file — what mgx_column_file_read returns,
 * entry for entry. */
int mgx_column_file_decode_device(const char *const *paths, uint32_t n_paths, int device, mgx_column_file **out);
/* mgx_column_coord_file_read + mgx_annotation_create_from_file with everything decoded by kernels, under the contract
 * of mgx_annotation_load_columns_device: the delimiter vectors (in whichever of sd / inverted sd / stat / rrr they are stored) and
 * the values' raw words go up with the binary columns in the same single copy; kernels decode the delimiters to bit maps, rank
 * them into coord_begin, unpack the values (widths 1 to 64) into coords, and mgx_annotation_set_coordinates_device transposes them.
 * No row index and no coordinate is copied to the host; launches and allocations do not depend on the number of columns; on any
 * fault the host reader runs on the same files and ITS code and message are returned. */
int mgx_annotation_load_coord_columns_device(const char *const *paths, uint32_t n_paths, int device, mgx_annotation **out, mgx_column_file **names_out);
/* Test hook: the same kernels, then rows, coord_begin and coords copied back into a host-owned mgx_column_file — what
 * mgx_column_coord_file_read returns, entry for entry. */
int mgx_column_coord_file_decode_device(const char *const *paths, uint32_t n_paths, int device, mgx_column_file **out);
/* Test hook: out4 = kernel launches, device allocations, bytes copied host-to-device, bytes copied device-to-host by the four calls
 * above — since the library was loaded (the copies inside mgx_annotation_create_sparse / _set_coordinates_device are not counted). */
void mgx_column_decode_kernel_launch_counts(uint64_t *out4);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H_ */
