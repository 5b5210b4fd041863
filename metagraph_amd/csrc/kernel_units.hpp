// kernel_units.hpp — what the translation units of libmgx.so call in one another: the launchers and build constants of the
// kernel units (the host units launch them: the align pipeline in mgx.hip, mgx_map.hip, mgx_results.hip, mgx_text.hip) and the
// library-internal accessors of mgx_annot.hip.  Declarations only.  Every unit that calls or defines one of these symbols includes
// this file, so that a signature which drifts on one side is a compile error instead of a call through a wrong prototype.
// (What the host units share among themselves — handles, error message, block pool — is host_state.hpp.)
#pragma once
#include <stddef.h>
#include <stdint.h>

// The launchers take their parameter block as `const void *` (every kernel unit instantiates the shared sources in a namespace of
// its own, so the struct types differ by name from unit to unit).  The blocks are the same plain data everywhere: each unit
// asserts the size of its own instantiation against these, next to the cast.
constexpr size_t MGX_ALIGN_PARAMS_BYTES = 728;          // sizeof(AlignParams), align_types.hpp
constexpr size_t MGX_LANE_PARAMS_BYTES = 864;          // sizeof(LaneParams), lane_types.hpp
constexpr size_t MGX_SEED_LANE_PARAMS_BYTES = 824;      // sizeof(SeedLaneParams), seed_lane.hpp
constexpr size_t MGX_DEV_GRAPH_BYTES = 160;             // sizeof(DevGraph), dev_graph.hpp
constexpr size_t MGX_FORMAT_ARGS_BYTES = 128;           // sizeof(TfBatch), tsv_format.hpp
constexpr size_t MGX_PARSE_ARGS_BYTES = 144;            // sizeof(RpChunk), reads_parse.hpp
constexpr size_t MGX_MAPFMT_ARGS_BYTES = 120;           // sizeof(MfBatch), map_format.hpp
constexpr size_t MGX_JSONFMT_ARGS_BYTES = 120;          // sizeof(JfBatch), json_format.hpp
constexpr size_t MGX_DECODE_ARGS_BYTES = 104;           // sizeof(RdBatch), results_decode.hpp
constexpr unsigned MGX_SEED_STATIC_LDS_BYTES = 1792;    // static LDS of k_align<PH_SEED>, either build of mgx_seed.hip

#ifndef MGX_SEL_ANCHOR_MAX
#define MGX_SEL_ANCHOR_MAX 8192      // entries of the select-anchor table mgx_graph.hip builds (32 KB of LDS per workgroup of k_map_pipe, mgx_map.hip)
#endif

struct mgx_annotation;

extern "C" {

// mgx.hip: the thread-local message behind mgx_last_error(), for the other units' failures
void mgx_set_last_error(const char *msg);

// mgx_grp.hip (MGX_GROUP = 8), four builds whose names differ by a suffix: the product, `_prim` (the product with the CanonicalDBG
// branches: PRIMARY graphs), `_alt` (room for MGX_MAX_ALTERNATIVE_PATHS alignments per query, either kind of graph) and `_lab`
// (the label-aware extender).  params: AlignParams (host memory); n_groups = arena slices; lds_bytes = dynamic LDS per group;
// phase = PH_EXTEND (the only half instantiated for sub-wave groups).
#define MGX_DECLARE_GRP8_BUILD(sfx)                                                                                          \
    int mgx_launch_align_grp8##sfx(const void *params, uint32_t n_groups, uint32_t lds_bytes, int phase, void *stream);      \
    int mgx_grp_waves_per_simd8##sfx(void);                                                                                  \
    unsigned mgx_grp_static_lds8##sfx(void);
MGX_DECLARE_GRP8_BUILD()
MGX_DECLARE_GRP8_BUILD(_prim)
MGX_DECLARE_GRP8_BUILD(_alt)
MGX_DECLARE_GRP8_BUILD(_lab)
MGX_DECLARE_GRP8_BUILD(_labx)        // `_lab` with per-branch x-drop compiled in (-DMGX_BRANCH_XDROP=1): aligners with global_xdrop = 0
#undef MGX_DECLARE_GRP8_BUILD
int mgx_grp_max_alt8_lab(void);
int mgx_grp_max_alt8_labx(void);

// mgx_ext64.hip / mgx_lab64.hip: the extension half with all 64 lanes on one read, plain and label-aware.  params: AlignParams
// (host memory); blocks = wavefronts; lds_bytes = dynamic LDS per wavefront.
int mgx_launch_ext64(const void *params, uint32_t blocks, uint32_t lds_bytes, void *stream);
unsigned mgx_ext64_static_lds(void);
int mgx_ext64_waves_per_simd(void);
int mgx_launch_lab64(const void *params, uint32_t blocks, uint32_t lds_bytes, void *stream);
unsigned mgx_lab64_static_lds(void);
int mgx_lab64_waves_per_simd(void);
int mgx_lab64_max_alt(void);
// ... and the build of mgx_lab64.hip with per-branch x-drop compiled in (-DMGX_BRANCH_XDROP=1): aligners with global_xdrop = 0
int mgx_launch_lab64x(const void *params, uint32_t blocks, uint32_t lds_bytes, void *stream);
unsigned mgx_lab64x_static_lds(void);
int mgx_lab64x_waves_per_simd(void);
int mgx_lab64x_max_alt(void);

// mgx_seed.hip: the wave-per-read seeding kernel (seed_kernel.hpp), two builds: the plain one and `_primary`
// (-DMGX_WITH_PRIMARY=1: the CanonicalDBG branches, PRIMARY graphs).  params: AlignParams (host memory); blocks = wavefronts;
// wps8 selects the 8-waves-per-SIMD instantiation.  static_lds: control block + sdust interval lists, rounded up to 128.
// (The figure is the same in both builds, which each assert it: the host sizes the dynamic LDS of either from the plain one.)
// mgx_seed_load: the plain build's code object onto the current device, without a launch (see load_map_kernels, host_state.hpp).
int mgx_launch_seed(const void *params, uint32_t blocks, uint32_t lds_bytes, int wps8, void *stream);
int mgx_launch_seed_primary(const void *params, uint32_t blocks, uint32_t lds_bytes, int wps8, void *stream);
unsigned mgx_seed_static_lds(void);
int mgx_seed_load(void);

// mgx_lane.hip: the lane-per-read kernel.  d_params: LaneParams in DEVICE memory; blocks = resident wavefronts
int mgx_launch_lane(const void *d_params, uint32_t blocks, void *stream);
int mgx_launch_lane_exact(const void *d_params, uint32_t blocks, int labeled, void *stream);    // k_lane_exact / k_lane_exact_labeled, before the work sort when LaneParams::exact
int mgx_launch_lane_exact_sub(const void *d_params, uint32_t blocks, int labeled, void *stream); // k_lane_exact_sub / k_lane_exact_sub_labeled, behind those when LaneParams::exact >= 3
int mgx_lane_waves_per_simd(void);

// mgx_seedlane.hip: the lane-per-read seeder.  d_params: SeedLaneParams in DEVICE memory; long_reads: the build for reads of
// more than SL_SHORT_L characters
int mgx_launch_seed_lane(const void *d_params, uint32_t blocks, int long_reads, void *stream);
int mgx_seed_lane_waves_per_simd(void);

// mgx_mapsum.hip: the per-read counts of `align --map` (map_summary.hpp).  counts: n_reads records of 12 bytes (mgx_map_counts);
// out_nodes: the merged node array or null; sorted: the long form's scratch (a word per k-mer of the batch); long_form selects
// the build for reads of more than mgx_map_summary_short_max() k-mers — each launch takes the reads of its form only.
// mgx_launch_map_subk: nodes[node_begin[r] + i] = the node of window i (map_length characters) of read r; dev_graph: a DevGraph.
int mgx_launch_map_summary(const uint64_t *node_begin, const uint32_t *fwd, const uint32_t *rc, uint32_t *sorted, void *counts,
                           uint64_t *out_nodes, const uint64_t *valid, uint64_t n_reads, uint32_t n_edges, int mode, int long_form,
                           void *stream);
int mgx_launch_map_subk(const void *dev_graph, const char *seqs, const uint64_t *offsets, const uint64_t *node_begin, uint32_t *nodes,
                        uint64_t n_reads, uint32_t map_length, void *stream);
uint32_t mgx_map_summary_short_max(void);

// mgx_format.hip: the TSV text of a batch (tsv_format.hpp).  args: a TfBatch (host memory).  size: line_len[q] for every query, and
// the capacity-status queries into cap_list / cap_count; write: the lines at text + line_begin[q]; patch: line_len[queries[i]] =
// lens[i] for the m lines the host formatted (device arrays).
int mgx_launch_format_size(const void *args, void *stream);
int mgx_launch_format_write(const void *args, void *stream);
int mgx_launch_format_patch(uint64_t *line_len, const uint32_t *queries, const uint64_t *lens, uint32_t m, void *stream);

// mgx_mapfmt.hip: the text of `align --map` for a batch (map_format.hpp).  args: an MfBatch (host memory).  size: line_len[q] for
// every query; write: the text at text + line_begin[q].
int mgx_launch_mapfmt_size(const void *args, void *stream);
int mgx_launch_mapfmt_write(const void *args, void *stream);

// mgx_jsonfmt.hip: the text of `align --json` for a range of a batch (json_format.hpp).  args: a JfBatch (host memory).  size:
// line_len[i] for every query of the range, and its capacity-status queries into cap_list / cap_count; write: the lines at
// text + line_begin[i].  (The lengths of host-formatted lines are patched in by mgx_launch_format_patch.)
int mgx_launch_jsonfmt_size(const void *args, void *stream);
int mgx_launch_jsonfmt_write(const void *args, void *stream);

// mgx_decode.hip: the results of a batch in the layout of mgx_results (results_decode.hpp).  args: an RdBatch (host memory).  size:
// counts[x * stride + q] for the five arrays x and every query q, and zeros at q = n_queries; write: status[q] and the alignments,
// nodes, CIGAR runs, path characters and labels of every query at begins[x * stride + q].
int mgx_launch_decode_size(const void *args, void *stream);
int mgx_launch_decode_write(const void *args, void *stream);

// mgx_parse.hip: FASTA / FASTQ text to read batches (reads_parse.hpp).  args: an RpChunk (host memory).  count: the '\n' mask and
// count of every 64-byte span; table: line_begin[] from the masks and the scanned counts; classify: what every line adds (items);
// records: offsets[] / name_offsets[] and the counters from the scanned items; copy: the sequence bytes, or (names != 0) the names.
int mgx_launch_parse_count(const void *args, void *stream);
int mgx_launch_parse_table(const void *args, void *stream);
int mgx_launch_parse_classify(const void *args, void *stream);
int mgx_launch_parse_records(const void *args, void *stream);
int mgx_launch_parse_copy(const void *args, int names, void *stream);

// mgx_annot.hip: the matrix as the label-aware extension kernels read it (AlignParams::anno_*), and the annotation's
// process-unique id
void mgx_annotation_device_view(const mgx_annotation *a, int *device, uint64_t *n_rows, const uint64_t **head,
                                const uint32_t **count, const uint32_t **more);
uint64_t mgx_annotation_uid(const mgx_annotation *a);
// ... and its row-major k-mer coordinates (mgx_chaintab.hip): the labels of row r are entries row_entry[r] .. row_entry[r + 1) in the
// order of its label list, entry e has the ascending coordinates coords[coord_off[e] .. coord_off[e + 1])
void mgx_annotation_coord_view(const mgx_annotation *a, const uint64_t **row_entry, const uint64_t **coord_off, const int64_t **coords);

}  // extern "C"
