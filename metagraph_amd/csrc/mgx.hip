// mgx.hip — libmgx.so's host driver: configuration, the aligner's lifecycle and options, the align pipeline (run_align: seeding,
// the work sort, extension) behind mgx_align_batch_device, statistics and streams.  The kernels live in units of their own
// (kernel_units.hpp); the graph, the mapping stage, the results and the output text are mgx_graph.hip, mgx_map.hip,
// mgx_results.hip and mgx_text.hip (host_state.hpp).  Plain C++ around the HIP runtime; there is no CPU execution path for the aligner.
#include <hip/hip_runtime.h>
#include "pack_swar.hpp"
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <cstdarg>
#include <memory>

#define MGX_NO_EXTEND 1      // of the device headers this unit wants the host-callable sizes (arena_bytes, fast_lds_bytes, ...) only
#include "seed_kernel.hpp"   // (MGX_SEED_WPS, MGX_ALIGN_WAVES_PER_SIMD; align_core.hpp)
#include "host_state.hpp"
#include "lane_types.hpp"
#include "seed_lane.hpp"
#include "kernel_units.hpp"

using namespace mgx;
static_assert(sizeof(AlignParams) == MGX_ALIGN_PARAMS_BYTES && sizeof(LaneParams) == MGX_LANE_PARAMS_BYTES
              && sizeof(SeedLaneParams) == MGX_SEED_LANE_PARAMS_BYTES, "a parameter block differs from what the kernel units take");

static thread_local std::string g_err;      // mgx_last_error()
DevPool g_pool;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int hip_fail(hipError_t e, const char *expr, const char *file, int line) {
    return fail(e == hipErrorOutOfMemory ? MGX_ERR_OOM : MGX_ERR_NO_DEVICE, "%s: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
}

// the reads' indices for the work sort (sort_by_work, extend_multi_pass)
__global__ void k_iota(uint32_t *v, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

hipError_t load_sort_kernels() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_iota));
}

int exclusive_sum(mgx_aligner *A, uint64_t *in, uint64_t *out, uint64_t n) {
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, out, (int)n, A->hstream));
    if (int rc = A->scan_tmp.ensure(tmp_bytes + 16)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A->scan_tmp.p, tmp_bytes, in, out, (int)n, A->hstream));
    return MGX_OK;
}

// The pipeline run_align launches ("split8", the only one): seeding — the lane-per-read seeder, then one wavefront per read
// (k_align<PH_SEED>) on what it left —, a radix sort of the reads by predicted extension work, extension — the lane-per-read
// kernel, then 8-lane groups (8 reads per wavefront, mgx_grp.hip) or one read per wavefront on what it left.

// launches of the counted extension kernels since the library was loaded (mgx_kernel_launch_counts; bit order of MGX_KERNEL_*)
enum LaunchCounter { CNT_NONE = -1, CNT_GRP8 = 0, CNT_GRP8_PRIM, CNT_GRP8_ALT, CNT_EXT64, CNT_LANE, CNT_N };
static std::atomic<uint64_t> g_kernel_launches[CNT_N];

// The builds of the extension kernel (kernel_units.hpp).  Slot sizing and the launch read the same row.
struct ExtBuild {
    int (*launch_grp)(const void *params, uint32_t n_groups, uint32_t lds_bytes, int phase, void *stream);     // 8 reads per wavefront ...
    int (*launch_64)(const void *params, uint32_t blocks, uint32_t lds_bytes, void *stream);                   // ... or one (the other is null)
    int (*waves_per_simd)(void);
    unsigned (*static_lds)(void);
    uint64_t kernel_bit;              // MGX_KERNEL_*
    LaunchCounter counter;            // its entry of g_kernel_launches (the label-aware builds are not counted)
};
enum ExtBuildId { EXT_GRP8, EXT_GRP8_PRIM, EXT_GRP8_ALT, EXT_GRP8_LAB, EXT_EXT64, EXT_LAB64, EXT_GRP8_LAB_BX, EXT_LAB64_BX };
static const ExtBuild g_ext_builds[] = {
    { mgx_launch_align_grp8, nullptr, mgx_grp_waves_per_simd8, mgx_grp_static_lds8, MGX_KERNEL_GRP8, CNT_GRP8 },
    { mgx_launch_align_grp8_prim, nullptr, mgx_grp_waves_per_simd8_prim, mgx_grp_static_lds8_prim, MGX_KERNEL_GRP8_PRIM, CNT_GRP8_PRIM },
    { mgx_launch_align_grp8_alt, nullptr, mgx_grp_waves_per_simd8_alt, mgx_grp_static_lds8_alt, MGX_KERNEL_GRP8_ALT, CNT_GRP8_ALT },
    { mgx_launch_align_grp8_lab, nullptr, mgx_grp_waves_per_simd8_lab, mgx_grp_static_lds8_lab, MGX_KERNEL_GRP8_LAB, CNT_NONE },
    { nullptr, mgx_launch_ext64, mgx_ext64_waves_per_simd, mgx_ext64_static_lds, MGX_KERNEL_EXT64, CNT_EXT64 },
    { nullptr, mgx_launch_lab64, mgx_lab64_waves_per_simd, mgx_lab64_static_lds, MGX_KERNEL_LAB64, CNT_NONE },
    // the label-aware builds with per-branch x-drop: what an aligner with global_xdrop = 0 launches instead of the two above
    { mgx_launch_align_grp8_labx, nullptr, mgx_grp_waves_per_simd8_labx, mgx_grp_static_lds8_labx, MGX_KERNEL_GRP8_LAB_BX, CNT_NONE },
    { nullptr, mgx_launch_lab64x, mgx_lab64x_waves_per_simd, mgx_lab64x_static_lds, MGX_KERNEL_LAB64_BX, CNT_NONE },
};
static uint32_t waves_per_cu(const ExtBuild &b) { return 4u * (uint32_t)b.waves_per_simd(); }
// The 8-lane-group build a configuration extends on: the label-aware one; else the one with room for alternative paths
// (either kind of graph); else, on PRIMARY graphs, the product with the CanonicalDBG branches; else the product.
static const ExtBuild &group_build(bool labeled, bool primary, uint64_t agg_cap, bool branch_xdrop) {
    return g_ext_builds[labeled ? (branch_xdrop ? EXT_GRP8_LAB_BX : EXT_GRP8_LAB) : agg_cap > 1 ? EXT_GRP8_ALT : primary ? EXT_GRP8_PRIM : EXT_GRP8];
}

// Latency-critical scalar arrays go to LDS when they fit next to the other resident wavefronts of the CU.  The budget: a
// wavefront's share of the CU's 160 KB minus the kernel's static LDS and a margin (overshooting by a few bytes costs a whole
// resident wavefront per CU); the dynamic LDS per read: what its arrays want (fast_lds_bytes) or its share of the budget.
static uint32_t lds_budget(uint32_t waves_cu, uint32_t static_lds, uint32_t margin) { return (160u * 1024u) / waves_cu - static_lds - margin; }
static uint32_t lds_per_read(uint32_t Lmax, uint32_t waves_cu, uint32_t static_lds, uint32_t margin, uint32_t reads_per_wave = 1) {
    return std::min<uint32_t>(fast_lds_bytes(Lmax), lds_budget(waves_cu, static_lds, margin) / reads_per_wave) & ~15u;
}


// (the functions of the C ABI stand in extern "C" blocks; what the host units call in one another — host_state.hpp — outside them)
extern "C" {

int mgx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char *mgx_last_error(void) { return g_err.c_str(); }
// the kernel units of libmgx.so (mgx_annot.hip) report through the same thread-local message
void mgx_set_last_error(const char *msg) { g_err = msg ? msg : ""; }
uint32_t mgx_abi_version(void) { return MGX_ABI_VERSION; }

void mgx_config_init_default(mgx_config *c) {
    memset(c, 0, sizeof(*c));
    c->num_alternative_paths = 1;
    c->max_num_seeds_per_locus = UINT64_MAX;
    c->min_cell_score = INT32_MIN + 100;
    c->min_path_score = 0;
    c->xdrop = INT32_MAX;
    c->max_nodes_per_seq_char = 1.7976931348623157e308;
    c->max_ram_per_alignment = 1.7976931348623157e308;
    c->gap_opening_penalty = -5;
    c->gap_extension_penalty = -2;
    c->forward_and_reverse_complement = 1;
    c->global_xdrop = 1;
    c->allow_left_trim = 1;
    c->seed_complexity_filter = 1;
}

void mgx_config_set_dna_matrix(mgx_config *c, int8_t match, int8_t mm_transition, int8_t mm_transversion) {
    for (int i = 0; i < 128; ++i)
        for (int j = 0; j < 128; ++j) c->score_matrix[i][j] = mm_transversion;
    c->score_matrix['A']['G'] = c->score_matrix['G']['A'] = mm_transition;
    c->score_matrix['C']['T'] = c->score_matrix['T']['C'] = mm_transition;
    c->score_matrix['A']['A'] = c->score_matrix['C']['C'] = c->score_matrix['G']['G'] = c->score_matrix['T']['T'] = match;
}

void mgx_config_set_unit_matrix(mgx_config *c, int8_t match) {
    for (int i = 0; i < 128; ++i)
        for (int j = 0; j < 128; ++j) c->score_matrix[i][j] = (int8_t)-match;
    c->score_matrix['A']['A'] = c->score_matrix['C']['C'] = c->score_matrix['G']['G'] = c->score_matrix['T']['T'] = match;
}

void mgx_config_set_scoring_matrix(mgx_config *c) {
    if (c->alignment_edit_distance) {
        mgx_config_set_unit_matrix(c, 1);
        c->left_end_bonus = 0;
        c->right_end_bonus = 0;
    } else {
        mgx_config_set_dna_matrix(c, c->alignment_match_score, (int8_t)-c->alignment_mm_transition_score,
                                  (int8_t)-c->alignment_mm_transversion_score);
    }
}

void mgx_config_init_cli(mgx_config *c, uint32_t k) {
    mgx_config_init_default(c);
    c->min_seed_length = std::min<uint64_t>(19, k);
    c->max_seed_length = UINT64_MAX;
    c->max_num_seeds_per_locus = 1000;
    c->xdrop = 27;
    c->min_exact_match = 0.7;
    c->max_nodes_per_seq_char = 5.0;
    c->max_ram_per_alignment = 200.0;
    c->rel_score_cutoff = 0.95;
    c->gap_opening_penalty = -6;
    c->gap_extension_penalty = -2;
    c->left_end_bonus = 5;
    c->right_end_bonus = 5;
    c->alignment_edit_distance = 0;            /* cli/config/config.hpp:117-120 */
    c->alignment_match_score = 2;
    c->alignment_mm_transition_score = 3;
    c->alignment_mm_transversion_score = 3;
    mgx_config_set_scoring_matrix(c);
}

void mgx_limits_init_default(mgx_limits *l, uint32_t max_query_length) {
    memset(l, 0, sizeof(*l));
    l->max_query_length = max_query_length;      // the rest: 0 = derive from the config at batch time
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// aligner
// ------------------------------------------------------------------------------------------------
static int aligner_create_for(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *anno, bool chainer,
                              mgx_aligner **out) {
    if (!g || !config || !out) return fail(MGX_ERR_INVALID, "null argument");
    auto *A = new mgx_aligner();
    std::unique_ptr<mgx_aligner> guard(A);
    A->chainer = chainer;
    A->graph = g;
    A->anno = anno;
    A->device = g->device;
    // every device buffer of an aligner goes through the per-device block pool (DevPool): the next aligner takes them over
    for (DevBuf *b : { &A->mlen_fwd, &A->mlen_rc, &A->pk_fwd, &A->pk_rc, &A->iv_fwd, &A->iv_rc, &A->rng_fwd, &A->rng_rc, &A->score_matrix,
                       &A->seqs, &A->offsets, &A->counts, &A->node_begin, &A->nodes_fwd, &A->nodes_rc, &A->arena, &A->results, &A->stream,
                       &A->cursors, &A->d_stats, &A->d_stats_map, &A->scan_tmp, &A->dbg_seeds, &A->seed_hdr, &A->seed_stream, &A->work_key,
                       &A->work_key_sorted, &A->order_in, &A->order, &A->sort_tmp, &A->retry_list, &A->resume_pool[0], &A->resume_pool[1],
                       &A->retry_list2, &A->retry_key[0], &A->retry_key[1], &A->lane_scratch, &A->lane_params, &A->lane_bail, &A->lane_hist, &A->seedlane_scratch, &A->seedlane_params,
                       &A->seedlane_bail, &A->seedlane_hist, &A->ms_counts, &A->ms_nodes, &A->ms_sorted, &A->mf_threshold, &A->tf_headers, &A->tf_header_offsets,
                       &A->tf_names, &A->tf_len, &A->tf_begin, &A->tf_text, &A->tf_cap, &A->tf_patch, &A->rd_counts, &A->rd_begins, &A->rd_totals, &A->rd_alns,
                       &A->rd_nodes, &A->rd_cigar, &A->rd_seqs, &A->rd_status, &A->rd_labels,
                       &A->ct.counts, &A->ct.begins, &A->ct.pair_key, &A->ct.pair_key_alt, &A->ct.pair_val, &A->ct.pair_val_alt, &A->ct.kept, &A->ct.n_kept,
                       &A->ct.seeds, &A->ct.nodes, &A->ct.num_matching, &A->ct.status, &A->ct.qsize, &A->ct.penalty, &A->ct.anchors, &A->ct.anchors_alt,
                       &A->ct.backtrace, &A->ct.perm, &A->ct.perm_alt, &A->ct.k32, &A->ct.k32_alt, &A->ct.k64, &A->ct.k64_alt, &A->ct.sort_tmp, &A->ct.sort_tmp_anchors })
        b->pooled = true;
    {
        std::string err;
        int rc = prepare_config(*config, g->g.k, &A->cfg, &A->dcfg, &err, anno != nullptr);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    if (anno) {
        // LabeledAligner<>(graph, config, annotator) (aligner_labeled.hpp:125-127).  On the device: BASIC-, PRIMARY- and
        // CANONICAL-mode graphs (labels looked up by base node through the CanonicalDBG wrapper, resp. by the k-mer's
        // representative: include/mgx.h), annotation without coordinates, as many alternative paths per label as the
        // labeled kernel build holds.
        const int lab_max_alt = std::min(std::min(mgx_lab64_max_alt(), mgx_grp_max_alt8_lab()), std::min(mgx_lab64x_max_alt(), mgx_grp_max_alt8_labx()));
        if (A->cfg.num_alternative_paths > (uint64_t)lab_max_alt)
            return fail(MGX_ERR_UNSUPPORTED, "label-aware alignment: num_alternative_paths <= %d on the device", lab_max_alt);
        int adev = 0; uint64_t arows = 0; const uint64_t *h; const uint32_t *c, *m;
        mgx_annotation_device_view(anno, &adev, &arows, &h, &c, &m);
        if (adev != g->device) return fail(MGX_ERR_INVALID, "the annotation lives on device %d, the graph on device %d", adev, g->device);
        // An annotation with coordinates makes LabeledAligner chain seeds (aligner_labeled.cpp:457-462: chain_alignments on, global
        // x-drop off).  Of that mode the device has the annotation (mgx_annotation_get_row_tuples) and the chaining DP
        // (mgx_chain_seeds); the extension between chain seeds (dbg_aligner.cpp:155-250,388-529) is not built: refused, so that
        // the caller keeps the reference's aligner — never answered with the plain label-aware mode
        // (the chain stage of that mode — seeds, their filter, the anchors and the chainer's tables — is a handle of its own:
        // mgx_seed_chainer_create)
        if (!chainer && mgx_annotation_has_coordinates(anno) && g->mode == MGX_MODE_BASIC)
            return fail(MGX_ERR_UNSUPPORTED, "label-aware alignment with coordinates (seed chaining) is not on the device");
        if (arows < g->g.n) return fail(MGX_ERR_INVALID, "the annotation has %llu rows, the graph %llu nodes (row = node - 1)",
                                        (unsigned long long)arows, (unsigned long long)g->g.n);
    }
    if (g->mode == MGX_MODE_CANONICAL) { A->dcfg.canonical = 1; A->dcfg.fwd_and_rc = 1; }     // dbg_aligner.cpp:225-226
    if (g->mode == MGX_MODE_PRIMARY) { A->dcfg.canonical = g->primary_tables ? 3 : 2; A->dcfg.fwd_and_rc = 1; }   // through the wrapper
    mgx_config &c = A->cfg;
    if (limits) { A->user_lim = *limits; A->have_user_lim = true; }
    HIP_TRY(hipSetDevice(g->device));
    if (anno) {
        if (int rc = graph_dummy_rows_clean(g, anno, &A->anno_dummy_clean)) return rc;
        if (g->mode == MGX_MODE_CANONICAL) if (int rc = graph_canon_repr(g)) return rc;
    }
    if (int rc = A->score_matrix.ensure(128 * 128)) return rc;
    HIP_TRY(hipMemcpy(A->score_matrix.p, c.score_matrix, 128 * 128, hipMemcpyHostToDevice));
    if (int rc = A->cursors.ensure(CUR_WORDS * 8)) return rc;
    if (int rc = A->d_stats.ensure(sizeof(KernelStats))) return rc;
    if (int rc = A->d_stats_map.ensure(sizeof(KernelStats))) return rc;
    for (auto &e : A->ev) HIP_TRY(hipEventCreate(&e));
    memset(&A->hstats, 0, sizeof(A->hstats));
    memset(&A->lim, 0, sizeof(A->lim));
    *out = guard.release();
    return MGX_OK;
}

int aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *anno, mgx_aligner **out) {
    return aligner_create_for(g, config, limits, anno, false, out);
}
int refuse_chainer(const mgx_aligner *A, const char *call) {
    return A && A->chainer ? fail(MGX_ERR_UNSUPPORTED, "%s: a seed-chainer handle runs mgx_chain_tables_batch / mgx_chain_tables_fetch only", call) : MGX_OK;
}

extern "C" {

int mgx_aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, mgx_aligner **out) {
    return aligner_create(g, config, limits, nullptr, out);
}
/* The chain stage of LabeledAligner's coordinate mode (include/mgx.h): the handle's config is what LabeledAligner's constructor
 * leaves for an annotation with coordinates (aligner_labeled.cpp:456-465). */
int mgx_seed_chainer_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *annotation,
                            mgx_aligner **out) {
    if (!g || !config || !annotation || !out) return fail(MGX_ERR_INVALID, "null argument");
    if (g->mode != MGX_MODE_BASIC)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_seed_chainer_create: graph mode %u (the reference has k-mer coordinates on BASIC graphs only)", g->mode);
    if (!mgx_annotation_has_coordinates(annotation))
        return fail(MGX_ERR_UNSUPPORTED, "mgx_seed_chainer_create: the annotation has no k-mer coordinates (LabeledAligner chains seeds only with them)");
    if (!config->forward_and_reverse_complement)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_seed_chainer_create: forward_and_reverse_complement = 0 (the reference chains only where it seeds both strands)");
    if (config->chain_alignments)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_seed_chainer_create: chain_alignments is set by LabeledAligner itself, never by the caller");
    mgx_config c = *config;
    c.global_xdrop = 0;
    if (int rc = aligner_create_for(g, &c, limits, annotation, true, out)) return rc;
    (*out)->cfg.chain_alignments = 1;
    return MGX_OK;
}
int mgx_labeled_aligner_create(const mgx_graph *g, const mgx_config *config, const mgx_limits *limits, const mgx_annotation *annotation,
                               mgx_aligner **out) {
    if (!annotation) return fail(MGX_ERR_INVALID, "null argument");
    return aligner_create(g, config, limits, annotation, out);
}

void mgx_aligner_destroy(mgx_aligner *a) {
    if (!a) return;
    (void)hipSetDevice(a->device);                          // (its own copy: the graph may be gone by now — a binding's GC order)
    (void)hipStreamSynchronize(a->hstream);
    for (auto &e : a->ev) if (e) (void)hipEventDestroy(e);
    if (a->h_text) (void)hipHostFree(a->h_text);
    for (void *p : a->h_rd) if (p) (void)hipHostFree(p);
    if (a->own_stream) (void)hipStreamDestroy(a->hstream);
    delete a;
}

int mgx_aligner_get_config(const mgx_aligner *a, mgx_config *out) { *out = a->cfg; return MGX_OK; }

int mgx_aligner_get_limits(const mgx_aligner *a, mgx_limits *out) {
    if (!a || !out) return fail(MGX_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    out->max_query_length = a->lim.Lmax;
    out->max_columns = a->lim.max_columns;
    out->max_seeds = a->lim.max_seeds;
    out->cell_arena_bytes = (uint64_t)a->lim.cell_words * 4;
    return MGX_OK;
}

} // extern "C"

// bits of the work-sort key: 12 of predicted work + the segment number (align_core.hpp, WORK_SEGMENT_SHIFT)
static int work_key_bits(uint64_t n) {
    int b = 12;
    for (uint64_t seg = n ? (n - 1) >> WORK_SEGMENT_SHIFT : 0; seg; seg >>= 1) ++b;
    return std::min(b, 32);
}

// ------------------------------------------------------------------------------------------------
// run_align: one staged and mapped batch through seeding, the work sort and extension
// ------------------------------------------------------------------------------------------------
// What the stages of run_align hand to one another (the limits of the batch are A->lim).
struct AlignPlan {
    uint64_t n = 0;                   // reads
    bool labeled = false;
    uint32_t cus = 0;                 // compute units of the device
    bool lane_ok = false;             // the lane-per-read kernel takes this batch's configuration (and got its scratch)
    uint32_t lane_blocks = 0;         // its resident wavefronts
    uint64_t n_exact = 0;             // reads k_lane_exact finished before the sort (LP.exact): the last n_exact items of the sorted order
    int key_bits = 0;                 // bits of the work-sort key (one more with LP.exact: LaneParams::done_key)
    LaneParams LP;
    uint64_t agg_cap = 1;             // alignments kept per query
    const ExtBuild *grp = nullptr;    // the 8-lane-group build the configuration extends on (group_build)
    uint64_t wave_slots = 0;          // resident wavefronts of the seeding kernel (one per read)
    uint64_t stride = 0, slots = 0;   // the arena: bytes per slice, slices
    size_t sort_tmp_bytes = 0;
    AlignParams P;
};

// The lane-per-read kernel (mgx_lane.hip) in front of the group kernel: does this batch's configuration qualify?  Its scratch
// is taken before the arena is sized from what is free.
static int plan_lane(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    LaneParams &LP = pl.LP;
    memset(&LP, 0, sizeof(LP));
    std::string lane_why;
    pl.lane_blocks = pl.cus * 4u * (uint32_t)mgx_lane_waves_per_simd();
    // (label-aware batches, round 6: the lane takes the reads whose seeds and columns all carry one and the same single label —
    // lane_read.hpp; it needs the annotation's "no dummy node's row holds a label" flag, as it reads rows without the W test)
    pl.lane_ok = A->opt.lane != 0 && A->packed_valid && A->opt.multi_pass != 1
                 && lane_enabled(A->cfg, A->dcfg, A->graph->g.k, l.Lmax, A->no_fast, &LP, &lane_why,
                                 pl.labeled ? (1u | (A->anno_dummy_clean ? 2u : 0u)) : 0u)
                 && (A->opt.lane == 1 || pl.n >= (uint64_t)pl.lane_blocks * 16);       // (a small batch: the spread / 64-lane kernels are quicker)
    // The exact exit (lane_read.hpp lane_exact(), k_lane_exact): option exact = 1 / 2 forces it at that level (1: reads whose first
    // seed spans the query; 2: also the path class; 3: also the substitution class), 0 turns it off; automatic: level 3
    // (LANE_EXACT_AUTO_SUB; label-aware batches: LANE_EXACT_AUTO_SUB_LABELED, else 2) for the
    // batches the lane kernel takes of its own accord — a small batch run with lane=1 keeps every read's fate in lane_read_dp()
    // what the tests of its hand-over reasons pin.  (lane_enabled() filled the flag for the host model: decided here.)
    // Label-aware batches (the reads that keep one label all along, lane_exact_class()): under the same rule, where no dummy
    // node's row holds a label (lane_exact_config()); LANE_EXACT_AUTO_LABELED records that the automatic default includes them.
    const uint32_t lflags = pl.labeled ? (1u | (A->anno_dummy_clean ? 2u : 0u)) : 0u;
    const bool exact_auto = pl.n >= (uint64_t)pl.lane_blocks * 16 && (!pl.labeled || LANE_EXACT_AUTO_LABELED);
    // (level 3, the substitution class: under lane_exact_sub_config(), else 3 means 2 — lane_exact_level())
    const uint32_t exact_auto_level = (pl.labeled ? LANE_EXACT_AUTO_SUB_LABELED : LANE_EXACT_AUTO_SUB) ? 3u : 2u;
    LP.exact = (pl.lane_ok && A->opt.exact != 0 && (A->opt.exact >= 1 || exact_auto))
                   ? lane_exact_level(A->cfg, A->dcfg, lflags, A->opt.exact >= 1 ? (uint32_t)A->opt.exact : exact_auto_level) : 0u;
    LP.sub_list = nullptr;
    pl.key_bits = work_key_bits(pl.n) + (LP.exact ? 1 : 0);
    LP.done_key = LP.exact ? 1u << work_key_bits(pl.n) : 0u;
    if (!pl.lane_ok) return MGX_OK;
    LP.max_cols = lane_max_cols(l.Lmax, A->dcfg.xdrop);
    LP.hash_slots = next_pow2(2ull * LP.max_cols);
    if (int hm; env_int("MGX_LANE_HASH_MULT", &hm)) LP.hash_slots *= (uint32_t)std::max(1, hm);
    LP.rest_stride = (lane_rest_bytes(LP.max_cols, LP.hash_slots) + 63) & ~63ull;
    LP.wave_stride = lane_wave_scratch_bytes(LP.max_cols, LP.rest_stride);
    const size_t before = A->lane_scratch.bytes;
    if (A->lane_scratch.ensure((size_t)pl.lane_blocks * LP.wave_stride, true) != MGX_OK) pl.lane_ok = false;      // (no room: the group kernel alone)
    else if (A->lane_scratch.bytes != before) HIP_TRY(hipMemsetAsync(A->lane_scratch.p, 0, A->lane_scratch.bytes, A->hstream));    // node tables start empty
    return MGX_OK;
}

// How many reads are in flight at once (slots), each with a slice of the arena: as many as the kernels keep resident, or as
// the free memory holds.
static int size_arena(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    const uint64_t n = pl.n, stride = arena_bytes(l);
    pl.stride = stride;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    pl.wave_slots = (uint64_t)pl.cus * 4 * MGX_ALIGN_WAVES_PER_SIMD;
    // (post_chain_alignments keeps up to MGX_MAX_ALTERNATIVE_PATHS alignments per query: the build with room for them)
    pl.agg_cap = std::max<uint64_t>(1, A->cfg.post_chain_alignments ? (uint64_t)post_chain_capacity(A->cfg.num_alternative_paths) : A->cfg.num_alternative_paths);
    pl.grp = &group_build(pl.labeled, A->dcfg.canonical >= 2, pl.agg_cap, A->dcfg.branch_xdrop != 0);
    // (label-aware batches: seeding as ever, extension on the labeled builds)
    const uint64_t want_slots = std::max<uint64_t>(pl.wave_slots, (uint64_t)pl.cus * waves_per_cu(*pl.grp) * 8);
    // The arena gets what is free after the buffers this stage allocates AFTER it (result records, output stream, seed
    // stream, sort arrays: estimated generously) and a margin; buffers kept from an earlier batch are already outside
    // `free_b`.  (Half of the free memory, as before, left 15 % of the extension kernel's groups without a slice at
    // 10 M reads next to a host framework's cached allocations.)
    const uint64_t later = n * (sizeof(ReadResult) + sizeof(SeedHdr) + 24 + 16)
                           + (n * (((uint64_t)l.Lmax + l.Lmax / 4 + 40) * pl.agg_cap) + 1024) * 4
                           + (n * 24 + A->total_kmers / 8 + 4096) * A->seed_scale * sizeof(DevSeed) + (1ull << 30);
    const uint64_t held = A->results.bytes + A->stream.bytes + A->seed_stream.bytes + A->seed_hdr.bytes;     // re-used as far as they reach
    const uint64_t need_later = later > held ? later - held : 0;
    const uint64_t avail = (uint64_t)free_b + A->arena.bytes + g_pool.held_bytes();     // a growing arena frees its old block first; what the
                                                                                          // block pool holds is handed out or freed on demand
    uint64_t budget = avail > need_later ? (avail - need_later) / 10 * 9 : avail / 2;
    // (device_share: this handle is one of several at work on the device — each gets its share of the slots the machine can keep
    // resident and of the memory, instead of the first handles taking all of it and the later ones what is left)
    const uint64_t share = (uint64_t)std::max(1, A->opt.device_share);
    budget /= share;
    uint64_t slots = std::min<uint64_t>(std::min<uint64_t>((want_slots + share - 1) / share, std::max<uint64_t>(n, 1)), std::max<uint64_t>(1, budget / stride));
    if (slots == 0) slots = 1;
    // The hash tables of the convergence checker are cleared by generation tags that persist in each slice,
    // so a slice only needs zeroing when its layout (stride) changes or the buffer is new.
    const size_t before = A->arena.bytes;
    if (int rc = A->arena.ensure(slots * stride, true)) return rc;
    if (A->arena.bytes != before || A->arena_stride != stride) {
        HIP_TRY(hipMemsetAsync(A->arena.p, 0, A->arena.bytes, A->hstream));
        A->arena_stride = stride;
    }
    pl.slots = slots;
    A->n_slots = (uint32_t)slots;
    if (probe_env_set("MGX_DEBUG_SLOTS")) fprintf(stderr, "run_align: n %llu stride %llu want_slots %llu slots %llu free %.1f GB\n", (unsigned long long)n, (unsigned long long)stride, (unsigned long long)want_slots, (unsigned long long)slots, free_b / 1e9);
    return MGX_OK;
}

// Result records, output stream, seed stream and sort arrays of the batch; the cursors and counters of this run start at zero.
static int size_buffers(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    const uint64_t n = pl.n;
    if (int rc = A->results.ensure(n * sizeof(ReadResult))) return rc;
    uint64_t words_per_read = ((uint64_t)l.Lmax + l.Lmax / 4 + 40) * pl.agg_cap;
    if (pl.labeled) words_per_read = words_per_read * 2 + 16;      // (an alignment per label group + the label lists; heuristic as below)
    // heuristic size (one alignment per read: nodes + CIGAR runs + path characters); a batch that needs more is re-run
    // with what it asked for (mgx_align_batch_device), so the size is never a correctness limit
    A->out_words = std::max<uint64_t>(n * words_per_read + 1024, A->out_min_words);
    if (int rc = A->stream.ensure(A->out_words * 4)) return rc;
    if (A->keep_seeds) {
        if (int rc = A->dbg_seeds.ensure(n * 2 * (uint64_t)l.max_seeds * sizeof(DevSeed))) return rc;
        HIP_TRY(hipMemsetAsync(A->dbg_seeds.p, 0, n * 2 * (uint64_t)l.max_seeds * sizeof(DevSeed), A->hstream));
    }
    HIP_TRY(clear_cursors(A, CUR_OUT, CUR_RETRY));
    HIP_TRY(hipMemsetAsync(A->d_stats.p, 0, sizeof(KernelStats), A->hstream));     // counters of this run of the stage only
    // Seeds travel from the seeding kernels to the extension kernels through a compact stream.  Typical reads carry a handful
    // of seeds; long or repetitive ones scale with their k-mer count.  The stream is sized by a heuristic times A->seed_scale;
    // mgx_align_batch_device re-runs the stage with a larger scale if the seeding kernel ran out of room (the cursor keeps
    // counting), so the size is never a correctness limit.
    A->seed_cap = std::min<uint64_t>(n * 2 * (uint64_t)l.max_seeds, (n * 24 + A->total_kmers / 8 + 4096) * A->seed_scale);
    if (int rc = A->seed_hdr.ensure(n * sizeof(SeedHdr))) return rc;
    if (int rc = A->seed_stream.ensure(A->seed_cap * sizeof(DevSeed))) return rc;
    if (int rc = A->work_key.ensure(n * 4)) return rc;
    if (int rc = A->work_key_sorted.ensure(n * 4)) return rc;
    if (int rc = A->order_in.ensure(n * 4)) return rc;
    if (int rc = A->order.ensure(n * 4)) return rc;
    if (int rc = A->retry_list.ensure(n * 4 + 4)) return rc;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, pl.sort_tmp_bytes, A->work_key.as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                               A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)n, 0, pl.key_bits, A->hstream));
    return A->sort_tmp.ensure(pl.sort_tmp_bytes);
}

// the kernels' parameter block (host side only: every buffer it points to exists by now)
static void fill_params(mgx_aligner *A, AlignPlan &pl, const char *d_seqs, const uint64_t *d_offsets) {
    AlignParams &P = pl.P;
    memset(&P, 0, sizeof(P));
    P.g = A->graph->g;
    P.cfg = A->dcfg;
    P.lim = A->lim;
    P.score_matrix = A->score_matrix.as<int8_t>();
    P.seqs = d_seqs;
    P.offsets = d_offsets;
    P.node_begin = A->node_begin.as<uint64_t>();
    P.nodes_fwd = A->nodes_fwd.as<uint32_t>();
    P.nodes_rc = A->nodes_rc.as<uint32_t>();
    P.mlen_fwd = A->mlen_fwd.as<uint8_t>();
    P.mlen_rc = A->mlen_rc.as<uint8_t>();
    P.rng_fwd = A->have_rng ? A->rng_fwd.as<uint2>() : nullptr;
    P.rng_rc = A->have_rng ? A->rng_rc.as<uint2>() : nullptr;
    P.n_reads = pl.n;
    P.arena = A->arena.as<uint8_t>();
    P.arena_stride = pl.stride;
    P.results = A->results.as<ReadResult>();
    P.out_stream = A->stream.as<uint32_t>();
    P.out_capacity = A->out_words;
    P.out_cursor = cursor(A, CUR_OUT);
    P.read_cursor = cursor(A, CUR_READ);
    P.stats = A->d_stats.as<KernelStats>();
    P.dbg_seeds = A->keep_seeds ? A->dbg_seeds.as<DevSeed>() : nullptr;
    P.no_fast = A->no_fast;
    if (A->packed_valid) {
        P.pkw[0] = A->pk_fwd.as<uint64_t>(); P.ivw[0] = A->iv_fwd.as<uint32_t>();
        P.pkw[1] = A->dcfg.fwd_and_rc ? A->pk_rc.as<uint64_t>() : nullptr; P.ivw[1] = A->dcfg.fwd_and_rc ? A->iv_rc.as<uint32_t>() : nullptr;
    }
    P.no_compact = A->opt.no_compact != 0;
    P.no_alias = A->opt.no_alias != 0;
    P.no_bt_runs = A->opt.no_bt_runs != 0;
    P.no_flat = A->opt.no_flat != 0 || A->cfg.post_chain_alignments;       // (the flat group loop is the one-alignment-per-query driver)
    if (pl.labeled) {
        int adev = 0;
        mgx_annotation_device_view(A->anno, &adev, &P.anno_rows, &P.anno_head, &P.anno_count, &P.anno_more);
        P.labeled = 1u | (A->anno_dummy_clean ? 2u : 0u);
        P.anno_base = A->graph->mode == MGX_MODE_CANONICAL ? A->graph->canon_repr.as<uint32_t>() : nullptr;
        P.no_alias = 1;           // (a flush clears columns in place: convergence entries must not alias their S windows)
    }
    P.ablate = probe_env_u32("MGX_ABLATE", 0u);      // timing probes: WRONG results (probe builds only)
    P.seed_hdr = A->seed_hdr.as<SeedHdr>();
    P.seed_stream = A->seed_stream.as<DevSeed>();
    P.seed_capacity = A->seed_cap;
    P.seed_cursor = cursor(A, CUR_SEED);
    P.work_key = A->work_key.as<uint32_t>();
}

// The lane-per-read seeder (seed_lane.hpp, mgx_seedlane.hip) first: every lane seeds its own read and either publishes
// header, seeds and work key as the seeding kernel would, or lists the read for a second pass with bigger buffers; what that
// leaves is listed for the seeding kernel, which then seeds the list from scratch (no host round trip in between: the lists'
// lengths stay on the device).
static int seed_by_lanes(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    AlignParams &P = pl.P;
    const uint64_t n = pl.n;
    const bool seed_lane = A->opt.seed_lane != 0 && A->packed_valid && P.pkw[0] && P.ivw[0]
                           && (!A->dcfg.fwd_and_rc || (P.pkw[1] && P.ivw[1])) && P.mlen_fwd && P.rng_fwd
                           && (!A->dcfg.fwd_and_rc || (P.mlen_rc && P.rng_rc))
                           && seed_lane_enabled(A->dcfg, (uint32_t)A->graph->g.k, l.Lmax, true, true)
                           && (A->opt.seed_lane == 1 || n >= 4096);
    if (!seed_lane || !n) return MGX_OK;
    const bool long_reads = l.Lmax > (uint32_t)SL_SHORT_L;            // (the kernel's build with nine packed words per strand)
    const uint32_t resident = pl.cus * 4 * (uint32_t)mgx_seed_lane_waves_per_simd();
    const uint32_t blocks1 = (uint32_t)std::min<uint64_t>(resident, (n + 63) / 64);
    // (the second pass: what the first left — a sixth of a typical batch — with the big buffers)
    const uint32_t blocks2 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident / (long_reads ? 2 : 1), (n / 4 + 63) / 64));
    const bool many = (uint64_t)A->graph->g.k >= A->dcfg.max_seed_length;
    const uint32_t me1 = many ? (long_reads ? SL_SEEDS_1_MANY_LONG : SL_SEEDS_1_MANY) : SL_SEEDS_1, mp1 = many ? SL_PENDING_1_MANY : SL_PENDING_1;
    const uint32_t me2 = long_reads ? SL_SEEDS_2_LONG : SL_SEEDS_2, mp2 = long_reads ? SL_PENDING_2_LONG : SL_PENDING_2;
    const uint64_t words1 = seed_lane_wave_scratch_words(me1, mp1), words2 = seed_lane_wave_scratch_words(me2, mp2);
    if (int rc = A->seedlane_scratch.ensure((size_t)std::max<uint64_t>(blocks1 * words1, blocks2 * words2) * 4)) return rc;
    if (int rc = A->seedlane_params.ensure(2 * sizeof(SeedLaneParams))) return rc;
    if (int rc = A->seedlane_bail.ensure(2 * (n * 4 + 4))) return rc;
    if (int rc = A->seedlane_hist.ensure(32 * 8)) return rc;          // ([16 .. 24): section timers of -DMGX_SL_TIMERS builds)
    HIP_TRY(hipMemsetAsync(A->seedlane_hist.p, 0, 32 * 8, A->hstream));
    HIP_TRY(clear_cursors(A, CUR_SL_BAIL, CUR_SL_BAIL_BACK));
    SeedLaneParams SP[2];
    memset(SP, 0, sizeof(SP));
    uint32_t *list1 = A->seedlane_bail.as<uint32_t>(), *list2 = list1 + n + 1;
    for (int ps = 0; ps < 2; ++ps) {
        SP[ps].P = P;
        SP[ps].P.n_items = n;
        SP[ps].scratch = A->seedlane_scratch.as<uint32_t>();
        SP[ps].long_reads = long_reads ? 1u : 0u;
        SP[ps].second_pass = (uint32_t)ps;
        SP[ps].list_len = n;
        SP[ps].done_count = cursor(A, CUR_SL_DONE);
    }
    // first pass: every read; what it leaves goes to list1 from both ends
    SP[0].max_entries = me1; SP[0].max_pending = mp1;
    SP[0].bail_list = list1; SP[0].bail_count = cursor(A, CUR_SL_BAIL); SP[0].bail_count_back = cursor(A, CUR_SL_BAIL_BACK);
    // second pass: list1; what it leaves goes to list2 (why a read left is counted where it leaves for the wave program)
    SP[1].max_entries = me2; SP[1].max_pending = mp2;
    SP[1].in_list = list1; SP[1].in_count = cursor(A, CUR_SL_BAIL); SP[1].in_count_back = cursor(A, CUR_SL_BAIL_BACK);
    SP[1].bail_list = list2; SP[1].bail_count = cursor(A, CUR_SL_BAIL2);
    SP[1].bail_hist = A->seedlane_hist.as<unsigned long long>();
    HIP_TRY(copy_sync(A, A->seedlane_params.p, SP, sizeof(SP), hipMemcpyHostToDevice));
    if (int rc = mgx_launch_seed_lane(A->seedlane_params.p, blocks1, long_reads, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane-per-read seeder: %d", rc);
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    if (int rc = mgx_launch_seed_lane(A->seedlane_params.as<SeedLaneParams>() + 1, blocks2, long_reads, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane-per-read seeder, second pass: %d", rc);
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    P.seed_list = list2;
    P.n_items_ptr = cursor(A, CUR_SL_BAIL2);
    A->seedlane_launched = 1;
    return MGX_OK;
}

// The seeding kernel, one wavefront per read, on every read or on what the lane-per-read seeder listed: the instantiation at
// 8 wavefronts per SIMD for short reads on a full machine, else the one at MGX_ALIGN_WAVES_PER_SIMD; PRIMARY graphs: the
// build with the CanonicalDBG branches (mgx_seed.hip holds both).
static int seed_by_waves(mgx_aligner *A, AlignPlan &pl) {
    const DevLimits &l = A->lim;
    AlignParams &P = pl.P;
    const bool primary = A->dcfg.canonical >= 2;
    const auto launch = primary ? mgx_launch_seed_primary : mgx_launch_seed;
    const uint32_t static_lds = mgx_seed_static_lds();        // (either build: each asserts MGX_SEED_STATIC_LDS_BYTES)
    uint32_t blocks, lds;
    const bool wps8 = A->opt.seed_wps == 8 && l.Lmax <= 192 && pl.slots >= (uint64_t)pl.cus * 4 * 8;
    if (wps8) {
        // (measured on 150-bp reads: the kernel is 10 % faster with 4944 B of LDS per wavefront than with 5056 B, although
        // both leave room for 32 wavefronts per CU; hence the wider margin)
        uint32_t lds8 = lds_per_read(l.Lmax, 4 * MGX_SEED_WPS, static_lds, 192u);
        lds8 = std::min<uint32_t>(lds8, probe_env_u32("MGX_SEED_LDS_CAP", lds8)) & ~15u;     // tuning probe
        if (probe_env_set("MGX_SEED_LDS_PRINT")) fprintf(stderr, "k_seed: static_lds %u budget8 %u lds8 %u (fast_lds_bytes %u)\n", static_lds, lds_budget(4 * MGX_SEED_WPS, static_lds, 192u), lds8, fast_lds_bytes(l.Lmax));
        // tuning probe (plain build): MGX_SEED_WAVES_PCT=50 launches half the resident wavefronts (is the kernel bound by what
        // each wavefront waits for, or by what all of them move?)
        const uint32_t spct = probe_env_pct("MGX_SEED_WAVES_PCT");
        blocks = primary ? pl.cus * 4 * MGX_SEED_WPS : std::max(1u, pl.cus * 4 * MGX_SEED_WPS * spct / 100);
        lds = lds8;
    } else {
        blocks = (uint32_t)std::min<uint64_t>(pl.slots, pl.wave_slots);
        lds = lds_per_read(l.Lmax, 4 * MGX_ALIGN_WAVES_PER_SIMD, static_lds, 64u);
    }
    if (int rc = launch(&P, blocks, lds, wps8 ? 1 : 0, A->hstream))
        return primary ? fail(MGX_ERR_NO_DEVICE, "seeding kernel (PRIMARY): %d", rc) : hip_fail((hipError_t)rc, "hipGetLastError()", __FILE__, __LINE__);
    P.seed_list = nullptr; P.n_items_ptr = nullptr;
    return MGX_OK;
}

// the reads in the order of their predicted extension work (the seeding kernels wrote the keys)
static int sort_by_work(mgx_aligner *A, AlignPlan &pl) {
    const uint64_t n = pl.n;
    k_iota<<<(uint32_t)((n + 255) / 256), 256, 0, A->hstream>>>(A->order_in.as<uint32_t>(), n);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(A->sort_tmp.p, pl.sort_tmp_bytes, A->work_key.as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                               A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)n, 0, pl.key_bits, A->hstream));
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    pl.P.order = A->order.as<uint32_t>();
    return MGX_OK;
}

// Multi-pass extension (option multi_pass; default: when a batch carries many seeds per read): a pass extends at most one seed
// per read; reads with live seeds left write a resume record and are re-sorted by the work of their next seed for the next pass
// (AlignParams::resume_*).  Reads of a wavefront then differ by one extension at most, instead of waiting for the mate with
// the most seeds.
static int choose_multi_pass(mgx_aligner *A, const AlignPlan &pl, bool *multi) {
    *multi = false;
    if (pl.labeled || A->cfg.post_chain_alignments) return MGX_OK;      // (resume records hold num_alternative_paths alignments)
    *multi = A->opt.multi_pass == 1;
    if (A->opt.multi_pass < 0) {
        // automatic: worth it when reads run many extensions, i.e. carry many seeds (sub-k seeds of a pan-genome: ~100 per
        // read; a plain read: a handful).  The seeding kernel has finished counting them by now.
        unsigned long long seeds_total = 0;
        HIP_TRY(copy_sync(A, &seeds_total, cursor(A, CUR_SEED), 8, hipMemcpyDeviceToHost));
        *multi = pl.n > 0 && seeds_total / pl.n >= 24;
    }
    return MGX_OK;
}

// The lane kernel's device-side parameter block, list and counters: taken and cleared once per run of the stage, before the first
// of k_lane_exact and k_lane.
static int prepare_lane(mgx_aligner *A, AlignPlan &pl) {
    LaneParams &LP = pl.LP;
    // (exact level 3: the candidate list of the substitution class, one record a read at most — LaneSubCand, label-aware
    // LaneSubCandLabeled — lives in the same buffer: k_lane_exact writes it, k_lane_exact_sub reads it, and only then, behind the sort,
    // k_lane lists the reads it passes on)
    const uint64_t cand_bytes = pl.labeled ? sizeof(LaneSubCandLabeled) : sizeof(LaneSubCand);
    if (int rc = A->lane_bail.ensure(std::max<uint64_t>(pl.n * 4 + 4, LP.exact >= 3u ? pl.n * cand_bytes : 0))) return rc;
    if (int rc = A->lane_params.ensure(sizeof(LaneParams))) return rc;
    if (int rc = A->lane_hist.ensure(64 * 8)) return rc;          // ([32 .. 41]: section timers of -DMGX_LANE_TIMERS builds, [LANE_HIST_EXACT])
    HIP_TRY(hipMemsetAsync(A->lane_hist.p, 0, 64 * 8, A->hstream));
    HIP_TRY(clear_cursors(A, CUR_LANE_BAIL, CUR_LANE_DONE));
    LP.pk[0] = A->pk_fwd.as<uint64_t>(); LP.pk[1] = A->pk_rc.as<uint64_t>();
    LP.iv[0] = A->iv_fwd.as<uint32_t>(); LP.iv[1] = A->iv_rc.as<uint32_t>();
    LP.scratch = A->lane_scratch.as<uint8_t>();
    LP.bail_list = A->lane_bail.as<uint32_t>();
    LP.sub_list = A->lane_bail.as<LaneSubCand>();
    LP.bail_count = cursor(A, CUR_LANE_BAIL);
    LP.done_count = cursor(A, CUR_LANE_DONE);
    LP.bail_hist = A->lane_hist.as<unsigned long long>();
    return MGX_OK;
}

// The exact exit, between seeding and the work sort (plan_lane set LP.exact): k_lane_exact finishes every read whose first seed
// spans the query (at level 2 also every read of the path class, lane_read.hpp) and gives it the work key LP.done_key, which sorts it behind the reads that are still to be aligned; their number
// comes back to the host, which launches k_lane on the items in front of them.
static int exact_by_lanes(mgx_aligner *A, AlignPlan &pl) {
    LaneParams &LP = pl.LP;
    LP.P = pl.P;
    LP.P.n_items = pl.n;
    HIP_TRY(copy_sync(A, A->lane_params.p, &LP, sizeof(LP), hipMemcpyHostToDevice));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)pl.cus * 4 * 8 * 4, (pl.n + 63) / 64);
    if (int rc = mgx_launch_lane_exact(A->lane_params.p, blocks, pl.labeled ? 1 : 0, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane kernel, exact exit: %d", rc);
    // level 3: k_lane_exact listed the candidates of the substitution class; k_lane_exact_sub (label-aware: k_lane_exact_sub_labeled
    // behind k_lane_exact_labeled) walks them, a lane each, taking their number from device memory — sized for the most there can
    // be, its wavefronts leave at once where there are fewer
    if (LP.exact >= 3u) {
        if (int rc = mgx_launch_lane_exact_sub(A->lane_params.p, blocks, pl.labeled ? 1 : 0, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane kernel, exact exit (substitutions): %d", rc);
    }
    unsigned long long done = 0;
    HIP_TRY(copy_sync(A, &done, cursor(A, CUR_LANE_DONE), 8, hipMemcpyDeviceToHost));      // (synchronises with the kernels)
    pl.n_exact = done;
    // ... of them in the path class (level 2) and in the substitution class (level 3): counted apart, the first-seed-spans class keeps
    // its counter (two neighbouring words of the histogram, one copy)
    static_assert(LANE_HIST_EXACT_SUB == LANE_HIST_EXACT_PATH + 1, "read back together");
    unsigned long long apart[2] = { 0, 0 };
    if (LP.exact >= 2u && done)
        HIP_TRY(copy_sync(A, apart, A->lane_hist.as<unsigned long long>() + LANE_HIST_EXACT_PATH, LP.exact >= 3u ? 16 : 8, hipMemcpyDeviceToHost));
    A->lane_exact = done - apart[0] - apart[1];
    A->lane_exact_path = apart[0];
    A->lane_exact_sub = apart[1];
    return MGX_OK;
}

// Every read through the lane-per-read kernel first, in the sorted order; what it lists goes on to the extension kernel
// (the plan's order and item count become that list; *all_done: it is empty).
static int extend_by_lanes(mgx_aligner *A, AlignPlan &pl, bool *all_done) {
    AlignParams &P = pl.P;
    LaneParams &LP = pl.LP;
    // (the reads k_lane_exact finished are the last items of the sorted order: not k_lane's)
    const uint64_t n = pl.n - pl.n_exact;
    if (n == 0) {                 // every read left through the exact exit
        A->lane_done = pl.n_exact;
        A->kernels_ran |= MGX_KERNEL_LANE;
        HIP_TRY(hipEventRecord(A->ev[EV_LANE_END], A->hstream));
        *all_done = true;
        return MGX_OK;
    }
    LP.P = P;
    LP.P.n_items = n;
    LP.tag_seed = ++A->lane_epoch * 0x632BE5ABu;
    HIP_TRY(copy_sync(A, A->lane_params.p, &LP, sizeof(LP), hipMemcpyHostToDevice));
    uint32_t blocks = (uint32_t)std::min<uint64_t>(pl.lane_blocks, (n + 63) / 64);
    if (int pct; env_int("MGX_LANE_BLOCKS_PCT", &pct)) blocks = std::max<uint32_t>(1u, (uint32_t)((uint64_t)blocks * (uint64_t)pct / 100));
    if (int rc = mgx_launch_lane(A->lane_params.p, blocks, A->hstream)) return fail(MGX_ERR_NO_DEVICE, "lane kernel: %d", rc);
    A->kernels_ran |= MGX_KERNEL_LANE;
    ++g_kernel_launches[CNT_LANE];
    HIP_TRY(hipEventRecord(A->ev[EV_LANE_END], A->hstream));
    unsigned long long counts[2] = { 0, 0 };      // CUR_LANE_BAIL, CUR_LANE_DONE
    HIP_TRY(copy_sync(A, counts, cursor(A, CUR_LANE_BAIL), 16, hipMemcpyDeviceToHost));     // (synchronises with the kernel)
    A->lane_done = counts[1];
    HIP_TRY(copy_sync(A, A->lane_hist_h, A->lane_hist.p, 32 * 8, hipMemcpyDeviceToHost));
    if (int on; env_int("MGX_LANE_TIMERS", &on)) {
        unsigned long long t[16];
        HIP_TRY(copy_sync(A, t, A->lane_hist.as<unsigned long long>() + 32, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "k_lane timers (cycles of lane 0, summed over %u wavefronts): setup %llu children %llu column %llu node-table %llu commit %llu frontier %llu trace %llu result %llu | emit %llu kernel %llu\n",
                blocks, t[0], t[1], t[2], t[7], t[3], t[4], t[5], t[6], t[8], t[9]);
    }
    HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
    P.order = A->lane_bail.as<uint32_t>();
    P.n_items = counts[0];
    *all_done = counts[0] == 0;
    return MGX_OK;
}

// One launch of the extension kernel on the plan's work items (P.order / P.n_items): which build, on how many groups or
// wavefronts (never more than arena slices), with how much LDS per read.  Returns the launcher's hipError_t.
static int launch_extension(mgx_aligner *A, AlignPlan &pl) {
    const uint32_t Lmax = A->lim.Lmax;
    const int gpw_opt = A->opt.groups_per_wave;                             // -1 = automatic, 0 = all 8
    const uint64_t items = pl.P.n_items ? pl.P.n_items : pl.n;             // (a later pass of the multi-pass extension: its retry positions)
    const ExtBuild *b = pl.grp;
    uint32_t gpw, count, lds;         // AlignParams::groups_per_wave (0 = all 8); groups (8-lane builds) or wavefronts; LDS per read
    if (pl.labeled) {
        // label-aware extension: the labeled builds — 8 reads per wavefront (mgx_grp.hip, per-read program), or one read
        // per wavefront on the 64-lane kernel (mgx_lab64.hip) for batches with fewer reads than resident wavefronts
        const ExtBuild &lab64 = g_ext_builds[A->dcfg.branch_xdrop ? EXT_LAB64_BX : EXT_LAB64];
        const uint64_t resident64 = (uint64_t)pl.cus * waves_per_cu(lab64);
        if ((items <= resident64 && A->opt.ext64 != 0) || A->opt.ext64 == 2) {
            b = &lab64; gpw = 1;
            count = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(pl.slots, resident64));
        } else {
            gpw = gpw_opt > 0 ? (uint32_t)std::min(8, gpw_opt) : 0u;
            count = (uint32_t)pl.slots;
        }
    } else {
        // tuning probe: MGX_EXT_GROUPS_PCT=50 launches half the resident groups (occupancy experiments)
        const uint32_t pct = probe_env_pct("MGX_EXT_GROUPS_PCT");
        count = (uint32_t)std::min<uint64_t>(pl.slots, std::max<uint64_t>(1, pl.slots * pct / 100));
        // Fewer reads than resident groups (long-read batches, single queries): spread them over the wavefronts.  The 8
        // groups of a wavefront execute in lock-step, and reads of 1 .. 12 kbp side by side wait for each other's general
        // steps two thirds of the time (config 0: 1.35 s with 8 reads per wavefront on 125 of 3072 wavefronts).  The arena
        // slices stay what they are: slot = wavefront x groups_per_wave + group.
        const uint64_t resident_waves = (uint64_t)pl.cus * waves_per_cu(*pl.grp);
        const uint64_t busy = std::min<uint64_t>(count, std::max<uint64_t>(1, items));
        const uint64_t want_gpw = std::min<uint64_t>(8, std::max<uint64_t>(1, (busy + resident_waves - 1) / resident_waves));
        gpw = gpw_opt >= 0 ? (uint32_t)std::min(8, gpw_opt) : (want_gpw < 8 ? (uint32_t)want_gpw : 0u);
        // One read per wavefront: the 64-lane instantiation (mgx_ext64.hip) — the read has the wavefront to itself, so it may as
        // well use all of its lanes.  (Option ext64=0: the 8-lane groups all the same.)
        if (A->opt.ext64 != 0 && gpw == 1) b = &g_ext_builds[EXT_EXT64];
    }
    if (b->launch_64) {
        lds = lds_per_read(Lmax, waves_per_cu(*b), b->static_lds(), 128u);
    } else {
        lds = lds_per_read(Lmax, waves_per_cu(*b), b->static_lds(), 64u, 8);
        if (!pl.labeled) lds = std::min<uint32_t>(lds, probe_env_u32("MGX_EXT_LDS_CAP", lds)) & ~15u;   // tuning probe
    }
    pl.P.groups_per_wave = gpw;
    A->kernels_ran |= b->kernel_bit;
    if (b->counter != CNT_NONE) ++g_kernel_launches[b->counter];
    // (8-lane builds: a partial last wavefront is fine, the kernel returns for slot >= n_groups)
    return b->launch_64 ? b->launch_64(&pl.P, count, lds, A->hstream) : b->launch_grp(&pl.P, count, lds, PH_EXTEND, A->hstream);
}

// The passes of the multi-pass extension (choose_multi_pass): launch, count the reads that want another pass, sort their
// retry positions by the work of their next seed, again.
static int extend_multi_pass(mgx_aligner *A, AlignPlan &pl) {
    AlignParams &P = pl.P;
    const uint64_t n = pl.n;
    const uint32_t rb = resume_rec_bytes(A->lim, (uint32_t)std::max<uint64_t>(1, A->cfg.num_alternative_paths));
    size_t fb = 0, tb = 0;
    HIP_TRY(hipMemGetInfo(&fb, &tb));
    fb += g_pool.held_bytes();
    const uint64_t have = A->resume_pool[0].bytes + A->resume_pool[1].bytes;
    uint64_t cap = std::min<uint64_t>(n, ((uint64_t)fb / 2 + have) / (2ull * rb));      // two pools
    if (cap > 0xFFFFFFF0ull) cap = 0xFFFFFFF0ull;
    if (A->opt.resume_cap >= 0) cap = std::min<uint64_t>(cap, (uint64_t)A->opt.resume_cap);      // (option resume_cap: fewer records than that)
    if (cap == 0) {               // (no room for resume records: every seed of a read in one launch)
        HIP_TRY((hipError_t)launch_extension(A, pl));
        return MGX_OK;
    }
    for (int b = 0; b < 2; ++b) {
        if (int rc = A->resume_pool[b].ensure(cap * rb, true)) return rc;
        if (int rc = A->retry_key[b].ensure(n * 4 + 4)) return rc;
    }
    if (int rc = A->retry_list2.ensure(n * 4 + 4)) return rc;
    DevBuf *lists[2] = { &A->retry_list, &A->retry_list2 };
    P.resume_rec_bytes = rb; P.resume_cap = (uint32_t)cap;
    P.retry_count = cursor(A, CUR_RETRY);
    P.resume_in = nullptr; P.resume_reads = nullptr;
    int out = 0;
    for (uint32_t pass = 0;; ++pass) {
        P.resume_out = A->resume_pool[out].as<uint8_t>();
        P.retry_list = lists[out]->as<uint32_t>();
        P.retry_key = A->retry_key[out].as<uint32_t>();
        P.seed_limit = multi_pass_seed_limit(pass);
        HIP_TRY((hipError_t)launch_extension(A, pl));
        unsigned long long c = 0;
        HIP_TRY(copy_sync(A, &c, cursor(A, CUR_RETRY), 8, hipMemcpyDeviceToHost));     // (synchronises with the pass)
        c = std::min<unsigned long long>(c, cap);
        A->n_passes = pass + 1;
        if (c == 0 || P.seed_limit == 0) break;
        // next pass: the retry positions of this one, sorted by their work key
        k_iota<<<(uint32_t)((c + 255) / 256), 256, 0, A->hstream>>>(A->order_in.as<uint32_t>(), c);
        size_t tmp_bytes = pl.sort_tmp_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(A->sort_tmp.p, tmp_bytes, A->retry_key[out].as<uint32_t>(), A->work_key_sorted.as<uint32_t>(),
                                                   A->order_in.as<uint32_t>(), A->order.as<uint32_t>(), (int)c, 0, 12, A->hstream));
        HIP_TRY(clear_cursors(A, CUR_READ, CUR_READ));
        HIP_TRY(clear_cursors(A, CUR_RETRY, CUR_RETRY));
        P.order = A->order.as<uint32_t>();
        P.n_items = c;
        P.resume_in = A->resume_pool[out].as<uint8_t>();
        P.resume_reads = lists[out]->as<uint32_t>();
        out ^= 1;
    }
    return MGX_OK;
}

// The stages of a batch up to its seeds: limits, the plan, arena and buffers, the parameter block, the two seeders.  lane: plan the
// lane-per-read extension kernel too (run_align; its scratch is taken before the arena is sized) — a handle that only seeds does not.
static int seed_stage(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax, bool lane, AlignPlan &pl) {
    {
        std::string err;
        int rc = derive_limits(A->cfg, A->have_user_lim ? &A->user_lim : nullptr, Lmax, &A->lim, &err, A->anno != nullptr, A->label_scale);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, A->graph->device));
    pl.n = n;
    pl.labeled = A->anno != nullptr;
    pl.cus = (uint32_t)prop.multiProcessorCount;
    if (lane) {
        if (int rc = plan_lane(A, pl)) return rc;
    } else {
        memset(&pl.LP, 0, sizeof(pl.LP));
        pl.key_bits = work_key_bits(n);
    }
    if (int rc = size_arena(A, pl)) return rc;
    if (int rc = size_buffers(A, pl)) return rc;
    fill_params(A, pl, d_seqs, d_offsets);
    HIP_TRY(hipEventRecord(A->ev[EV_ALIGN_BEGIN], A->hstream));
    A->kernels_ran = 0;
    A->seedlane_launched = 0;
    if (int rc = seed_by_lanes(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SEED_LANE_END], A->hstream));
    if (int rc = seed_by_waves(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SEEDED], A->hstream));
    return MGX_OK;
}

static int run_align(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax) {
    AlignPlan pl;
    if (int rc = seed_stage(A, d_seqs, d_offsets, n, Lmax, true, pl)) return rc;
    A->n_passes = 1;
    A->lane_done = 0;
    A->lane_exact = 0;
    A->lane_exact_path = A->lane_exact_sub = 0;
    memset(A->lane_hist_h, 0, sizeof(A->lane_hist_h));
    // (with the exact exit the choice of the multi-pass extension comes before the sort: the exit belongs to the lane kernel's path)
    bool multi = false;
    const bool exact = pl.lane_ok && pl.LP.exact && n;
    if (exact) { if (int rc = choose_multi_pass(A, pl, &multi)) return rc; }
    const bool by_lanes = pl.lane_ok && !multi && n;
    if (by_lanes) { if (int rc = prepare_lane(A, pl)) return rc; }
    if (by_lanes && exact) { if (int rc = exact_by_lanes(A, pl)) return rc; }
    if (int rc = sort_by_work(A, pl)) return rc;
    HIP_TRY(hipEventRecord(A->ev[EV_SORTED], A->hstream));
    if (!exact) { if (int rc = choose_multi_pass(A, pl, &multi)) return rc; }
    HIP_TRY(hipEventRecord(A->ev[EV_LANE_END], A->hstream));      // (recorded again behind the lane kernel, if it runs)
    bool all_done = false;        // every read finished in the lane kernel
    if (pl.lane_ok && !multi && n) {
        if (int rc = extend_by_lanes(A, pl, &all_done)) return rc;
    }
    if (multi) {
        if (int rc = extend_multi_pass(A, pl)) return rc;
    } else if (!all_done) {
        HIP_TRY((hipError_t)launch_extension(A, pl));
    }
    HIP_TRY(hipEventRecord(A->ev[EV_ALIGN_END], A->hstream));
    return MGX_OK;
}

// the seeding stage alone (host_state.hpp)
int run_seeding(mgx_aligner *A, const char *d_seqs, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax, uint64_t *seeds_wanted) {
    AlignPlan pl;
    if (int rc = seed_stage(A, d_seqs, d_offsets, n, Lmax, false, pl)) return rc;
    for (AlignEvent e : { EV_SORTED, EV_LANE_END, EV_ALIGN_END }) HIP_TRY(hipEventRecord(A->ev[e], A->hstream));      // (what collect_stats reads)
    A->n_passes = 0;
    A->lane_done = A->lane_exact = A->lane_exact_path = A->lane_exact_sub = 0;
    memset(A->lane_hist_h, 0, sizeof(A->lane_hist_h));
    unsigned long long wanted = 0;
    HIP_TRY(copy_sync(A, &wanted, cursor(A, CUR_SEED), 8, hipMemcpyDeviceToHost));
    *seeds_wanted = wanted;
    return MGX_OK;
}

int collect_stats(mgx_aligner *A, bool mapped, bool aligned) {
    HIP_TRY(hipStreamSynchronize(A->hstream));
    KernelStats ks, km;
    HIP_TRY(copy_sync(A, &ks, A->d_stats.p, sizeof(ks), hipMemcpyDeviceToHost));
    HIP_TRY(copy_sync(A, &km, A->d_stats_map.p, sizeof(km), hipMemcpyDeviceToHost));
    ks.rank_lines += km.rank_lines; ks.select_lines += km.select_lines; ks.bit_lines += km.bit_lines; ks.map_lines += km.map_lines;
    mgx_stats &s = A->hstats;
    memset(&s, 0, sizeof(s));
    s.n_reads = A->n_reads;
    s.n_rank_lines = ks.rank_lines; s.n_select_lines = ks.select_lines; s.n_bit_lines = ks.bit_lines;
    s.n_columns = ks.columns; s.n_extensions = ks.extensions; s.n_seeds = ks.seeds;
    s.n_map_lines = ks.map_lines; s.n_capacity_errors = ks.capacity_errors; s.n_seed_lines = ks.seed_lines;
    s.n_fast_columns = ks.fast_columns;
    s.extend_kernels = A->kernels_ran;
    s.n_lane_reads = A->lane_done;
    s.n_lane_exact_reads = A->lane_exact;
    s.n_lane_exact_path_reads = A->lane_exact_path;
    s.n_lane_exact_sub_reads = A->lane_exact_sub;
    s.n_lane_lines = ks.lane_lines; s.n_lane_columns = ks.lane_columns;
    for (int x = 0; x < 32; ++x) s.lane_bail_reads[x] = A->lane_hist_h[x];
    if (int on; aligned && A->seedlane_launched && env_int("MGX_SL_TIMERS", &on)) {
        unsigned long long t[8];
        HIP_TRY(copy_sync(A, t, A->seedlane_hist.as<unsigned long long>() + 16, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "k_seed_lane timers (cycles of lane 0, summed over the wavefronts): strands %llu masks %llu scan %llu walks %llu dust %llu ranges+enumerate %llu publish %llu wave-mates %llu\n",
                t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
    if (aligned && A->seedlane_launched) {
        unsigned long long done = 0, why[16];
        HIP_TRY(copy_sync(A, &done, cursor(A, CUR_SL_DONE), 8, hipMemcpyDeviceToHost));
        HIP_TRY(copy_sync(A, why, A->seedlane_hist.p, sizeof(why), hipMemcpyDeviceToHost));
        s.n_seed_lane_reads = done;
        for (int x = 0; x < 16; ++x) s.seed_lane_left_reads[x] = why[x];
    }
    for (int x = 0; x < 8; ++x) { s.phase_cycles[x] = ks.cyc[x]; s.extend_cycles[x] = ks.xcyc[x]; }
    float ms = 0;
    if (mapped) { HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_MAP_BEGIN], A->ev[EV_MAP_END])); s.seed_kernel_ms = ms; }
    if (aligned) {
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_ALIGN_END])); s.align_kernel_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_SEEDED])); s.seeding_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SEEDED], A->ev[EV_SORTED])); s.sort_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SORTED], A->ev[EV_ALIGN_END])); s.extend_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_SORTED], A->ev[EV_LANE_END])); s.lane_ms = ms;
        if (A->seedlane_launched) { HIP_TRY(hipEventElapsedTime(&ms, A->ev[EV_ALIGN_BEGIN], A->ev[EV_SEED_LANE_END])); s.seed_lane_ms = ms; }
    }
    return MGX_OK;
}

extern "C" {

// the device blocks kept from destroyed aligners (DevPool) go back to the driver
int mgx_device_trim(int device) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    HIP_TRY(hipSetDevice(device));
    g_pool.flush();
    HIP_TRY(hipSetDevice(cur));
    return MGX_OK;
}

int mgx_aligner_set_stream(mgx_aligner *A, void *hip_stream) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(A->graph->device));
    HIP_TRY(hipStreamSynchronize(A->hstream));              // what the handle has in flight finishes where it was issued
    if (A->own_stream) { (void)hipStreamDestroy(A->hstream); A->own_stream = false; }
    A->hstream = (hipStream_t)hip_stream;
    return MGX_OK;
}
int mgx_aligner_create_stream(mgx_aligner *A) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(A->graph->device));
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (int rc = mgx_aligner_set_stream(A, st)) { (void)hipStreamDestroy(st); return rc; }
    A->own_stream = true;
    return MGX_OK;
}
void *mgx_aligner_get_stream(const mgx_aligner *A) { return A ? (void *)A->hstream : nullptr; }

int mgx_aligner_set_pipeline(mgx_aligner *A, const char *name) {
    if (!A) return fail(MGX_ERR_INVALID, "null argument");
    if (!name) return fail(MGX_ERR_INVALID, "unknown pipeline '(null)'");
    // "+general" / "+chain" suffix-free test switches: the extension's register-resident chain path off / on
    if (!strcmp(name, "general")) { A->no_fast = true; return MGX_OK; }
    if (!strcmp(name, "chain")) { A->no_fast = false; return MGX_OK; }
    if (strchr(name, '=')) {
        const std::string key(name, strchr(name, '=') - name);
        const int v = atoi(strchr(name, '=') + 1);
        mgx_aligner::Options &o = A->opt;
        if (key == "ext64") o.ext64 = v;
        else if (key == "groups_per_wave") o.groups_per_wave = std::min(8, v);
        else if (key == "multi_pass") o.multi_pass = v;
        else if (key == "resume_cap") o.resume_cap = std::max(-1, v);
        else if (key == "no_compact") o.no_compact = v;
        else if (key == "decode_on_device") o.decode_on_device = v != 0;
        else if (key == "no_alias") o.no_alias = v;
        else if (key == "no_bt_runs") o.no_bt_runs = v;
        else if (key == "no_flat") o.no_flat = v;
        else if (key == "lane") o.lane = v;
        else if (key == "exact") {
            if (v < -1 || v > 3) return fail(MGX_ERR_INVALID, "unknown option '%s'", name);
            o.exact = v;
        }
        else if (key == "device_share") o.device_share = std::max(1, std::min(v, 64));
        else if (key == "map_pipe") o.map_pipe = v;
        else if (key == "seed_wps") o.seed_wps = v;
        else if (key == "seed_lane") {
            if (v < -1 || v > 1) return fail(MGX_ERR_INVALID, "unknown option '%s'", name);
            o.seed_lane = v;
        }
        else if (key == "retry_capacity") A->retry_capacity = v != 0;
        else return fail(MGX_ERR_INVALID, "unknown option '%s'", name);
        return MGX_OK;
    }
    // (the one pipeline there is, see the top of this file: its name selects nothing)
    if (strcmp(name, "split8")) return fail(MGX_ERR_INVALID, "unknown pipeline '%s'", name);
    return MGX_OK;
}


// kernels only; results stay in HBM
int mgx_align_batch_device(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int on_device) {
    if (!A || !seqs || !offsets) return fail(MGX_ERR_INVALID, "null argument");
    if (int rc = refuse_chainer(A, "mgx_align_batch_device")) return rc;
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    const char *d_seqs; const uint64_t *d_offsets; uint32_t Lmax;
    if (n == 0) { A->n_reads = 0; A->aligned_empty = true; return MGX_OK; }
    A->aligned_empty = false;
    { HostStageTimer t("stage_batch"); if (int rc = stage_batch(A, seqs, offsets, n, on_device, &d_seqs, &d_offsets, &Lmax)) return rc; }
    A->last_d_seqs = d_seqs; A->last_d_offsets = d_offsets; A->aligned_generation = A->stage_generation;
    bool mapped = A->cfg.max_seed_length >= A->graph->g.k;
    { HostStageTimer t("run_map"); if (int rc = run_map(A, d_seqs, d_offsets, n, A->dcfg.fwd_and_rc != 0, mapped, Lmax)) return rc; }
    for (;;) {
        { HostStageTimer t("run_align"); if (int rc = run_align(A, d_seqs, d_offsets, n, Lmax)) return rc; }
        { HostStageTimer t("collect_stats"); if (int rc = collect_stats(A, mapped, true)) return rc; }
        // both streams keep counting past their capacity: reads that found no room got a capacity status and the
        // stage is redone with what it asked for
        unsigned long long out_wanted = 0, seeds_wanted = 0;
        HIP_TRY(copy_sync(A, &out_wanted, cursor(A, CUR_OUT), 8, hipMemcpyDeviceToHost));
        bool again = false;
        if (out_wanted > A->out_words) { A->out_min_words = out_wanted + out_wanted / 8 + 1024; again = true; }
        HIP_TRY(copy_sync(A, &seeds_wanted, cursor(A, CUR_SEED), 8, hipMemcpyDeviceToHost));
        if (seeds_wanted > A->seed_cap) {
            A->seed_scale = seeds_wanted / std::max<uint64_t>(1, A->seed_cap / A->seed_scale) + 2;
            again = true;
        }
        if (!again) break;
    }
    A->h_results.clear();          // host copies of an earlier batch must not be mistaken for this one's
    return MGX_OK;
}


int mgx_aligner_stats(const mgx_aligner *A, mgx_stats *out) { *out = A->hstats; return MGX_OK; }
void mgx_kernel_launch_counts(uint64_t *out5) { for (int x = 0; x < 5; ++x) out5[x] = g_kernel_launches[x].load(); }

} // extern "C"
