// lane_types.hpp — what the host needs to know about the lane-per-read kernel (lane_read.hpp, mgx_lane.hip): its launch
// parameters, its scratch layout and the test of whether a batch's configuration is one the kernel takes at all.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/mgx.h"
#include "align_types.hpp"


namespace mgx {

// longest read a lane takes (packed strand in LDS: LANE_QWORDS words per lane).  The host lays the scratch out for 256, and the
// kernel is built once (mgx_lane.hip), for reads of up to 256 characters.  (MGX_LANE_MAX_L remains as a build parameter: the second
// build for batches whose longest read has at most 160 characters — a smaller packed strand, a third wavefront per SIMD — was
// measured and not kept.)
#ifndef MGX_LANE_MAX_L
#define MGX_LANE_MAX_L 256
#endif
constexpr int LANE_MAX_L = MGX_LANE_MAX_L;
constexpr int LANE_MAX_L_HOST = 256;       // what the scratch layout is sized for, whichever build runs
constexpr int LANE_QWORDS = LANE_MAX_L / 32 + 2;
constexpr int LANE_MAX_RUNS = 16;          // CIGAR runs of a trace kept in LDS
constexpr int LANE_MAX_SEEDS = 512;        // seeds of the strand (the later ones are checked against the extension one by one)
constexpr int LANE_SLOT_WORDS = 12;        // per column: 8 flag words (32 cells, a byte each) + node + base + geometry + link
constexpr int LANE_WAVE = 64;              // lanes whose column slots and S rows are interleaved word by word (below)
constexpr int LANE_MAX_DEFER = 3;          // columns that may stay behind in the frontier (the other children of forks)
constexpr int LANE_DSLOT_WORDS = 80;       // a column that stays behind: its window (64 words) + nine words of column state
constexpr uint32_t LANE_GEOM_ROW = 1u << 31;   // in a slot's geometry word: the column's S row was written
constexpr int LANE_S8_FILTER_SEEDS = 16;   // later seeds whose last nodes select the columns that keep their S row (more: every column does)
constexpr int LANE_S8_WORDS = 8;           // per column: S of the window as 8-bit offsets from `base` (read at the trace's end only)

// what one launch of the lane kernel needs on top of AlignParams
struct LaneParams {
    AlignParams P;
    const uint64_t *pk[2];               // 2-bit packed strands (k_pack_reads): word j of read r at packed_word_begin(offsets[r], r) + j
    const uint32_t *iv[2];               // invalid-character flags, same indexing
    // Scratch of a resident wavefront (round 6: wave-interleaved).  The 64 lanes of a wavefront step their columns in lock-step —
    // lane_read() starts every lane at column 1 and each loop iteration commits one — so the column slots and S rows are laid
    // out [column][word][lane]: the store of "word w of column c" by the 64 lanes is 256 contiguous bytes (four full lines)
    // where lane-private slices made it 64 partial-line writes 18 KB apart, and the trace's reads of a column's words find
    // the lanes' words in the same lines.  What is addressed by a lane's own data (the node table) or touched rarely (parked
    // windows, the forward alignment during a backward pass, counters) stays in a private slice per lane behind them:
    //   wave w:  [ slots: max_cols x LANE_SLOT_WORDS x 64 words | S rows: max_cols x LANE_S8_WORDS x 64 words
    //              | CIGAR runs of the trace: LANE_MAX_RUNS x 64 words | 64 x rest_stride bytes ]
    uint8_t *scratch;
    uint64_t wave_stride;                // bytes per wavefront (lane_wave_scratch_bytes)
    uint64_t rest_stride;                // bytes of a lane's private slice (lane_rest_bytes, rounded to 64)
    uint32_t max_cols;                   // columns a lane's scratch holds (lane_max_cols)
    uint32_t hash_slots;                 // power of two >= 2 * max_cols
    uint32_t tag_seed;                   // changes per launch (node-table entries of earlier launches read as empty)
    uint32_t t4[4];                      // score_matrix[c][q] for c, q in ACGT: row c as four bytes (q = A in the low byte)
    int32_t self_score;                  // score(A, A) == ... == score(T, T) > 0 (else the kernel is not launched)
    uint32_t *bail_list;                 // reads for the group kernel, in processing order
    unsigned long long *bail_count;
    unsigned long long *done_count;
    unsigned long long *bail_hist;       // [32] reads passed on, by the LANE_BAIL code of the test that sent them (lane_read.hpp);
                                         // [LANE_HIST_EXACT] reads finished through the exact exit (part of *done_count, which is
                                         // what the host reads; the word is there for probes of a launch's counters);
                                         // [LANE_HIST_EXACT_PATH] those of them without a spanning first seed (the path class);
                                         // [LANE_HIST_EXACT_SUB] those of them k_lane_exact_sub finished (the substitution class);
                                         // [LANE_HIST_SUB_CAND] the entries of sub_list
    // (behind what k_lane reads, whose offsets stay what they were)
    uint32_t exact;                      // the level of the exact exit (lane_read.hpp; only where lane_exact_config() holds).  1: a read whose
                                         // first seed spans the query is finished without DP; 2: also a read whose first seed starts at
                                         // the query's first character and whose every k-mer is a node (the path class); 3: also a read
                                         // with one substitution behind its first k characters (the substitution class, under
                                         // lane_exact_sub_config() only; label-aware: the read keeps one label along the walked nodes
                                         // too).  0 by default: every read runs its columns
    uint32_t done_key;                   // exact, on the device: the work key k_lane_exact gives the reads it finished — above every
                                         // key of the seeding phase, so that the work sort puts them behind the items k_lane is launched on
    struct LaneSubCand *sub_list;        // exact >= 3: the reads that passed the header tests and have one run of zeros in their node
                                         // array, listed by k_lane_exact for k_lane_exact_sub (bail_hist[LANE_HIST_SUB_CAND] of them);
                                         // label-aware batches: LaneSubCandLabeled records at the same address, listed by
                                         // k_lane_exact_labeled for k_lane_exact_sub_labeled
};
// a candidate of the substitution class: the read, the strand aligned, the run of zeros [lo, hi] in that strand's node array
struct alignas(16) LaneSubCand { uint32_t read, strand, lo, hi; };
// ... of a label-aware batch (k_lane_exact_labeled lists, k_lane_exact_sub_labeled reads; the same buffer, a record type of its own):
// also what the one-label seed filter found, which gathered the seeds' rows for it and is not run a second time — the read's
// label, and num_matching and the seed counts of both strands as the filter left them (the result record's)
struct alignas(16) LaneSubCandLabeled { uint32_t read, strand, lo, hi, label, nm[2], ns[2], pad[3]; };
static_assert(sizeof(LaneSubCandLabeled) == 48, "three 16-byte loads");
constexpr int LANE_HIST_EXACT = 48;        // (bail_hist has 64 words; [32 .. 41] are the section timers of -DMGX_LANE_TIMERS builds)
constexpr int LANE_HIST_EXACT_PATH = 49;
constexpr int LANE_HIST_EXACT_SUB = 50;
constexpr int LANE_HIST_SUB_CAND = 51;
constexpr int LANE_SUB_MAX_WALK = 32;      // nodes a walk across a substitution makes at most: k <= 32 (lane_enabled)

// columns of an extension along one path: the root, one per query character, the deletions past the query's end that the x-drop
// still allows, the spare slot of the `size >= capacity - 1` test (a read that needs more goes to the group kernel)
inline uint32_t lane_max_cols(uint32_t Lmax, int32_t xdrop) {
    return Lmax + (uint32_t)std::min<int64_t>(Lmax, std::max<int64_t>(xdrop, 0)) + 8;
}

// a lane's private slice: node table | two parked windows (S, F of 32 cells each; one unused) | the forward alignment while the
// backward pass runs (nodes, character codes, CIGAR runs) | the result's scalars and counters | the merged vector of a replayed
// node | the columns that stayed behind in the frontier
inline uint64_t lane_rest_bytes(uint32_t max_cols, uint32_t hash_slots) {
    return (uint64_t)hash_slots * 8 + 2 * 2 * 32 * 4
           + (uint64_t)max_cols * 8 + LANE_MAX_RUNS * 4 + 32 * 4 + (uint64_t)(LANE_MAX_L_HOST + 8) * 4
           + (uint64_t)LANE_MAX_DEFER * LANE_DSLOT_WORDS * 4;
}
inline uint64_t lane_slots_bytes(uint32_t max_cols) { return (uint64_t)max_cols * LANE_SLOT_WORDS * LANE_WAVE * 4; }
inline uint64_t lane_s8_bytes(uint32_t max_cols) { return (uint64_t)max_cols * LANE_S8_WORDS * LANE_WAVE * 4; }
inline uint64_t lane_runs_bytes() { return (uint64_t)LANE_MAX_RUNS * LANE_WAVE * 4; }
inline uint64_t lane_wave_scratch_bytes(uint32_t max_cols, uint64_t rest_stride) {
    return lane_slots_bytes(max_cols) + lane_s8_bytes(max_cols) + lane_runs_bytes() + (uint64_t)LANE_WAVE * rest_stride;
}


// Whether the exact exit (lane_read.hpp lane_exact(), mgx_lane.hip k_lane_exact) may be on, given that lane_enabled() holds: the conditions, beyond lane_enabled()'s, under
// which a read whose first seed spans the query has the all-match alignment over the seed's nodes as its one result, with the score
// m L + left_end_bonus + right_end_bonus (DESIGN.md 3.4 "the exact exit").  What depends on the read's length — min_path_score
// and min_cell_score against that score — is tested per read in lane_exact().  The path class of level 2 (first seed at the query's
// first character, every k-mer of the strand a node) stands on the same conditions: past the seed's end the strand's next node is
// the one child that scores a match, so the first two items carry the fork argument from "inside the seed" to "along the path".
//  - every mismatch scores strictly below a match and a gap strictly below 0: no second alignment reaches the full score, and at a
//    fork the all-match child is the only top of the extender's queue (no tie for the order of equal columns to resolve);
//  - right_end_bonus >= 0: an alignment that stops short of the query's end cannot score above the full one;
//  - xdrop >= 0: the cell that holds the best score so far never falls under the x-drop cut-off;
//  - max_nodes_per_seq_char and max_ram_per_alignment need no condition: extend() tests them only for a column whose maximum is
//    below the best score so far (aligner_extender_methods.cpp:521-547), which the all-match head never is;
//  - label-aware (labeled_flags: AlignParams::labeled): only with bit 1, no dummy node's row holds a label, as the lane itself.  The
//    exit then takes the reads that keep one label all along: the one-label seed filter leaves a label L, and every node of the
//    path has the row { L } (lane_exact_class(), DESIGN.md 3.4 "label-aware batches"); side branches carry a mismatch or a gap
//    whatever their labels, so the argument above stands with { L } behind the alignment.
inline bool lane_exact_config(const mgx_config &c, const DevConfig &d, uint32_t labeled_flags) {
    if ((labeled_flags & 1u) && !(labeled_flags & 2u)) return false;
    const char acgt[4] = { 'A', 'C', 'G', 'T' };
    const int m = c.score_matrix[(int)'A'][(int)'A'];
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y)
            if (x != y && c.score_matrix[(int)acgt[x]][(int)acgt[y]] >= m) return false;
    if (c.gap_opening_penalty >= 0) return false;
    if (c.right_end_bonus < 0 || d.right_end_bonus < 0) return false;
    if (c.xdrop < 0) return false;
    return true;
}

// Whether level 3 of the exact exit (the substitution class, lane_read.hpp lane_exact_sub()) may be on, given lane_exact_config():
// the conditions that make the alignment with one mismatch at p — score m (L - 1) + mm + both end
// bonuses, mm the score of the graph's character against the read's — the strict optimum AND what extend() finds (DESIGN.md 3.4
// "the substitution class").  Label-aware batches under lane_exact_config()'s label condition: LabeledExtender only takes
// alternatives away from the plain extender where every node of the path has the row { L } (DESIGN.md 3.4 "the substitution
// class, label-aware").  With lo / hi the smallest / largest score off the matrix' diagonal:
//  - gap_opening_penalty + m < lo: an alignment with a gap, every other character matched, scores below one mismatch (the deletion
//    of one graph character inside a homopolymer matches all L characters: m L + gap_opening);
//  - 2 hi - lo < m: two mismatches score below one;
//  - hi - lo < m: a child parked at a fork in front of p, with its own mismatch, stays below the head behind p;
//  - lo + xdrop >= 0: the x-drop does not cut the head at the mismatch.
// What depends on the read (the thresholds, strictness against stopping in front of p, the extension cut-off of rel_score_cutoff,
// max_nodes_per_seq_char and max_ram_per_alignment, which ARE tested while the head runs below the best score) is in lane_exact_sub().
inline bool lane_exact_sub_config(const mgx_config &c, const DevConfig &d, uint32_t labeled_flags) {
    if (!lane_exact_config(c, d, labeled_flags)) return false;
    const char acgt[4] = { 'A', 'C', 'G', 'T' };
    const int m = c.score_matrix[(int)'A'][(int)'A'];
    int lo = m, hi = -128;
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y)
            if (x != y) { const int v = c.score_matrix[(int)acgt[x]][(int)acgt[y]]; lo = std::min(lo, v); hi = std::max(hi, v); }
    if (!((int64_t)c.gap_opening_penalty + m < lo)) return false;
    if (!(2 * hi - lo < m) || !(hi - lo < m)) return false;
    if (!((int64_t)lo + c.xdrop >= 0)) return false;
    return true;
}
// the level the exit runs at when `level` is asked for: 3 falls back to 2 where only lane_exact_config() holds
inline uint32_t lane_exact_level(const mgx_config &c, const DevConfig &d, uint32_t labeled_flags, uint32_t level) {
    if (!level || !lane_exact_config(c, d, labeled_flags)) return 0u;
    return level >= 3u ? (lane_exact_sub_config(c, d, labeled_flags) ? 3u : 2u) : level;
}

// whether the automatic default of the exact exit (option exact absent) extends to label-aware batches: decided by measurement —
// four alternating pairs on BASELINE config 3 put the range with the exit wholly above the range without it
// (profiles/r09_exact_labels_ab_pairs.txt; README.md, "And the label-aware batches")
constexpr bool LANE_EXACT_AUTO_LABELED = true;
// whether the automatic default for unlabeled batches is level 3 (the substitution class) instead of 2: decided by measurement —
// four alternating pairs against the parent commit put the range at level 3 wholly above the parent's, 17.17 - 17.38 against
// 15.69 - 15.81 x 10^6 reads/s (profiles/r10_exact_sub_ab_pairs.txt).
constexpr bool LANE_EXACT_AUTO_SUB = true;
// ... and whether the automatic default for label-aware batches is level 3 as well (k_lane_exact_sub_labeled) instead of 2: by the
// same rule, on BASELINE config 3 against the parent commit (profiles/r11_exact_sub_labels_ab_pairs.txt)
constexpr bool LANE_EXACT_AUTO_SUB_LABELED = true;

// Whether the lane-per-read kernel may run in front of the group kernel for this configuration (every read it cannot finish
// goes to the group kernel anyway; this only rules out configurations in which its shortcuts would not be exact or no read
// could finish), and the scoring constants it runs with.  `why`: the first reason against.
// labeled: label-aware alignment (LabeledAligner); labeled_flags: AlignParams::labeled — bit 1 must be set (no dummy node's row holds
// a label: the lane reads rows without the W test)
inline bool lane_enabled(const mgx_config &c, const DevConfig &d, uint32_t k, uint32_t Lmax, bool no_fast, LaneParams *LP, std::string *why,
                         uint32_t labeled_flags = 0) {
    auto no = [&](const char *w) { if (why) *why = w; return false; };
    if ((labeled_flags & 1u) && !(labeled_flags & 2u)) return no("label-aware: rows of dummy nodes hold labels");
    if (d.num_alt != 1 || d.post_chain) return no("alternative paths");
    if (d.canonical != 0) return no("CANONICAL / PRIMARY graph");
    if (k > 32 || k < 2) return no("k > 32: reads are not 2-bit packed");
    if (Lmax < 1 || Lmax > (uint32_t)LANE_MAX_L_HOST) return no("reads longer than a lane takes");
    if (no_fast || c.xdrop > 30000) return no("chain path off");
    if (d.branch_xdrop) return no("per-branch x-drop (global_xdrop = 0): the lane kernels encode the global rule");
    const char acgt[4] = { 'A', 'C', 'G', 'T' };
    const int m = c.score_matrix[(int)'A'][(int)'A'];
    if (m <= 0) return no("match score");
    for (int x = 0; x < 4; ++x) {
        if (c.score_matrix[(int)acgt[x]][(int)acgt[x]] != m) return no("match scores differ");
        uint32_t row = 0;
        for (int y = 0; y < 4; ++y) {
            const int v = c.score_matrix[(int)acgt[x]][(int)acgt[y]];
            if (v > m) return no("a mismatch scores above a match");
            row |= (uint32_t)(uint8_t)(int8_t)v << (8 * y);
        }
        LP->t4[x] = row;
    }
    if (c.gap_opening_penalty > 0 || c.gap_extension_penalty > 0) return no("positive gap scores");
    if (c.left_end_bonus < 0) return no("negative left end bonus");
    if (!(c.rel_score_cutoff >= 0.0 && c.rel_score_cutoff <= 1.0)) return no("rel_score_cutoff outside [0, 1]");
    LP->self_score = m;
    // (the host model: MGX_EMU_LANE_EXACT=1 / 2 / 3 sets the exact exit's level where the configuration allows it; the product's
    // plan_lane() decides by its own rule and overwrites this)
    const char *ex = std::getenv("MGX_EMU_LANE_EXACT");
    const uint32_t level = (ex && *ex >= '1' && *ex <= '3' && !ex[1]) ? (uint32_t)(*ex - '0') : 0u;
    LP->exact = lane_exact_level(c, d, labeled_flags, level);
    LP->sub_list = nullptr;
    return true;
}

} // namespace mgx
