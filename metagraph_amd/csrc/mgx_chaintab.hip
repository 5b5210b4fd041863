// mgx_chaintab.hip — the chain stage of LabeledAligner's coordinate mode as one device pipeline (mgx_seed_chainer_create,
// mgx_chain_tables_batch; include/mgx.h): from the seeds the seeding kernels left (SeedHdr / DevSeed) to the filtered seeds and
// the finished tables of chain_seeds for every (query, strand), all of it resident in device memory.
//
//   filter_seeds with coordinates (A/aligner_labeled.cpp:594-721)        k_chtab_pair_count -> scan -> k_chtab_pair_write -> segmented sort
//                                                                        -> k_chtab_labels -> k_chtab_seed_count -> scans
//   the anchors, one per (seed, label, coordinate) (A/aligner_chainer.cpp:341-381)        k_chtab_emit
//   the sort and the banded DP (:383-542)                                three segmented radix passes -> k_chtab_permute -> k_chtab_chain_dp
//
// A list = one (query, strand); one wavefront takes one list in every kernel but the element-wise ones.  Nothing is bounded by an
// arena: the labels a list's seeds carry are found by sorting its (seed, label) pairs — key (label, first covered position),
// value the end of the covered range — so that a label's covered positions are the union of a run of intervals sorted by their
// begin, which a segmented scan measures; every output is counted, scanned and then written.  The DP keeps the scores and back
// pointers of a sliding window of anchors in LDS (anchor i only touches the 64 entries behind it), so a list may be as long as
// memory allows — mgx_chain_seeds (mgx_chain.hip) keeps whole lists in LDS and its limit.
#include <hip/hip_runtime.h>
#include "pack_swar.hpp"
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <cmath>

#define MGX_NO_EXTEND 1      // the graph primitives only (get_W: is a seed's first node a dummy node?)
#include "dev_graph.hpp"
#include "host_state.hpp"
#include "kernel_units.hpp"

using namespace mgx;

namespace {

constexpr uint32_t kNid = 0xFFFFFFFFu;
constexpr uint32_t CT_WAVES = 4;                // lists per workgroup of the wavefront-per-list kernels
constexpr uint32_t CT_NO_LABEL = 0xFFFFFFFFu;   // (labels are below 2^24: mgx_annotation_create)
constexpr uint32_t CT_RING = 256;               // window slots of the DP: anchors [i - 64, i + 128] are live at step i

// what the kernels read: the seeding stage's product, the reads' lengths, the annotation
struct CtIn {
    DevGraph g;
    const SeedHdr *hdr;
    const DevSeed *seed_stream;
    const uint64_t *offsets, *node_begin;
    const uint32_t *nodes[2];
    const uint64_t *anno_head;
    const uint32_t *anno_count, *anno_more;
    uint64_t anno_rows;
    const uint64_t *row_entry, *coord_off;
    const int64_t *coords;
    uint64_t n_lists, max_per_locus;
    double min_exact_match;
    uint32_t dummy_clean;                       // no row of a dummy node holds a label: the row is read without the W test
};

struct CtList { const DevSeed *seeds; const uint32_t *nodes; uint32_t n, L, num_matching; int32_t status; };
struct CtRow { uint32_t n, one; const uint32_t *more; uint64_t entry; };

__device__ inline int ct_lane() { return (int)(threadIdx.x & 63); }
__device__ inline uint64_t ct_list_index() { return (uint64_t)blockIdx.x * CT_WAVES + (threadIdx.x >> 6); }

__device__ inline CtList ct_list(const CtIn &in, uint64_t l) {
    const uint64_t q = l >> 1;
    const int s = (int)(l & 1);
    const SeedHdr h = in.hdr[q];
    CtList r;
    r.L = (uint32_t)(in.offsets[q + 1] - in.offsets[q]);
    r.status = h.status;
    r.n = h.status == ST_OK ? h.n_seeds[s] : 0u;
    r.num_matching = h.status == ST_OK ? h.num_matching[s] : 0u;
    r.seeds = in.seed_stream + h.off + (s ? h.n_seeds[0] : 0);
    r.nodes = in.nodes[s] + in.node_begin[q];
    return r;
}

// the labels of a seed's first node as AnnotationBuffer hands them out: none for a dummy node (W == 0) whatever its row says
__device__ inline CtRow ct_row(const CtIn &in, const CtList &lst, const DevSeed &sd) {
    CtRow r;
    r.n = 0; r.one = 0; r.more = nullptr; r.entry = 0;
    const uint32_t node0 = sd.offset == 0 ? lst.nodes[sd.clipping] : sd.node;
    if (!node0 || node0 > in.g.n || (uint64_t)node0 - 1 >= in.anno_rows) return r;
    if (!in.dummy_clean) {
        LineCtr lc = { 0, 0, 0 };
        if (get_W(in.g, node0, lc) == 0) return r;
    }
    const uint64_t row = (uint64_t)node0 - 1, head = in.anno_head[row];
    uint32_t c = (uint32_t)(head & 0xFFFF);
    if (c == 0xFFFF) c = in.anno_count[row];
    r.n = c; r.one = (uint32_t)(head >> 16);
    r.more = c >= 2 ? in.anno_more + (head >> 16) : nullptr;
    r.entry = in.row_entry[row];
    return r;
}
__device__ inline uint32_t ct_row_at(const CtRow &r, uint32_t x) { return r.n == 1 ? r.one : r.more[x]; }

// exclusive prefix sums over the wavefront; *total: the sum of all 64 lanes
__device__ inline uint32_t ct_scan(uint32_t v, uint32_t *total) {
    const int lane = ct_lane();
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    *total = __shfl(inc, 63);
    return inc - v;
}
__device__ inline uint32_t ct_wave_sum(uint32_t v) { uint32_t t; (void)ct_scan(v, &t); return t; }

__device__ inline bool ct_is_kept(const uint32_t *kept, uint32_t nk, uint32_t label) {
    uint32_t lo = 0, hi = nk;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (kept[mid] < label) lo = mid + 1; else hi = mid;
    }
    return lo < nk && kept[lo] == label;
}

// ---- filter_seeds, first half: the (seed, label) pairs of every list ----
__global__ void __launch_bounds__(64 * CT_WAVES) k_chtab_pair_count(CtIn in, uint64_t *pair_cnt, uint32_t *qsize, int32_t *status) {
    const uint64_t l = ct_list_index();
    if (l >= in.n_lists) return;
    const CtList lst = ct_list(in, l);
    uint32_t c = 0;
    for (uint32_t i = (uint32_t)ct_lane(); i < lst.n; i += 64) c += ct_row(in, lst, lst.seeds[i]).n;
    c = ct_wave_sum(c);
    if (ct_lane() == 0) {
        pair_cnt[l] = c;
        qsize[l] = lst.L;
        if (!(l & 1)) status[l >> 1] = lst.status == ST_OK ? MGX_OK : MGX_ERR_CAPACITY;
    }
}

// key = label << 16 | first covered query position, value = the end of the covered range [clipping, clipping + k - offset)
__global__ void __launch_bounds__(64 * CT_WAVES) k_chtab_pair_write(CtIn in, const uint64_t *pair_begin, uint64_t *keys, uint32_t *vals) {
    const uint64_t l = ct_list_index();
    if (l >= in.n_lists) return;
    const CtList lst = ct_list(in, l);
    uint64_t at = pair_begin[l];
    for (uint32_t base = 0; base < lst.n; base += 64) {
        const uint32_t i = base + (uint32_t)ct_lane();
        DevSeed sd = {};
        CtRow r;
        r.n = 0;
        if (i < lst.n) { sd = lst.seeds[i]; r = ct_row(in, lst, sd); }
        uint32_t total;
        const uint64_t o = at + ct_scan(r.n, &total);
        const uint32_t lo = sd.clipping, hi = min((uint32_t)sd.clipping + in.g.k - (uint32_t)sd.offset, lst.L);
        for (uint32_t x = 0; x < r.n; ++x) {
            keys[o + x] = ((uint64_t)ct_row_at(r, x) << 16) | lo;
            vals[o + x] = hi;
        }
        at += total;
    }
}

// The sorted pairs of a list: a label's pairs are one run, ordered by the begin of their ranges, so the positions a label covers
// are sum over the run of max(0, end - max(begin, the largest end before it in the run)) — two segmented scans per 64 pairs,
// carried from chunk to chunk.  Labels at or above the cut-off (aligner_labeled.cpp:642-664) are listed, ascending.
__global__ void __launch_bounds__(64 * CT_WAVES) k_chtab_labels(CtIn in, const uint64_t *pair_begin, const uint64_t *keys, const uint32_t *vals,
                                                            uint32_t *kept, uint32_t *n_kept) {
    const uint64_t l = ct_list_index();
    if (l >= in.n_lists) return;
    const int lane = ct_lane();
    const uint64_t b0 = pair_begin[l], T = pair_begin[l + 1] - b0;
    const uint32_t L = (uint32_t)(in.offsets[(l >> 1) + 1] - in.offsets[l >> 1]);
    const double cutoff = in.min_exact_match * (double)L;
    uint32_t c_label = CT_NO_LABEL, c_max = 0, c_sum = 0, nk = 0;
    for (uint64_t base = 0; base < T; base += 64) {
        const uint64_t idx = base + (uint64_t)lane;
        const bool valid = idx < T;
        const uint64_t key = valid ? keys[b0 + idx] : 0;
        const uint32_t lab = valid ? (uint32_t)(key >> 16) : CT_NO_LABEL - 1, lo = (uint32_t)(key & 0xFFFF), hi = valid ? vals[b0 + idx] : 0;
        const uint32_t next_lab = idx + 1 < T ? (uint32_t)(keys[b0 + idx + 1] >> 16) : CT_NO_LABEL;
        // inclusive maximum of the ends over the lanes of the same label up to this one
        uint32_t mx = hi;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ol = __shfl_up(lab, d), om = __shfl_up(mx, d);
            if (lane >= d && ol == lab) mx = max(mx, om);
        }
        if (lab == c_label) mx = max(mx, c_max);
        const uint32_t p_lab = __shfl_up(lab, 1), p_mx = __shfl_up(mx, 1);
        const uint32_t before = (lane > 0 && p_lab == lab) ? p_mx : (lab == c_label ? c_max : 0u);
        const uint32_t from = max(lo, before);
        uint32_t sum = hi > from ? hi - from : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ol = __shfl_up(lab, d), os = __shfl_up(sum, d);
            if (lane >= d && ol == lab) sum += os;
        }
        if (lab == c_label) sum += c_sum;
        const bool keep = valid && next_lab != lab && !((double)sum < cutoff);
        const uint64_t km = __ballot(keep);
        if (keep) kept[b0 + nk + (uint32_t)__popcll(km & ((1ull << lane) - 1))] = lab;
        nk += (uint32_t)__popcll(km);
        c_label = __shfl(lab, 63); c_max = __shfl(mx, 63); c_sum = __shfl(sum, 63);
    }
    if (lane == 0) n_kept[l] = nk;
}

// a seed after the filter: the kept labels of its first node's row and the anchors they give (one per coordinate, at most
// max_num_seeds_per_locus per label)
__device__ inline uint32_t ct_seed_kept(const CtIn &in, const CtRow &r, const uint32_t *kept, uint32_t nk, uint32_t *anchors) {
    uint32_t kl = 0, an = 0;
    for (uint32_t x = 0; x < r.n && nk; ++x) {
        if (!ct_is_kept(kept, nk, ct_row_at(r, x))) continue;
        ++kl;
        const uint64_t e = r.entry + x;
        an += (uint32_t)min(in.coord_off[e + 1] - in.coord_off[e], in.max_per_locus);
    }
    *anchors = an;
    return kl;
}

// ---- filter_seeds, second half (size pass): the kept seeds, their nodes and anchors, num_matching ----
// get_num_char_matches_in_seeds (alignment.hpp:100-127) incl. its quirk: nothing behind the first sub-k seed is counted
__global__ void __launch_bounds__(64 * CT_WAVES) k_chtab_seed_count(CtIn in, const uint64_t *pair_begin, const uint32_t *kept_all, const uint32_t *n_kept,
                                                                uint64_t *seed_cnt, uint64_t *node_cnt, uint64_t *anchor_cnt, uint64_t *num_matching) {
    const uint64_t l = ct_list_index();
    if (l >= in.n_lists) return;
    const int lane = ct_lane();
    const CtList lst = ct_list(in, l);
    const uint32_t *kept = kept_all + pair_begin[l];
    const uint32_t nk = n_kept[l];
    uint32_t m = 0, nn = 0, na = 0, nm = 0, last_end = 0;
    bool counting = true;
    for (uint32_t base = 0; base < lst.n; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        DevSeed sd = {};
        uint32_t an = 0;
        bool keep = false;
        if (i < lst.n) { sd = lst.seeds[i]; keep = ct_seed_kept(in, ct_row(in, lst, sd), kept, nk, &an) != 0; }
        const uint64_t km = __ballot(keep), below = km & ((1ull << lane) - 1);
        const uint32_t qb = sd.clipping, qe = (uint32_t)sd.clipping + sd.length;
        // the query end of the kept seed before this one
        const uint32_t prev_lane_end = __shfl(qe, below ? 63 - __clzll(below) : 0);
        const uint32_t prev_end = below ? prev_lane_end : last_end;
        const uint64_t subk = __ballot(keep && sd.offset != 0);
        const int stop = subk ? __ffsll((long long)subk) - 1 : 64;                  // the first kept sub-k seed of the chunk still counts
        uint32_t c = 0;
        if (keep && counting && lane <= stop && qe > prev_end) c = (qe - qb) - (qb < prev_end ? prev_end - qb : 0u);
        nm += ct_wave_sum(c);
        m += (uint32_t)__popcll(km);
        nn += ct_wave_sum(keep ? (uint32_t)sd.n_nodes : 0u);
        na += ct_wave_sum(keep ? an : 0u);
        if (km) last_end = __shfl(qe, 63 - __clzll(km));
        if (subk) counting = false;
    }
    if (lane == 0) {
        seed_cnt[l] = m; node_cnt[l] = nn; anchor_cnt[l] = na;
        num_matching[l] = lst.n ? nm : lst.num_matching;
    }
}

// ---- write pass: the kept seeds in reversed order with their nodes, and their anchors in the order chain_seeds emits them ----
__global__ void __launch_bounds__(64 * CT_WAVES) k_chtab_emit(CtIn in, const uint64_t *pair_begin, const uint32_t *kept_all, const uint32_t *n_kept,
                                                          const uint64_t *seed_begin, const uint64_t *node_begin, const uint64_t *list_begin,
                                                          mgx_chain_seed *seeds_out, uint64_t *nodes_out, mgx_chain_anchor *anchors_out) {
    const uint64_t l = ct_list_index();
    if (l >= in.n_lists) return;
    const int lane = ct_lane();
    const CtList lst = ct_list(in, l);
    const uint32_t *kept = kept_all + pair_begin[l];
    const uint32_t nk = n_kept[l];
    const uint64_t sb = seed_begin[l], nb = node_begin[l], lb = list_begin[l];
    const uint32_t m = (uint32_t)(seed_begin[l + 1] - sb);
    const uint64_t n_anchors = list_begin[l + 1] - lb;
    if (!m) return;
    uint32_t pos0 = 0, node0 = 0;
    uint64_t anchor0 = 0;
    for (uint32_t base = 0; base < lst.n; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        DevSeed sd = {};
        CtRow r;
        r.n = 0;
        uint32_t an = 0;
        bool keep = false;
        if (i < lst.n) { sd = lst.seeds[i]; r = ct_row(in, lst, sd); keep = ct_seed_kept(in, r, kept, nk, &an) != 0; }
        const uint64_t km = __ballot(keep);
        uint32_t node_total, anchor_total;
        const uint32_t node_at = node0 + ct_scan(keep ? (uint32_t)sd.n_nodes : 0u, &node_total);
        const uint64_t anchor_end = anchor0 + ct_scan(keep ? an : 0u, &anchor_total) + an;      // anchors of the kept seeds up to this one
        if (keep) {
            const uint32_t pos = pos0 + (uint32_t)__popcll(km & ((1ull << lane) - 1));
            const uint32_t rev = m - 1 - pos;                       // std::reverse(seeds): seed_index counts in this order
            mgx_chain_seed o;
            o.clipping = sd.clipping; o.length = sd.length; o.offset = sd.offset; o.n_nodes = sd.n_nodes;
            o.nodes_begin = nb + node_at;
            seeds_out[sb + rev] = o;
            for (uint32_t t = 0; t < sd.n_nodes; ++t) nodes_out[nb + node_at + t] = sd.offset == 0 ? lst.nodes[sd.clipping + t] : sd.node;
            // the seeds behind this one come first in the reversed order
            uint64_t w = lb + (n_anchors - anchor_end);
            for (uint32_t x = 0; x < r.n; ++x) {
                const uint32_t label = ct_row_at(r, x);
                if (!ct_is_kept(kept, nk, label)) continue;
                const uint64_t e = r.entry + x, c0 = in.coord_off[e], c1 = in.coord_off[e + 1];
                const uint64_t take = min(c1 - c0, in.max_per_locus);
                for (uint64_t t = 0; t < take; ++t) {               // from the largest coordinate down
                    mgx_chain_anchor a;
                    a.label = label;
                    a.coordinate = in.coords[c1 - 1 - t] + (int64_t)sd.offset;      // a sub-k seed: the coordinate of its first nucleotide
                    a.seed_clipping = (int32_t)sd.clipping; a.seed_end = (int32_t)sd.clipping + (int32_t)sd.length;
                    a.chain_score = (int32_t)sd.length; a.seed_index = rev;
                    anchors_out[w++] = a;
                }
            }
        }
        pos0 += (uint32_t)__popcll(km); node0 += node_total; anchor0 += anchor_total;
    }
}

// ---- the sort of chain_seeds: (label, coordinate, seed_clipping, seed_end) descending within every list — three stable
// segmented radix passes from the least significant key up, the keys gathered through the permutation so far ----
__global__ void k_chtab_iota(uint32_t *perm, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}
__global__ void k_chtab_key_query(const mgx_chain_anchor *a, const uint32_t *perm, uint64_t n, uint32_t *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mgx_chain_anchor &e = a[perm[i]];
    keys[i] = ((uint32_t)e.seed_clipping << 16) | (uint32_t)e.seed_end;       // (both at most MGX_MAX_QUERY_LENGTH < 2^16)
}
__global__ void k_chtab_key_coord(const mgx_chain_anchor *a, const uint32_t *perm, uint64_t n, uint64_t *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = (uint64_t)a[perm[i]].coordinate ^ 0x8000000000000000ull;      // signed: the sign bit flipped gives the unsigned order
}
__global__ void k_chtab_key_label(const mgx_chain_anchor *a, const uint32_t *perm, uint64_t n, uint32_t *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = (uint32_t)a[perm[i]].label;
}
__global__ void k_chtab_permute(const mgx_chain_anchor *a, const uint32_t *perm, uint64_t n, mgx_chain_anchor *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[perm[i]];
}

// ---- the banded DP of chain_seeds (:383-542), one wavefront per sorted list: anchor i offers itself to the 64 anchors behind
// it of its label, the lanes take the 64 candidates (as k_chain_dp, mgx_chain.hip).  The window: anchors are loaded into a ring
// in LDS 64 at a time, one chunk ahead, and their final scores and back pointers leave it 64 at a time, one chunk behind, so a
// global access is waited for once per 64 steps.
__global__ void __launch_bounds__(64) k_chtab_chain_dp(mgx_chain_anchor *anchors, const uint64_t *list_begin, const uint32_t *query_size,
                                                    uint64_t n_lists, const int32_t *penalty, uint32_t penalty_len, uint32_t *back) {
    __shared__ int64_t r_coord[CT_RING];
    __shared__ int32_t r_clip[CT_RING], r_len[CT_RING], r_score[CT_RING];
    __shared__ uint32_t r_back[CT_RING], r_label[CT_RING];
    const uint64_t li = blockIdx.x;
    if (li >= n_lists) return;
    const uint64_t b0 = list_begin[li], n = list_begin[li + 1] - b0;
    if (!n) return;
    mgx_chain_anchor *A = anchors + b0;
    const int32_t qs = (int32_t)query_size[li];
    const uint64_t lane = threadIdx.x;
    auto load = [&](uint64_t x) {
        const mgx_chain_anchor e = A[x];
        const uint32_t s = (uint32_t)(x % CT_RING);
        r_coord[s] = e.coordinate; r_clip[s] = e.seed_clipping; r_len[s] = e.seed_end - e.seed_clipping;
        r_score[s] = e.chain_score; r_back[s] = kNid; r_label[s] = (uint32_t)e.label;
    };
    auto store = [&](uint64_t x) {
        const uint32_t s = (uint32_t)(x % CT_RING);
        A[x].chain_score = r_score[s];
        back[b0 + x] = r_back[s];
    };
    for (uint64_t x = lane; x < n && x < 65; x += 64) load(x);                   // anchors [0, 65)
    __syncthreads();
    for (uint64_t i = 0; i < n; ++i) {
        if ((i & 63) == 0) {
            if (i + 65 + lane < n) load(i + 65 + lane);                          // anchors [i + 65, i + 129): needed from step i + 1 on
            if (i) store(i - 64 + lane);                                         // anchors [i - 64, i) are final
        }
        const uint32_t si = (uint32_t)(i % CT_RING);
        const int32_t prev_clipping = r_clip[si];
        if (prev_clipping) {                                                     // (uniform)
            const int64_t prev_coord = r_coord[si];
            const int32_t prev_score = r_score[si];
            const uint32_t label = r_label[si];
            const uint64_t j = i + 1 + lane;
            const uint32_t sj = (uint32_t)(j % CT_RING);
            // (anchors of a label are one run of the sorted list, and coordinates fall along it: past the first anchor below the
            // cut-off every later one is below it too)
            if (j < n && r_label[sj] == label && !(prev_coord - (int64_t)qs > r_coord[sj])) {
                const int32_t dist = prev_clipping - r_clip[sj];
                const int32_t coord_dist = (int32_t)(prev_coord - r_coord[sj]);
                if (dist > 0 && max(dist, coord_dist) < qs) {
                    int32_t cur = prev_score + min(min(dist, coord_dist), r_len[sj]);
                    const int32_t coord_diff = abs(coord_dist - dist);
                    if (coord_diff > 0) cur -= penalty[min((uint32_t)coord_diff, penalty_len - 1)];
                    if (cur >= r_score[sj]) { r_score[sj] = cur; r_back[sj] = (uint32_t)i; }
                }
            }
        }
        __syncthreads();                                                         // (one wavefront: orders the LDS writes before the next step's reads)
    }
    const uint64_t tail = ((n - 1) / 64) * 64;
    if (tail + lane < n) store(tail + lane);
}

// ---- host side ----
std::atomic<uint64_t> g_ct_counts[4];       // launches and device-library calls, buffers taken or grown, bytes up, bytes down
enum { CTC_LAUNCH = 0, CTC_ALLOC, CTC_H2D, CTC_D2H };

int ct_ensure(DevBuf &b, size_t bytes) {
    const size_t before = b.bytes;
    if (int rc = b.ensure(std::max<size_t>(bytes, 16))) return rc;
    if (b.bytes != before) ++g_ct_counts[CTC_ALLOC];
    return MGX_OK;
}
int ct_download(mgx_aligner *A, void *dst, const void *src, size_t bytes) {
    if (!bytes) return MGX_OK;
    g_ct_counts[CTC_D2H] += bytes;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, A->hstream));
    return MGX_OK;
}
uint32_t ct_blocks(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

// exclusive sums of the n + 1 words of `which` (the last one is zero: its sum is the total)
int ct_scan_counts(mgx_aligner *A, int which, uint64_t n_lists) {
    uint64_t *in = A->ct.counts.as<uint64_t>() + (uint64_t)which * (n_lists + 1), *out = A->ct.begins.as<uint64_t>() + (uint64_t)which * (n_lists + 1);
    ++g_ct_counts[CTC_LAUNCH];
    return exclusive_sum(A, in, out, n_lists + 1);
}

void ct_view(const mgx_aligner *A, bool host, mgx_chain_tables *out) {
    const ChainTabState &c = A->ct;
    const uint64_t stride = 2 * c.n + 1;
    memset(out, 0, sizeof(*out));
    out->n_queries = c.n;
    if (host) {
        out->seed_begin = c.h_seed_begin.data(); out->seeds = c.h_seeds.data(); out->nodes = c.h_nodes.data();
        out->num_matching = c.h_num_matching.data(); out->list_begin = c.h_list_begin.data(); out->anchors = c.h_anchors.data();
        out->backtrace = c.h_backtrace.data(); out->status = c.h_status.data();
    } else {
        out->seed_begin = c.begins.as<uint64_t>() + ChainTabState::CT_SEEDS * stride; out->seeds = c.seeds.as<mgx_chain_seed>();
        out->nodes = c.nodes.as<uint64_t>(); out->num_matching = c.num_matching.as<uint64_t>();
        out->list_begin = c.begins.as<uint64_t>() + ChainTabState::CT_ANCHORS * stride; out->anchors = c.anchors_alt.as<mgx_chain_anchor>();
        out->backtrace = c.backtrace.as<uint32_t>(); out->status = c.status.as<int32_t>();
    }
}

// the device tables of the handle's last batch into its host arrays
int ct_fetch(mgx_aligner *A) {
    ChainTabState &c = A->ct;
    const uint64_t L = 2 * c.n, stride = L + 1;
    c.h_seed_begin.assign(stride, 0); c.h_list_begin.assign(stride, 0);
    c.h_num_matching.assign(std::max<uint64_t>(L, 1), 0); c.h_status.assign(std::max<uint64_t>(c.n, 1), 0);
    c.h_seeds.resize(std::max<uint64_t>(c.n_seeds, 1)); c.h_nodes.resize(std::max<uint64_t>(c.n_nodes, 1));
    c.h_anchors.resize(std::max<uint64_t>(c.n_anchors, 1)); c.h_backtrace.resize(std::max<uint64_t>(c.n_anchors, 1));
    if (!c.n) return MGX_OK;
    mgx_chain_tables d;
    ct_view(A, false, &d);
    if (int rc = ct_download(A, c.h_seed_begin.data(), d.seed_begin, stride * 8)) return rc;
    if (int rc = ct_download(A, c.h_list_begin.data(), d.list_begin, stride * 8)) return rc;
    if (int rc = ct_download(A, c.h_num_matching.data(), d.num_matching, L * 8)) return rc;
    if (int rc = ct_download(A, c.h_status.data(), d.status, c.n * 4)) return rc;
    if (int rc = ct_download(A, c.h_seeds.data(), d.seeds, c.n_seeds * sizeof(mgx_chain_seed))) return rc;
    if (int rc = ct_download(A, c.h_nodes.data(), d.nodes, c.n_nodes * 8)) return rc;
    if (int rc = ct_download(A, c.h_anchors.data(), d.anchors, c.n_anchors * sizeof(mgx_chain_anchor))) return rc;
    if (int rc = ct_download(A, c.h_backtrace.data(), d.backtrace, c.n_anchors * 4)) return rc;
    HIP_TRY(hipStreamSynchronize(A->hstream));
    return MGX_OK;
}

// the chain stage over the seeds the seeding stage left for the staged batch
int ct_run(mgx_aligner *A, const uint64_t *d_offsets, uint64_t n, uint32_t Lmax) {
    ChainTabState &c = A->ct;
    const uint64_t L = 2 * n, stride = L + 1;
    hipStream_t st = A->hstream;
    CtIn in;
    memset(&in, 0, sizeof(in));
    in.g = A->graph->g;
    in.hdr = A->seed_hdr.as<SeedHdr>(); in.seed_stream = A->seed_stream.as<DevSeed>();
    in.offsets = d_offsets; in.node_begin = A->node_begin.as<uint64_t>();
    in.nodes[0] = A->nodes_fwd.as<uint32_t>(); in.nodes[1] = A->nodes_rc.as<uint32_t>();
    int adev = 0;
    mgx_annotation_device_view(A->anno, &adev, &in.anno_rows, &in.anno_head, &in.anno_count, &in.anno_more);
    if (adev != A->graph->device) return fail(MGX_ERR_INVALID, "the annotation lives on device %d, the graph on device %d", adev, A->graph->device);
    mgx_annotation_coord_view(A->anno, &in.row_entry, &in.coord_off, &in.coords);
    in.n_lists = L; in.max_per_locus = A->cfg.max_num_seeds_per_locus; in.min_exact_match = A->cfg.min_exact_match;
    in.dummy_clean = A->anno_dummy_clean ? 1u : 0u;
    // the gap cost by coordinate difference, with the reference's float expression (aligner_chainer.cpp:404,466-481) and the
    // host's libm, as mgx_chain_seeds tabulates it: coord_diff < query size <= Lmax
    const float sl = (float)((double)(float)A->cfg.min_seed_length * 0.01);
    c.h_penalty.assign((size_t)Lmax + 1, 0);
    for (uint32_t d = 1; d <= Lmax; ++d) c.h_penalty[d] = (int32_t)std::lrintf((float)d * sl + std::log2((float)(d + 1)) * 0.5f);
    if (int rc = ct_ensure(c.penalty, c.h_penalty.size() * 4)) return rc;
    HIP_TRY(hipMemcpyAsync(c.penalty.p, c.h_penalty.data(), c.h_penalty.size() * 4, hipMemcpyHostToDevice, st));
    g_ct_counts[CTC_H2D] += c.h_penalty.size() * 4;
    if (int rc = ct_ensure(c.counts, ChainTabState::CT_ARRAYS * stride * 8)) return rc;
    if (int rc = ct_ensure(c.begins, ChainTabState::CT_ARRAYS * stride * 8)) return rc;
    if (int rc = ct_ensure(c.qsize, L * 4)) return rc;
    if (int rc = ct_ensure(c.status, n * 4)) return rc;
    if (int rc = ct_ensure(c.n_kept, L * 4)) return rc;
    if (int rc = ct_ensure(c.num_matching, L * 8)) return rc;
    HIP_TRY(hipMemsetAsync(c.counts.p, 0, ChainTabState::CT_ARRAYS * stride * 8, st));
    uint64_t *cnt = c.counts.as<uint64_t>(), *beg = c.begins.as<uint64_t>();
    uint64_t *pair_begin = beg + ChainTabState::CT_PAIRS * stride, *seed_begin = beg + ChainTabState::CT_SEEDS * stride,
             *node_begin = beg + ChainTabState::CT_NODES * stride, *list_begin = beg + ChainTabState::CT_ANCHORS * stride;
    const uint32_t wb = ct_blocks(L, CT_WAVES), wt = 64 * CT_WAVES;

    // filter_seeds: the (seed, label) pairs, sorted within every list
    k_chtab_pair_count<<<wb, wt, 0, st>>>(in, cnt + ChainTabState::CT_PAIRS * stride, c.qsize.as<uint32_t>(), c.status.as<int32_t>());
    ++g_ct_counts[CTC_LAUNCH];
    if (int rc = ct_scan_counts(A, ChainTabState::CT_PAIRS, L)) return rc;
    uint64_t n_pairs = 0;
    if (int rc = ct_download(A, &n_pairs, pair_begin + L, 8)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (n_pairs >= 0x7FFFFFF0ull)       // (the segmented sort counts items and segments in int)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_chain_tables_batch: %llu (seed, label) pairs in one call (at most 2^31 - 17): run the batch in parts",
                    (unsigned long long)n_pairs);
    if (int rc = ct_ensure(c.pair_key, n_pairs * 8)) return rc;
    if (int rc = ct_ensure(c.pair_key_alt, n_pairs * 8)) return rc;
    if (int rc = ct_ensure(c.pair_val, n_pairs * 4)) return rc;
    if (int rc = ct_ensure(c.pair_val_alt, n_pairs * 4)) return rc;
    if (int rc = ct_ensure(c.kept, n_pairs * 4)) return rc;
    k_chtab_pair_write<<<wb, wt, 0, st>>>(in, pair_begin, c.pair_key.as<uint64_t>(), c.pair_val.as<uint32_t>());
    ++g_ct_counts[CTC_LAUNCH];
    size_t tmp_pairs = 0, tmp32 = 0, tmp64 = 0;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tmp_pairs, c.pair_key.as<uint64_t>(), c.pair_key_alt.as<uint64_t>(), c.pair_val.as<uint32_t>(),
                                                        c.pair_val_alt.as<uint32_t>(), (int)n_pairs, (int)L, pair_begin, pair_begin + 1, 0, 40, st));
    if (int rc = ct_ensure(c.sort_tmp, tmp_pairs)) return rc;
    if (n_pairs) HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(c.sort_tmp.p, tmp_pairs, c.pair_key.as<uint64_t>(), c.pair_key_alt.as<uint64_t>(), c.pair_val.as<uint32_t>(),
                                                        c.pair_val_alt.as<uint32_t>(), (int)n_pairs, (int)L, pair_begin, pair_begin + 1, 0, 40, st));
    ++g_ct_counts[CTC_LAUNCH];
    k_chtab_labels<<<wb, wt, 0, st>>>(in, pair_begin, c.pair_key_alt.as<uint64_t>(), c.pair_val_alt.as<uint32_t>(), c.kept.as<uint32_t>(), c.n_kept.as<uint32_t>());
    ++g_ct_counts[CTC_LAUNCH];
    // ... the seeds it keeps: sizes, then the seeds, their nodes and their anchors
    k_chtab_seed_count<<<wb, wt, 0, st>>>(in, pair_begin, c.kept.as<uint32_t>(), c.n_kept.as<uint32_t>(), cnt + ChainTabState::CT_SEEDS * stride,
                                       cnt + ChainTabState::CT_NODES * stride, cnt + ChainTabState::CT_ANCHORS * stride, c.num_matching.as<uint64_t>());
    ++g_ct_counts[CTC_LAUNCH];
    for (int which : { ChainTabState::CT_SEEDS, ChainTabState::CT_NODES, ChainTabState::CT_ANCHORS })
        if (int rc = ct_scan_counts(A, which, L)) return rc;
    uint64_t totals[3] = { 0, 0, 0 };
    if (int rc = ct_download(A, &totals[0], seed_begin + L, 8)) return rc;
    if (int rc = ct_download(A, &totals[1], node_begin + L, 8)) return rc;
    if (int rc = ct_download(A, &totals[2], list_begin + L, 8)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    c.n_seeds = totals[0]; c.n_nodes = totals[1]; c.n_anchors = totals[2];
    const uint64_t T = c.n_anchors;
    if (T >= 0x7FFFFFF0ull)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_chain_tables_batch: %llu anchors in one call (at most 2^31 - 17): run the batch in parts", (unsigned long long)T);
    if (int rc = ct_ensure(c.seeds, c.n_seeds * sizeof(mgx_chain_seed))) return rc;
    if (int rc = ct_ensure(c.nodes, c.n_nodes * 8)) return rc;
    if (int rc = ct_ensure(c.anchors, T * sizeof(mgx_chain_anchor))) return rc;
    if (int rc = ct_ensure(c.anchors_alt, T * sizeof(mgx_chain_anchor))) return rc;
    if (int rc = ct_ensure(c.backtrace, T * 4)) return rc;
    if (int rc = ct_ensure(c.perm, T * 4)) return rc;
    if (int rc = ct_ensure(c.perm_alt, T * 4)) return rc;
    if (int rc = ct_ensure(c.k32, T * 4)) return rc;
    if (int rc = ct_ensure(c.k32_alt, T * 4)) return rc;
    if (int rc = ct_ensure(c.k64, T * 8)) return rc;
    if (int rc = ct_ensure(c.k64_alt, T * 8)) return rc;
    k_chtab_emit<<<wb, wt, 0, st>>>(in, pair_begin, c.kept.as<uint32_t>(), c.n_kept.as<uint32_t>(), seed_begin, node_begin, list_begin,
                                 c.seeds.as<mgx_chain_seed>(), c.nodes.as<uint64_t>(), c.anchors.as<mgx_chain_anchor>());
    ++g_ct_counts[CTC_LAUNCH];
    // chain_seeds: the sort ...
    uint32_t *perm = c.perm.as<uint32_t>(), *perm2 = c.perm_alt.as<uint32_t>();
    const mgx_chain_anchor *raw = c.anchors.as<mgx_chain_anchor>();
    mgx_chain_anchor *sorted = c.anchors_alt.as<mgx_chain_anchor>();
    const uint32_t tb = 256, eb = std::max(1u, ct_blocks(T, tb));
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(nullptr, tmp32, c.k32.as<uint32_t>(), c.k32_alt.as<uint32_t>(), perm, perm2, (int)T, (int)L,
                                                                  list_begin, list_begin + 1, 0, 32, st));
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(nullptr, tmp64, c.k64.as<uint64_t>(), c.k64_alt.as<uint64_t>(), perm, perm2, (int)T, (int)L,
                                                                  list_begin, list_begin + 1, 0, 64, st));
    const size_t tmp_bytes = std::max(tmp32, tmp64);
    if (int rc = ct_ensure(c.sort_tmp_anchors, tmp_bytes)) return rc;
    if (!T) return MGX_OK;            // (no anchor in the batch: the tables are empty)
    g_ct_counts[CTC_LAUNCH] += 9;     // iota, three key gathers, three sorts, the permutation, the DP
    k_chtab_iota<<<eb, tb, 0, st>>>(perm, T);
    k_chtab_key_query<<<eb, tb, 0, st>>>(raw, perm, T, c.k32.as<uint32_t>());
    size_t tmp = tmp_bytes;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(c.sort_tmp_anchors.p, tmp, c.k32.as<uint32_t>(), c.k32_alt.as<uint32_t>(), perm, perm2, (int)T, (int)L,
                                                                  list_begin, list_begin + 1, 0, 32, st));
    std::swap(perm, perm2);
    k_chtab_key_coord<<<eb, tb, 0, st>>>(raw, perm, T, c.k64.as<uint64_t>());
    tmp = tmp_bytes;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(c.sort_tmp_anchors.p, tmp, c.k64.as<uint64_t>(), c.k64_alt.as<uint64_t>(), perm, perm2, (int)T, (int)L,
                                                                  list_begin, list_begin + 1, 0, 64, st));
    std::swap(perm, perm2);
    k_chtab_key_label<<<eb, tb, 0, st>>>(raw, perm, T, c.k32.as<uint32_t>());
    tmp = tmp_bytes;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(c.sort_tmp_anchors.p, tmp, c.k32.as<uint32_t>(), c.k32_alt.as<uint32_t>(), perm, perm2, (int)T, (int)L,
                                                                  list_begin, list_begin + 1, 0, 24, st));
    std::swap(perm, perm2);
    k_chtab_permute<<<eb, tb, 0, st>>>(raw, perm, T, sorted);
    // ... and the DP
    k_chtab_chain_dp<<<(uint32_t)L, 64, 0, st>>>(sorted, list_begin, c.qsize.as<uint32_t>(), L, c.penalty.as<int32_t>(), (uint32_t)c.h_penalty.size(),
                                              c.backtrace.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return MGX_OK;
}

} // namespace

extern "C" {

int mgx_chain_tables_batch(mgx_aligner *A, const char *seqs, const uint64_t *offsets, uint64_t n, int seqs_on_device, uint32_t flags,
                           mgx_chain_tables *out) {
    if (!A || !out || (n && (!seqs || !offsets))) return fail(MGX_ERR_INVALID, "mgx_chain_tables_batch: null argument");
    if (!A->chainer) return fail(MGX_ERR_INVALID, "mgx_chain_tables_batch: not a seed-chainer handle (mgx_seed_chainer_create)");
    if (flags & ~MGX_CHAIN_TABLES_ON_DEVICE) return fail(MGX_ERR_INVALID, "mgx_chain_tables_batch: unknown flags 0x%x", flags);
    if (n >= 0x3FFFFFF0ull) return fail(MGX_ERR_UNSUPPORTED, "mgx_chain_tables_batch: %llu queries in one call (at most 2^30 - 17)", (unsigned long long)n);
    if (mgx_device_count() <= A->graph->device) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(A->graph->device));
    ChainTabState &c = A->ct;
    c.have = false;
    c.n = n; c.n_seeds = c.n_nodes = c.n_anchors = 0;
    if (n == 0) {
        A->n_reads = 0;
        if (int rc = ct_fetch(A)) return rc;
        c.have = true;
        ct_view(A, true, out);        // (no query: nothing to point to on the device)
        return MGX_OK;
    }
    const char *d_seqs; const uint64_t *d_offsets; uint32_t Lmax;
    if (int rc = stage_batch(A, seqs, offsets, n, seqs_on_device, &d_seqs, &d_offsets, &Lmax)) return rc;
    const bool mapped = A->cfg.max_seed_length >= A->graph->g.k;
    if (int rc = run_map(A, d_seqs, d_offsets, n, true, mapped, Lmax)) return rc;
    for (;;) {
        // the seed stream keeps counting past its capacity: the stage is redone with what it asked for (as mgx_align_batch_device does)
        uint64_t seeds_wanted = 0;
        if (int rc = run_seeding(A, d_seqs, d_offsets, n, Lmax, &seeds_wanted)) return rc;
        if (seeds_wanted <= A->seed_cap) break;
        A->seed_scale = seeds_wanted / std::max<uint64_t>(1, A->seed_cap / A->seed_scale) + 2;
    }
    if (int rc = collect_stats(A, mapped, true)) return rc;
    if (int rc = ct_run(A, d_offsets, n, Lmax)) return rc;
    if (flags & MGX_CHAIN_TABLES_ON_DEVICE) {
        HIP_TRY(hipStreamSynchronize(A->hstream));
    } else if (int rc = ct_fetch(A)) {
        return rc;
    }
    c.have = true;
    ct_view(A, !(flags & MGX_CHAIN_TABLES_ON_DEVICE), out);
    return MGX_OK;
}

int mgx_chain_tables_fetch(mgx_aligner *A, mgx_chain_tables *out_host) {
    if (!A || !out_host) return fail(MGX_ERR_INVALID, "mgx_chain_tables_fetch: null argument");
    if (!A->chainer || !A->ct.have) return fail(MGX_ERR_INVALID, "mgx_chain_tables_fetch: no chain tables on this handle (mgx_chain_tables_batch has not run)");
    HIP_TRY(hipSetDevice(A->graph->device));
    if (int rc = ct_fetch(A)) return rc;
    ct_view(A, true, out_host);
    return MGX_OK;
}

void mgx_chain_tables_kernel_launch_counts(uint64_t *out4) { for (int x = 0; x < 4; ++x) out4[x] = g_ct_counts[x].load(); }

} // extern "C"
