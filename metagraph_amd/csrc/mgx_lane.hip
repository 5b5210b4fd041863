// mgx_lane.hip — the lane-per-read kernel (lane_read.hpp): every lane of a wavefront aligns its own read, 64 reads per
// instruction, in front of the 8-lane group kernel of mgx_grp.hip.  A lane finishes a "simple" read completely (result record
// + output stream) or lists it for the group kernel, which then aligns it from scratch; see lane_read.hpp for the contract.
//
// Shape: persistent wavefronts; a wavefront takes 64 consecutive items of the work-sorted order at a time (neighbours need about
// the same number of columns), runs lane_read() on them — the column loop is where the lanes spend their time; a lane whose read
// ends or bails early idles until its 63 wave-mates are through — hands out the output-stream words of the whole wavefront with
// ONE atomic, and writes results.  Per-lane state: the DP window (32 S + 32 F cells) and the bookkeeping of one extension in
// VGPRs; the packed query and the cold per-read state in LDS (word-major, conflict free); column slots, S rows and the CIGAR
// runs of the trace in the wavefront's HBM scratch, interleaved over its lanes (the lanes commit their columns in lock-step:
// full-line stores); the node table in a private slice per lane.
#include <hip/hip_runtime.h>

#define mgx mgx_lane_ns
#include "wave.hpp"
#include "graph_build.hpp"
#include "lane_read.hpp"
#include "kernel_units.hpp"

using namespace mgx;

#ifndef MGX_LANE_WAVES_PER_SIMD
#define MGX_LANE_WAVES_PER_SIMD 2
#endif

__global__ void __launch_bounds__(64, MGX_LANE_WAVES_PER_SIMD) k_lane(const LaneParams *__restrict__ LPp) {
    // (the parameter block stays in memory: its ~90 uniform words are re-read with scalar loads where they are used instead of
    // occupying — and spilling — scalar registers across the column loop)
    const LaneParams &LP = *LPp;
    __shared__ uint64_t s_qw[LANE_QWORDS][64];
    __shared__ uint32_t s_cold[LANE_COLD_WORDS][64];
    const int lane = (int)threadIdx.x;
    // the wavefront's scratch from this lane's word on (layout: LaneParams — column slots and S rows interleaved over the lanes)
    uint8_t *scratch = LP.scratch + (uint64_t)blockIdx.x * LP.wave_stride + 4u * (uint32_t)lane;
    LaneChip chip;
    chip.lane = lane;
    chip.qw = &s_qw[0][lane]; chip.qstride = 64;
    chip.cold = &s_cold[0][lane]; chip.cstride = 64;
    const uint64_t n_items = LP.P.n_items ? LP.P.n_items : LP.P.n_reads;
    LaneCounters ctr;
    memset(&ctr, 0, sizeof(ctr));
#if MGX_LANE_TIMERS
    const uint64_t t_kernel = cycle_clock();
    uint64_t t_emit = 0;
#endif
    {
        uint32_t *rec = lane_record(LP, scratch, lane);
        for (int x = 26; x < 32; ++x) gst(rec + x, 0u);
    }
    // Every lane holds one read at a time: a new one from the sorted order, or — after LR_AGAIN — the same one for its backward
    // pass, while its wave-mates move on to new reads.
    uint64_t read = 0, item = 0;
    int pass = 0;
    bool holding = false;
    for (;;) {
        LV<bool> wantv;
        wantv.v = !holding;
        const uint64_t wm = wave_ballot(wantv);
        LV<uint64_t> bv;
        bv.v = 0;
        if (lane == 0 && wm) bv.v = atomicAdd(LP.P.read_cursor, (unsigned long long)popc64(wm));
        const uint64_t base = wave_bcast(bv, 0);
        if (!holding) {
            item = base + (uint64_t)popc64(wm & ((1ull << lane) - 1));
            pass = 0;
            if (item < n_items) { holding = true; read = LP.P.order ? (uint64_t)gld(LP.P.order + item) : item; }
        }
        LV<bool> actv;
        actv.v = holding;
        if (!wave_ballot(actv)) break;                       // nobody holds a read and the order is exhausted
        const bool active = holding;
        int rc = LR_DONE;
        LaneResult R;
        R.words = 0; R.have_aln = 0;
        if (active) rc = lane_read_dp(LP, read, (uint32_t)item, pass, scratch, chip, ctr, R);       // (the exact exit: k_lane_exact, below)
        if (active && rc == LR_AGAIN) pass = 1; else holding = false;
        const bool done = active && rc == LR_DONE, bail = active && rc == LR_BAIL;
        // output-stream words of the wavefront's finished reads: one atomic, a prefix sum over the lanes
        LV<int32_t> wv;
        wv.v = done ? (int32_t)R.words : 0;
        const LV<int32_t> pre = wave_prefix_sum_excl(wv);
        const int32_t total = wave_sum(wv);
        LV<uint64_t> sv;
        sv.v = 0;
        if (lane == 0 && total) sv.v = atomicAdd(LP.P.out_cursor, (unsigned long long)total);
        const uint64_t so = wave_bcast(sv, 0) + (uint64_t)pre.v;
#if MGX_LANE_TIMERS
        const uint64_t te0 = cycle_clock();
#endif
        if (done) {
            lane_emit_t<false>(LP, read, scratch, chip, R, so);
            uint32_t *rec = lane_record(LP, scratch, lane);
            gst(rec + 29, gld(rec + 29) + 1u); gst(rec + 30, gld(rec + 30) + R.rr.n_extensions);
            gst(rec + 31, gld(rec + 31) + (uint32_t)(R.rr.status != ST_OK));
        }
#if MGX_LANE_TIMERS
        t_emit += cycle_clock() - te0;
#endif
        // the reads for the group kernel, in processing order
        LV<bool> bl;
        bl.v = bail;
        const uint64_t bm = wave_ballot(bl);
        if (bm) {
            LV<uint64_t> pv;
            pv.v = 0;
            if (lane == 0) pv.v = atomicAdd(LP.bail_count, (unsigned long long)popc64(bm));
            const uint64_t p0 = wave_bcast(pv, 0);
            if (bail) gst(LP.bail_list + p0 + (uint64_t)popc64(bm & ((1ull << lane) - 1)), (uint32_t)read);
            // ... and why, for the statistics: one atomic per distinct reason of the wavefront
            uint64_t left = bm;
            while (left) {
                LV<uint32_t> rv;
                rv.v = ctr.reason;
                const uint32_t code = wave_bcast(rv, ctz64(left)) & 31u;
                LV<bool> same;
                same.v = bail && (ctr.reason & 31u) == code;
                const uint64_t sm = wave_ballot(same);
                if (lane == 0) atomicAdd(LP.bail_hist + code, (unsigned long long)popc64(sm));
                left &= ~sm;
            }
        }
    }
    // counters: one atomic per wavefront and counter
    const uint32_t *rec = lane_record(LP, scratch, lane);
    LV<int32_t> v;
    v.v = (int32_t)gld(rec + 27); const int32_t rl = wave_sum(v);
    v.v = (int32_t)gld(rec + 28); const int32_t sl = wave_sum(v);
    v.v = (int32_t)gld(rec + 26); const int32_t cl = wave_sum(v);
    v.v = (int32_t)gld(rec + 29); const int32_t nd = wave_sum(v);
    v.v = (int32_t)gld(rec + 30); const int32_t ne = wave_sum(v);
    v.v = (int32_t)gld(rec + 31); const int32_t nc = wave_sum(v);
#if MGX_LANE_TIMERS
    // (bail_hist[32 .. 39]: the sections of lane_read(), [40] lane_emit, [41] the kernel: cycles of lane 0 of every wavefront)
    if (lane == 0) {
        for (int x = 0; x < 8; ++x) atomicAdd(LP.bail_hist + 32 + x, (unsigned long long)ctr.t[x]);
        atomicAdd(LP.bail_hist + 40, (unsigned long long)t_emit);
        atomicAdd(LP.bail_hist + 41, (unsigned long long)(cycle_clock() - t_kernel));
    }
#endif
    if (lane == 0) {
        atomicAdd(&LP.P.stats->rank_lines, (unsigned long long)rl);
        atomicAdd(&LP.P.stats->select_lines, (unsigned long long)sl);
        atomicAdd(&LP.P.stats->columns, (unsigned long long)cl);
        atomicAdd(&LP.P.stats->fast_columns, (unsigned long long)cl);
        atomicAdd(&LP.P.stats->lane_lines, (unsigned long long)rl + (unsigned long long)sl);
        atomicAdd(&LP.P.stats->lane_columns, (unsigned long long)cl);
        atomicAdd(&LP.P.stats->extensions, (unsigned long long)ne);
        atomicAdd(&LP.P.stats->capacity_errors, (unsigned long long)nc);
        atomicAdd(LP.done_count, (unsigned long long)nd);
    }
}

// The exact exit (lane_read.hpp, lane_exact()) for launches with LaneParams::exact, BEFORE the work sort: every read whose first
// seed spans the query (and, at level 2, every read of the path class: first seed at the query's first character, every k-mer a node;
// counted apart in bail_hist[LANE_HIST_EXACT_PATH]) gets its result record and output stream here, in closed form, and the work key LaneParams::done_key, which
// sorts it behind every read that still has to be aligned; the host then launches k_lane on the items in front of them.  A kernel
// of its own because k_lane has no register to spare — the same test inside its loop, in front of the DP, made the allocator
// spill 33 VGPRs in the column loop, a mark tested where k_lane fetches its items cost 25 more spilled SGPRs there — and because
// this way k_lane is the code it was: it never meets these reads.  One lane per read, in read order.
// Label-aware batches have a kernel of their own, k_lane_exact_labeled (and k_lane_exact_sub_labeled behind it at level 3): the same loop around lane_exact_t<true>, whose filter over
// the seeds' rows and scan over the path's rows (up to ~120 independent 8-byte gathers a read, four in flight at a time) take 30
// registers more; k_lane_exact, compiled without them, keeps its code and its occupancy for the unlabeled batches.
template <bool LABELED>
__device__ __forceinline__ void lane_exact_body(const LaneParams &LP) {
    const int lane = (int)threadIdx.x;
    const uint64_t n_reads = LP.P.n_reads;
    LaneChip chip;
    chip.lane = lane; chip.qw = nullptr; chip.qstride = 0; chip.cold = nullptr; chip.cstride = 0;     // (the closed form needs neither)
    uint32_t n_done = 0, n_path = 0, n_cap = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_reads; base += (uint64_t)gridDim.x * 64) {
        const uint64_t read = base + (uint64_t)lane;
        LaneResult R;
        R.words = 0;
        LV<bool> hv;
        int32_t run_lo = 0, run_hi = 0;
        const int cls = read < n_reads ? lane_exact_t<LABELED>(LP, read, R, run_lo, run_hi) : LANE_EXACT_NONE;
        if constexpr (!LABELED) {
            // level 3: the candidates of the substitution class go on a list for k_lane_exact_sub — one atomic per wavefront — which
            // walks them side by side; nothing of theirs is written here
            LV<bool> cv;
            cv.v = cls == LANE_EXACT_SUB;
            const uint64_t cm = wave_ballot(cv);
            if (cm) {
                LV<uint64_t> pv;
                pv.v = 0;
                if (lane == 0) pv.v = atomicAdd(LP.bail_hist + LANE_HIST_SUB_CAND, (unsigned long long)popc64(cm));
                const uint64_t p0 = wave_bcast(pv, 0) + (uint64_t)popc64(cm & ((1ull << lane) - 1));
                if (cv.v) {
                    LaneSubCand c;
                    c.read = (uint32_t)read; c.strand = (uint32_t)R.strand; c.lo = (uint32_t)run_lo; c.hi = (uint32_t)run_hi;
                    gst(LP.sub_list + p0, c);
                }
            }
        } else {
            // ... label-aware: for k_lane_exact_sub_labeled, with what the seed filter found (it is not run again there)
            LV<bool> cv;
            cv.v = cls == LANE_EXACT_SUB;
            const uint64_t cm = wave_ballot(cv);
            if (cm) {
                LV<uint64_t> pv;
                pv.v = 0;
                if (lane == 0) pv.v = atomicAdd(LP.bail_hist + LANE_HIST_SUB_CAND, (unsigned long long)popc64(cm));
                const uint64_t p0 = wave_bcast(pv, 0) + (uint64_t)popc64(cm & ((1ull << lane) - 1));
                if (cv.v) {
                    LaneSubCandLabeled c;
                    c.read = (uint32_t)read; c.strand = (uint32_t)R.strand; c.lo = (uint32_t)run_lo; c.hi = (uint32_t)run_hi;
                    c.label = R.label;
                    c.nm[0] = R.rr.num_matches_fwd; c.nm[1] = R.rr.num_matches_rc; c.ns[0] = R.rr.n_seeds_fwd; c.ns[1] = R.rr.n_seeds_rc;
                    c.pad[0] = c.pad[1] = c.pad[2] = 0u;
                    gst((LaneSubCandLabeled *)LP.sub_list + p0, c);
                }
            }
        }
        hv.v = cls == LANE_EXACT_SPAN || cls == LANE_EXACT_PATH;
        if (!wave_ballot(hv)) continue;
        // output-stream words of the wavefront's reads: one atomic, a prefix sum over the lanes (as k_lane)
        LV<int32_t> wv;
        wv.v = hv.v ? (int32_t)R.words : 0;
        const LV<int32_t> pre = wave_prefix_sum_excl(wv);
        const int32_t total = wave_sum(wv);
        LV<uint64_t> sv;
        sv.v = 0;
        if (lane == 0) sv.v = atomicAdd(LP.P.out_cursor, (unsigned long long)total);
        const uint64_t so = wave_bcast(sv, 0) + (uint64_t)pre.v;
        if (hv.v) {
            lane_emit_t<true>(LP, read, nullptr, chip, R, so);
            gst(LP.P.work_key + read, LP.done_key);
            ++n_done; n_path += (uint32_t)(cls == LANE_EXACT_PATH); n_cap += (uint32_t)(R.rr.status != ST_OK);
        }
    }
    LV<int32_t> v;
    v.v = (int32_t)n_done; const int32_t nd = wave_sum(v);
    v.v = (int32_t)n_cap; const int32_t nc = wave_sum(v);
    v.v = (int32_t)n_path; const int32_t np = wave_sum(v);
    if (lane == 0 && nd) {
        atomicAdd(LP.done_count, (unsigned long long)nd);
        atomicAdd(LP.bail_hist + LANE_HIST_EXACT, (unsigned long long)nd);
        if (np) atomicAdd(LP.bail_hist + LANE_HIST_EXACT_PATH, (unsigned long long)np);
        if (nc) atomicAdd(&LP.P.stats->capacity_errors, (unsigned long long)nc);
    }
}

__global__ void __launch_bounds__(64) k_lane_exact(const LaneParams *__restrict__ LPp) { lane_exact_body<false>(*LPp); }

// The substitution class (lane_read.hpp lane_exact_sub(); LaneParams::exact >= 3), behind k_lane_exact and before the work sort:
// one lane per candidate of LaneParams::sub_list, grid-stride, the count read from device memory (bail_hist[LANE_HIST_SUB_CAND]: no
// host read-back between the two kernels).  The lanes that walk sit side by side: in k_lane_exact a walking lane would have its
// 63 wave-mates wait out up to k + 1 dependent graph steps.  The walked nodes stay in LDS until every test has passed; only then
// is the stream cursor advanced (one atomic per wavefront) and the read written, with the work key that takes it out of k_lane's
// launch.  A candidate that fails is left as it was: k_lane aligns it.
__global__ void __launch_bounds__(64) k_lane_exact_sub(const LaneParams *__restrict__ LPp) {
    const LaneParams &LP = *LPp;
    __shared__ uint32_t s_walk[LANE_SUB_MAX_WALK][64];
    const int lane = (int)threadIdx.x;
    const uint64_t n_cand = (uint64_t)gld(LP.bail_hist + LANE_HIST_SUB_CAND);
    LaneChip chip;
    chip.lane = lane; chip.qw = nullptr; chip.qstride = 0; chip.cold = &s_walk[0][lane]; chip.cstride = 64;
    LineCtr lc = { 0, 0, 0 };
    uint32_t n_done = 0, n_cap = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_cand; base += (uint64_t)gridDim.x * 64) {
        const uint64_t at = base + (uint64_t)lane;
        LaneResult R;
        R.words = 0;
        LV<bool> hv;
        hv.v = false;
        uint64_t read = 0;
        if (at < n_cand) {
            const LaneSubCand c = gld(LP.sub_list + at);
            read = c.read;
            hv.v = lane_exact_sub(LP, read, (int)c.strand, (int32_t)c.lo, (int32_t)c.hi, chip.cold, chip.cstride, R, lc);
        }
        if (!wave_ballot(hv)) continue;
        LV<int32_t> wv;
        wv.v = hv.v ? (int32_t)R.words : 0;
        const LV<int32_t> pre = wave_prefix_sum_excl(wv);
        const int32_t total = wave_sum(wv);
        LV<uint64_t> sv;
        sv.v = 0;
        if (lane == 0) sv.v = atomicAdd(LP.P.out_cursor, (unsigned long long)total);
        const uint64_t so = wave_bcast(sv, 0) + (uint64_t)pre.v;
        if (hv.v) {
            lane_emit_t<true, true>(LP, read, nullptr, chip, R, so);
            gst(LP.P.work_key + read, LP.done_key);
            ++n_done; n_cap += (uint32_t)(R.rr.status != ST_OK);
        }
    }
    LV<int32_t> v;
    v.v = (int32_t)n_done; const int32_t nd = wave_sum(v);
    v.v = (int32_t)n_cap; const int32_t nc = wave_sum(v);
    v.v = (int32_t)(lc.rank_lines + lc.bit_lines); const int32_t rl = wave_sum(v);
    v.v = (int32_t)lc.select_lines; const int32_t sl = wave_sum(v);
    if (lane == 0) {
        if (nd) {
            atomicAdd(LP.done_count, (unsigned long long)nd);
            atomicAdd(LP.bail_hist + LANE_HIST_EXACT, (unsigned long long)nd);
            atomicAdd(LP.bail_hist + LANE_HIST_EXACT_SUB, (unsigned long long)nd);
        }
        if (nc) atomicAdd(&LP.P.stats->capacity_errors, (unsigned long long)nc);
        if (rl | sl) {
            atomicAdd(&LP.P.stats->rank_lines, (unsigned long long)rl);
            atomicAdd(&LP.P.stats->select_lines, (unsigned long long)sl);
            atomicAdd(&LP.P.stats->lane_lines, (unsigned long long)rl + (unsigned long long)sl);
        }
    }
}
__global__ void __launch_bounds__(64) k_lane_exact_labeled(const LaneParams *__restrict__ LPp) { lane_exact_body<true>(*LPp); }

// The substitution class of a label-aware batch, behind k_lane_exact_labeled: k_lane_exact_sub's loop over LaneSubCandLabeled
// records.  k_lane_exact_labeled has tested the rows of the mapped nodes on both sides of the run (in the pass its path-class reads
// make anyway), so only candidates whose mapped nodes all carry { L } walk; lane_exact_sub<true>() walks, tests the walked nodes'
// rows — up to k gathers, four in flight — and the rest.  Nothing is written before every test has passed.
__global__ void __launch_bounds__(64) k_lane_exact_sub_labeled(const LaneParams *__restrict__ LPp) {
    const LaneParams &LP = *LPp;
    __shared__ uint32_t s_walk[LANE_SUB_MAX_WALK][64];
    const int lane = (int)threadIdx.x;
    const uint64_t n_cand = (uint64_t)gld(LP.bail_hist + LANE_HIST_SUB_CAND);
    const LaneSubCandLabeled *list = (const LaneSubCandLabeled *)LP.sub_list;
    LaneChip chip;
    chip.lane = lane; chip.qw = nullptr; chip.qstride = 0; chip.cold = &s_walk[0][lane]; chip.cstride = 64;
    LineCtr lc = { 0, 0, 0 };
    uint32_t n_done = 0, n_cap = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_cand; base += (uint64_t)gridDim.x * 64) {
        const uint64_t at = base + (uint64_t)lane;
        LaneResult R;
        R.words = 0;
        LV<bool> hv;
        hv.v = false;
        uint64_t read = 0;
        if (at < n_cand) {
            const LaneSubCandLabeled c = gld(list + at);
            read = c.read;
            R.label = c.label;
            R.rr.num_matches_fwd = c.nm[0]; R.rr.num_matches_rc = c.nm[1]; R.rr.n_seeds_fwd = c.ns[0]; R.rr.n_seeds_rc = c.ns[1];
            hv.v = lane_exact_sub<true>(LP, read, (int)c.strand, (int32_t)c.lo, (int32_t)c.hi, chip.cold, chip.cstride, R, lc);
        }
        if (!wave_ballot(hv)) continue;
        LV<int32_t> wv;
        wv.v = hv.v ? (int32_t)R.words : 0;
        const LV<int32_t> pre = wave_prefix_sum_excl(wv);
        const int32_t total = wave_sum(wv);
        LV<uint64_t> sv;
        sv.v = 0;
        if (lane == 0) sv.v = atomicAdd(LP.P.out_cursor, (unsigned long long)total);
        const uint64_t so = wave_bcast(sv, 0) + (uint64_t)pre.v;
        if (hv.v) {
            lane_emit_t<true, true, true>(LP, read, nullptr, chip, R, so);
            gst(LP.P.work_key + read, LP.done_key);
            ++n_done; n_cap += (uint32_t)(R.rr.status != ST_OK);
        }
    }
    LV<int32_t> v;
    v.v = (int32_t)n_done; const int32_t nd = wave_sum(v);
    v.v = (int32_t)n_cap; const int32_t nc = wave_sum(v);
    v.v = (int32_t)(lc.rank_lines + lc.bit_lines); const int32_t rl = wave_sum(v);
    v.v = (int32_t)lc.select_lines; const int32_t sl = wave_sum(v);
    if (lane == 0) {
        if (nd) {
            atomicAdd(LP.done_count, (unsigned long long)nd);
            atomicAdd(LP.bail_hist + LANE_HIST_EXACT, (unsigned long long)nd);
            atomicAdd(LP.bail_hist + LANE_HIST_EXACT_SUB, (unsigned long long)nd);
        }
        if (nc) atomicAdd(&LP.P.stats->capacity_errors, (unsigned long long)nc);
        if (rl | sl) {
            atomicAdd(&LP.P.stats->rank_lines, (unsigned long long)rl);
            atomicAdd(&LP.P.stats->select_lines, (unsigned long long)sl);
            atomicAdd(&LP.P.stats->lane_lines, (unsigned long long)rl + (unsigned long long)sl);
        }
    }
}

// blocks = resident wavefronts (wavefront b owns LaneParams::scratch + b * wave_stride)
// d_params: the LaneParams of this launch in device memory
extern "C" int mgx_launch_lane(const void *d_params, uint32_t blocks, void *stream) {
    static_assert(sizeof(LaneParams) == MGX_LANE_PARAMS_BYTES, "LaneParams differs from what mgx.hip passes");
    k_lane<<<blocks, 64, 0, (hipStream_t)stream>>>(static_cast<const LaneParams *>(d_params));
    return (int)hipGetLastError();
}
// the exact exit, between seeding and the work sort (LaneParams::exact; done_count and bail_hist start at zero and are k_lane's too)
// labeled: the batch is label-aware (AlignParams::labeled != 0)
extern "C" int mgx_launch_lane_exact(const void *d_params, uint32_t blocks, int labeled, void *stream) {
    if (labeled) k_lane_exact_labeled<<<blocks, 64, 0, (hipStream_t)stream>>>(static_cast<const LaneParams *>(d_params));
    else k_lane_exact<<<blocks, 64, 0, (hipStream_t)stream>>>(static_cast<const LaneParams *>(d_params));
    return (int)hipGetLastError();
}
// the substitution class, behind mgx_launch_lane_exact on the same stream (LaneParams::exact >= 3)
// labeled: as mgx_launch_lane_exact
extern "C" int mgx_launch_lane_exact_sub(const void *d_params, uint32_t blocks, int labeled, void *stream) {
    if (labeled) k_lane_exact_sub_labeled<<<blocks, 64, 0, (hipStream_t)stream>>>(static_cast<const LaneParams *>(d_params));
    else k_lane_exact_sub<<<blocks, 64, 0, (hipStream_t)stream>>>(static_cast<const LaneParams *>(d_params));
    return (int)hipGetLastError();
}
extern "C" int mgx_lane_waves_per_simd(void) { return MGX_LANE_WAVES_PER_SIMD; }
