"""The substitution class of the lane extender's exact exit on label-aware batches on the GPU (level 3: k_lane_exact_labeled lists
the candidates with the seed filter's label and counts, k_lane_exact_sub_labeled walks them, tests the walked nodes' rows and
finishes the class reads — mgx_lane.hip, exact_by_lanes in mgx.hip).  Small batches with lane=1, multi_pass=0 and exact=3 on the
directed world of tests/lane_exact_sub_label_worlds.py — class reads, reads of both other classes, every refusal kind (a walked or
mapped node with another label, two labels, none; across the label boundary; the other strand's seeds with another label; a strand
the filter emptied; an insertion, a SNP site, two substitutions, a recombinant; a later seed off the path), reads without seeds
and reads the lane hands over share wavefronts, at 1, 63, 64, 65 and 129 reads — against the oracle's LabeledAligner (alignments
and label lists), against exact=0 and exact=2 on the same handle, the three counters against the predicate's counts.  Candidate
lists of 0, 1, 64 and 65 entries; a batch of class reads only, for which k_lane is not launched; a label on a dummy node's row; one
batch just above the automatic threshold.
Every assertion of n_lane_exact_sub_reads > 0 fails where exact=3 means 2 for label-aware batches.
(tests/test_lane_exact_sub_labels.py runs the same per-read functions in the host model.)"""
import numpy as np
import pytest

import lane_exact_sub_label_worlds as SLW
import orc
from labeled_worlds import with_labels
from metagraph_amd import aligner, capi
from test_gpu_lane_exact_labels import labeled_handle, lane_launches, run_arrays, same_arrays, segment_batch
from test_gpu_parity import gpu_graph

pytestmark = pytest.mark.gpu

K = 21
# whether the automatic default of the exit (no option exact) runs label-aware batches at level 3: lane_types.hpp
# LANE_EXACT_AUTO_SUB_LABELED, the decision the README's result paragraph records
AUTO_LEVEL_3_FOR_LABEL_AWARE_BATCHES = True


def counters(st):
    return st["n_lane_exact_reads"], st["n_lane_exact_path_reads"], st["n_lane_exact_sub_reads"]


def run_twice(A, reads, want, counts):
    for _ in range(2):                                        # (and again through the same handle: cursors and counters start afresh)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        st = A.stats()
        for q in range(len(reads)):
            assert got[q] == want[q], (q, reads[q], got[q], want[q])
        assert counters(st) == counts, (st, counts)
        assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    return got, st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_label_aware_batches_at_level_3(n):
    g, anno, named = SLW.mixed_batch(n)
    names, reads = [x[0] for x in named], [x[1] for x in named]
    cfg = capi.config_cli(K)
    cls, want = SLW.check_closed_form(g, anno, cfg, reads)
    every = set(cls.span) | set(cls.path) | set(cls.sub)
    if n == 1:
        assert len(cls.sub) == 1
    else:
        assert cls.span and cls.path and cls.sub and len(every) < n
        assert {s for s, _, _, _ in cls.sub.values()} == {0, 1}
        assert cls.refused_row and cls.refused_walk
        for kind in ("walk_row_other", "walk_row_two", "walk_row_none", "edge_lo", "edge_hi", "edge_lo_minus_1", "edge_hi_plus_1",
                     "boundary", "other_strand_label", "short_under", "insertion", "snp_site", "two_", "random", "with_n"):
            assert any(nm.startswith(kind) and q not in every for q, nm in enumerate(names)), kind
        assert any(not want[q] for q in range(n))
    if n == 129:
        assert cls.refused_seed
    A = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=3")
    got, st = run_twice(A, reads, want, (len(cls.span), len(cls.path), len(cls.sub)))
    assert st["extend_kernels"] & capi.KERNEL_LANE
    A.set_pipeline("exact=0")
    got0, st0 = run_twice(A, reads, want, (0, 0, 0))
    assert got0 == got
    # the reads outside the classes leave for the reasons they leave for with the exit off
    assert all(st["lane_bail_reads"].get(code, 0) <= v for code, v in st0["lane_bail_reads"].items())
    assert set(st["lane_bail_reads"]) <= set(st0["lane_bail_reads"])
    A.set_pipeline("exact=2")
    got2, st2 = run_twice(A, reads, want, (len(cls.span), len(cls.path), 0))
    assert got2 == got
    assert all(st["lane_bail_reads"].get(code, 0) <= v for code, v in st2["lane_bail_reads"].items())


def refused_candidate(G, j):
    """a read k_lane_exact_labeled lists and k_lane_exact_sub_labeled turns away: an insertion (the walk fails), or a walked node
    with two labels / with none (the mapped nodes all carry { 0 })"""
    kind = j % 3
    if kind == 0:
        a = SLW.free_read(j)
        r = G[a:a + 100]
        return r[:50] + SLW._other(r[50], r[49]) + r[50:99]
    s = dict(SLW.ROW_SITES)["two" if kind == 1 else "none"]
    at = 40 + j % 30
    return SLW._sub(G[s - at:s - at + 100], at)


@pytest.mark.parametrize("n_cand", [0, 1, 64, 65])
def test_candidate_lists_at_the_edges_of_a_wavefront(n_cand):
    """n_cand candidates among perfect reads: every second one a class read, the others turned away by the walking kernel"""
    g, anno, _ = SLW.directed_world(K)
    G = SLW.genome(K)
    reads = [G[SLW.free_read(i):SLW.free_read(i) + 100] for i in range(70)]
    for j in range(n_cand):
        reads.insert(j, SLW.class_read(G, j) if j % 2 == 0 else refused_candidate(G, j))
    cfg = capi.config_cli(K)
    cls, want = SLW.check_closed_form(g, anno, cfg, reads)
    assert len(cls.sub) == (n_cand + 1) // 2 and len(cls.path) == 70 and not cls.span
    assert len(cls.refused_row | cls.refused_walk) == n_cand // 2
    A = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=3")
    run_twice(A, reads, want, (0, 70, len(cls.sub)))


def test_every_read_of_a_label_aware_batch_leaves_through_the_exit_at_level_3():
    """class reads only (and a few perfect ones): k_lane is not launched at all"""
    g, anno, _ = SLW.directed_world(K)
    G = SLW.genome(K)
    cfg = capi.config_cli(K)
    reads = [SLW.class_read(G, i) for i in range(90)] + [G[SLW.free_read(i):SLW.free_read(i) + 100] for i in range(10)]
    cls, want = SLW.check_closed_form(g, anno, cfg, reads)
    assert len(cls.sub) == 90 and len(cls.path) == 10
    A = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=3")
    before = lane_launches()
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == want
    assert counters(st) == (0, 10, 90) and st["n_lane_reads"] == 100 and not st["lane_bail_reads"]
    assert st["n_lane_columns"] == 0 and st["n_extensions"] == 0 and lane_launches() == before
    A.set_pipeline("exact=2")
    got2, _ = A.align_batch(reads)
    st2 = A.stats()
    assert got2 == got and lane_launches() == before + 1 and counters(st2) == (0, 10, 0) and st2["n_lane_columns"] > 0


def test_a_label_on_a_dummy_nodes_row_keeps_the_lane_and_the_exit_off_at_level_3():
    g, anno, rows = SLW.directed_world(K)
    cfg = capi.config_cli(K)
    reads = [r[1] for r in rows]
    o = orc.LabeledAlignRun(g, cfg, anno, reads, validate=False)
    assert o.error == "", o.error
    W = g.export()[0]
    dummy = next(v for v in range(1, g.n_edges + 1) if W[v] == 0)
    cols = [anno.column_words(j) for j in range(anno.n_labels)]
    cols[2][(dummy - 1) >> 6] |= np.uint64(1) << np.uint64((dummy - 1) & 63)         # (the oracle never looks at a dummy node's row)
    A = aligner.Aligner(gpu_graph(g), cfg, annotation=aligner.Annotation(g.n_edges, cols))
    for opt in ("lane=1", "multi_pass=0", "exact=3"):
        A.set_pipeline(opt)
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == with_labels(o)
    assert not (st["extend_kernels"] & capi.KERNEL_LANE)
    assert st["n_lane_reads"] == 0 and counters(st) == (0, 0, 0)


def test_the_label_aware_batch_just_above_the_automatic_threshold_at_level_3():
    g, anno, reads = segment_batch(40000)
    cfg = capi.config_cli(31)
    A = labeled_handle(g, anno, cfg, "exact=3")
    blob, offs = aligner.pack_queries(reads)
    sample = list(range(0, len(reads), len(reads) // 300))
    arr, got = run_arrays(A, blob, offs, len(reads), sample)
    st = A.stats()
    assert not arr["status"].any() and st["extend_kernels"] & capi.KERNEL_LANE
    print("span:", st["n_lane_exact_reads"], "path:", st["n_lane_exact_path_reads"], "sub:", st["n_lane_exact_sub_reads"],
          "lane:", st["n_lane_reads"], "of", len(reads))
    assert st["n_lane_exact_sub_reads"] > 0 and st["n_lane_exact_path_reads"] > 0
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    arr_b, _ = run_arrays(A, blob, offs, len(reads), [])
    assert same_arrays(arr_b, arr) and counters(A.stats()) == counters(st)
    A.set_pipeline("exact=2")
    arr2, got2 = run_arrays(A, blob, offs, len(reads), sample)
    st2 = A.stats()
    assert same_arrays(arr2, arr) and got2 == got
    assert counters(st2) == (st["n_lane_exact_reads"], st["n_lane_exact_path_reads"], 0)
    assert all(st["lane_bail_reads"].get(c, 0) <= v for c, v in st2["lane_bail_reads"].items())
    # the oracle runs label-aware batches on one thread: the sample, against the big batch's results ...
    sreads = [reads[q] for q in sample]
    cls, want = SLW.check_closed_form(g, anno, cfg, sreads)
    for i, q in enumerate(sample):
        assert got[i] == want[i], (q, reads[q], got[i], want[i])
    assert cls.sub and cls.path
    # ... and as a batch of its own, where the three counters are the predicate's counts
    B = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=3")
    gots, status = B.align_batch(sreads)
    assert all(s == 0 for s in status) and gots == want
    assert counters(B.stats()) == (len(cls.span), len(cls.path), len(cls.sub)), (B.stats(), len(cls.span), len(cls.path), len(cls.sub))
    # the automatic default
    A.set_pipeline("exact=-1")
    arr_a, _ = run_arrays(A, blob, offs, len(reads), [])
    st_a = A.stats()
    assert same_arrays(arr_a, arr)
    assert st_a["n_lane_exact_path_reads"] == st["n_lane_exact_path_reads"]
    assert st_a["n_lane_exact_sub_reads"] == (st["n_lane_exact_sub_reads"] if AUTO_LEVEL_3_FOR_LABEL_AWARE_BATCHES else 0)
