"""The exact exit of the lane-per-read extender on the GPU (k_lane_exact in mgx_lane.hip, exact_by_lanes in mgx.hip): reads whose
first seed spans the query are finished in closed form between seeding and the work sort, get the work key that sorts them
behind everything else, and k_lane is launched on the items in front of them.  Small batches with lane=1 and exact=1 — mixed of
class reads, reads with substitutions, reads without seeds and reads the lane hands over, at 1, 63, 64, 65 and 129 reads — against
the oracle, against exact=0 on the same handle, the counter against the predicate's count (tests/lane_exact_worlds.py: from the
oracle's seeds) and the hand-over histogram of exact=0 against the fates tests/lane_cases.py pins.  Then one batch just above
the automatic threshold with default options: the only place where the sort behind the exit and the default rule are exercised.
(The output stream is sized for L + L / 4 + 40 words per read and a class read takes L - k + 2 + ceil(L / 4): these reads cannot
overflow it on their own, so the capacity status of the exit is tested where the capacity can be set — tests/test_lane_exact.py.)
(tests/test_lane_exact.py runs the same per-read functions in the host model.)"""
import collections
import os
import random

import pytest

import lane_cases as lc
import lane_exact_worlds as W
import orc
from metagraph_amd import aligner, capi
from test_emu_vs_oracle import rand_seq
from test_gpu_parity import gpu_graph
from test_lane_read import bench_like_world

pytestmark = pytest.mark.gpu


def mixed_batch(n):
    """the shape of tests/lane_cases.py at n reads (of six: three plain — the class —, one with substitutions, two that the lane
    hands over, perfect ones among them), every ninth read replaced by a random one (no seeds) -> (case, reads, expected codes)"""
    c = lc.CASES["shape_%d" % n]() if "shape_%d" % n in lc.CASES else lc.shape_n(n)
    rng = random.Random(900 + n)
    reads, expected = list(c.reads), list(c.expected)
    for i in range(8, n, 9):
        reads[i], expected[i] = rand_seq(rng, 100), 0
    return c, reads, expected


def histogram(codes):
    return {k: v for k, v in collections.Counter(codes).items() if k}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_batches_with_the_exit_forced(n):
    c, reads, expected = mixed_batch(n)
    cls, o = W.class_reads(c.graph, c.config, reads)
    want = o.results()
    assert cls and (n == 1 or (len(cls) < n and len(histogram(expected[q] for q in range(n) if q not in cls)) >= 4))
    A = aligner.Aligner(gpu_graph(c.graph), c.config, c.limits)
    for opt in ("lane=1", "multi_pass=0", "exact=1"):
        A.set_pipeline(opt)
    for _ in range(2):                                        # (and again through the same handle: cursors and counters start afresh)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        st = A.stats()
        for q in range(n):
            assert got[q] == want[q], (q, reads[q], got[q], want[q])
        assert st["extend_kernels"] & capi.KERNEL_LANE
        assert st["n_lane_exact_reads"] == len(cls), (st["n_lane_exact_reads"], len(cls))
        # every other read's fate is what it was; a class read is finished whatever the DP would have done with it
        assert st["lane_bail_reads"] == histogram(expected[q] for q in range(n) if q not in cls), st["lane_bail_reads"]
        assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == n
    A.set_pipeline("exact=0")
    got0, status0 = A.align_batch(reads)
    st0 = A.stats()
    assert all(s == 0 for s in status0) and got0 == got
    assert st0["n_lane_exact_reads"] == 0
    assert st0["lane_bail_reads"] == histogram(expected), (st0["lane_bail_reads"], histogram(expected))      # as before the exit existed
    assert st0["n_lane_reads"] + sum(st0["lane_bail_reads"].values()) == n
    # automatic: off for a batch the lane kernel takes only because it is forced
    A.set_pipeline("exact=-1")
    got_a, _ = A.align_batch(reads)
    assert got_a == got and A.stats()["n_lane_exact_reads"] == 0 and A.stats()["lane_bail_reads"] == histogram(expected)


def test_every_read_of_a_batch_leaves_through_the_exit():
    """k_lane is not launched at all (its item count would be 0)"""
    c = lc.CASES["shape_none_leave"]()
    cls, o = W.class_reads(c.graph, c.config, c.reads)
    assert len(cls) == len(c.reads)
    A = aligner.Aligner(gpu_graph(c.graph), c.config, c.limits)
    for opt in ("lane=1", "exact=1"):
        A.set_pipeline(opt)
    got, status = A.align_batch(c.reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == o.results()
    assert st["n_lane_exact_reads"] == st["n_lane_reads"] == len(c.reads) and not st["lane_bail_reads"]


def test_lengths_strands_and_reads_that_stay_out():
    g, reads = W.world_lengths()
    cfg = capi.config_cli(g.k)
    cls, o = W.class_reads(g, cfg, reads)
    A = aligner.Aligner(gpu_graph(g), cfg)
    for opt in ("lane=1", "exact=1"):
        A.set_pipeline(opt)
    got, status = A.align_batch(reads)
    assert all(s == 0 for s in status) and got == o.results()
    assert A.stats()["n_lane_exact_reads"] == len(cls) == 48


def test_a_batch_just_above_the_automatic_threshold_with_default_options():
    g, reads = bench_like_world(31, 40000, genome_len=50000, read_len=100, snp_every=490)
    cfg = capi.config_cli(31)
    A = aligner.Aligner(gpu_graph(g), cfg)
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and st["extend_kernels"] & capi.KERNEL_LANE
    cls, o = W.class_reads(g, cfg, reads, orc.AlignRun(g, cfg, reads, threads=os.cpu_count() or 8, validate=False))
    assert len(cls) > 0.15 * len(reads)
    assert st["n_lane_exact_reads"] == len(cls), (st["n_lane_exact_reads"], len(cls))
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    A.set_pipeline("exact=0")
    got0, status0 = A.align_batch(reads)
    st0 = A.stats()
    assert all(s == 0 for s in status0) and got0 == got and st0["n_lane_exact_reads"] == 0
    assert st0["n_lane_reads"] + sum(st0["lane_bail_reads"].values()) == len(reads)
    assert got == o.results()
    # below the threshold the lane kernel is not the automatic choice, and neither is the exit
    A.set_pipeline("exact=-1")
    got_s, _ = A.align_batch(reads[:500])
    assert got_s == got[:500] and A.stats()["n_lane_exact_reads"] == 0 and not (A.stats()["extend_kernels"] & capi.KERNEL_LANE)
