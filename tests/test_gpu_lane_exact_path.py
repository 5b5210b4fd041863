"""The path class of the lane extender's exact exit on the GPU (level 2: k_lane_exact in mgx_lane.hip, exact_by_lanes in mgx.hip): a
read whose first seed starts at the query's first character and whose every k-mer is a node is finished in closed form between
seeding and the work sort, like the reads whose first seed spans the query; mgx_stats::n_lane_exact_path_reads counts these reads
apart, n_lane_exact_reads keeps counting the first class only.  Small batches with lane=1 and exact=2 on the graph of tests/
lane_cases.py (bubbles, a three-way fork, a segment on both strands) — reads of both classes, reads with substitutions, reads
without seeds and reads the lane hands over share wavefronts, at 1, 63, 64, 65 and 129 reads — against the oracle, against exact=0
on the same handle, both counters against the predicate's counts (tests/lane_exact_path_worlds.py: from the oracle's seeds and
mapping()) and the hand-over histogram against that of exact=0 restricted to the reads outside both classes.  Then the batch just
above the automatic threshold with default options: level 2 is the default there.
(tests/test_lane_exact_path.py runs the same per-read functions in the host model.)"""
import ctypes as C
import os

import pytest

import lane_cases as lc
import lane_exact_path_worlds as PW
import orc
from metagraph_amd import aligner, capi
from test_gpu_parity import gpu_graph
from test_lane_read import bench_like_world

pytestmark = pytest.mark.gpu


def lane_launches():
    """launches of k_lane since the library was loaded"""
    out = (C.c_uint64 * 5)()
    capi.lib().mgx_kernel_launch_counts(out)           # grp8, grp8_prim, grp8_alt, ext64, lane
    return int(out[4])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_batches_at_level_2(n):
    c, reads, expected = PW.mixed_batch(n)
    cls = PW.classes(c.graph, c.config, reads)
    want = cls.run.results()
    both = set(cls.span) | set(cls.path)
    outside = PW.histogram(expected[q] for q in range(n) if q not in both)
    # both classes, and outside them reads that finish in the DP and reads that leave for several reasons
    assert cls.span and (n == 1 or (cls.path and len(both) < n and len(outside) >= 2))
    A = aligner.Aligner(gpu_graph(c.graph), c.config, c.limits)
    for opt in ("lane=1", "multi_pass=0", "exact=2"):
        A.set_pipeline(opt)
    for _ in range(2):                                        # (and again through the same handle: cursors and counters start afresh)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        st = A.stats()
        for q in range(n):
            assert got[q] == want[q], (q, reads[q], got[q], want[q])
        assert st["extend_kernels"] & capi.KERNEL_LANE
        assert st["n_lane_exact_reads"] == len(cls.span), (st["n_lane_exact_reads"], len(cls.span))
        assert st["n_lane_exact_path_reads"] == len(cls.path), (st["n_lane_exact_path_reads"], len(cls.path))
        assert st["lane_bail_reads"] == outside, (st["lane_bail_reads"], outside)
        assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == n
    A.set_pipeline("exact=0")
    for _ in range(2):
        got0, status0 = A.align_batch(reads)
        st0 = A.stats()
        assert all(s == 0 for s in status0) and got0 == got
        assert st0["n_lane_exact_reads"] == 0 and st0["n_lane_exact_path_reads"] == 0
        assert st0["lane_bail_reads"] == PW.histogram(expected), (st0["lane_bail_reads"], PW.histogram(expected))
        assert st0["n_lane_reads"] + sum(st0["lane_bail_reads"].values()) == n


def test_every_read_of_a_batch_leaves_through_the_exit_at_level_2():
    """perfect reads across the bubbles and the three-way fork of the main world and reads from its feature-free start: both classes
    and nothing else, so k_lane is not launched at all (its item count would be 0)"""
    g = lc.main_world()[0]
    cfg = lc.cli()
    reads = [lc.plain(570 - j, 130) for j in range(10)] + [lc.plain(lc.FORK3 - 70 + j) for j in range(10)]
    reads += [r for r, _ in lc.plain_reads(50)]
    cls = PW.classes(g, cfg, reads)
    assert len(cls.path) == 20 and len(cls.span) == 50
    A = aligner.Aligner(gpu_graph(g), cfg)
    for opt in ("lane=1", "exact=2"):
        A.set_pipeline(opt)
    before = lane_launches()
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == cls.run.results()
    assert st["n_lane_exact_reads"] == 50 and st["n_lane_exact_path_reads"] == 20 and st["n_lane_reads"] == 70 and not st["lane_bail_reads"]
    assert st["n_lane_columns"] == 0 and st["n_extensions"] == 0 and lane_launches() == before
    # ... and with the exit off it is
    A.set_pipeline("exact=0")
    got0, _ = A.align_batch(reads)
    assert got0 == got and lane_launches() == before + 1


def test_the_batch_just_above_the_automatic_threshold_with_default_options():
    g, reads = bench_like_world(31, 40000, genome_len=50000, read_len=100, snp_every=490)
    cfg = capi.config_cli(31)
    A = aligner.Aligner(gpu_graph(g), cfg)
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and st["extend_kernels"] & capi.KERNEL_LANE
    cls = PW.classes(g, cfg, reads, orc.AlignRun(g, cfg, reads, threads=min(16, os.cpu_count() or 8), validate=False))
    print("first class", len(cls.span), "path class", len(cls.path), "of", len(reads))
    assert len(cls.path) > 0
    assert st["n_lane_exact_path_reads"] == len(cls.path), (st["n_lane_exact_path_reads"], len(cls.path))
    assert st["n_lane_exact_reads"] == len(cls.span), (st["n_lane_exact_reads"], len(cls.span))
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    assert got == cls.run.results()
    A.set_pipeline("exact=1")
    got1, status1 = A.align_batch(reads)
    st1 = A.stats()
    assert all(s == 0 for s in status1) and got1 == got
    assert st1["n_lane_exact_path_reads"] == 0 and st1["n_lane_exact_reads"] == len(cls.span)
    assert st1["n_lane_reads"] + sum(st1["lane_bail_reads"].values()) == len(reads)
