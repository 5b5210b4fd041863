"""The substitution class of the lane extender's exact exit on the GPU (level 3: k_lane_exact lists the candidates, k_lane_exact_sub
walks them and finishes the class reads — mgx_lane.hip, exact_by_lanes in mgx.hip): a read with one substitution behind its first k
characters, whose walk across the run of zeros succeeds, is finished in closed form between seeding and the work sort;
mgx_stats::n_lane_exact_sub_reads counts these reads apart, n_lane_exact_reads and n_lane_exact_path_reads keep counting their
classes only.  Small batches with lane=1 and exact=3 on the graph of tests/lane_cases.py — class reads, perfect reads of both
other classes, reads the walk turns away (an insertion, a substitution on a SNP site, two substitutions), reads without seeds and
reads the lane hands over share wavefronts, at 1, 63, 64, 65 and 129 reads — against the oracle, against exact=0 on the same handle,
the three counters against the predicate's counts (tests/lane_exact_sub_worlds.py: from the oracle's seeds, mapping() and
Graph.outgoing()).  Candidate lists of 0, 1, 64 and 65 entries; a batch of class reads only, for which k_lane is not launched; the
batch just above the automatic threshold with default options.
(tests/test_lane_exact_sub.py runs the same per-read functions in the host model.)"""
import ctypes as C
import os

import pytest

import lane_cases as lc
import lane_exact_path_worlds as PW
import lane_exact_sub_worlds as SW
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


def class_read(i):
    """a read from the feature-free stretch of the main world with one substitution behind its first K characters, either strand"""
    lo, hi = lc.CLEAN
    r = lc.plain(lo + (i * 13) % (hi - lo - 100))
    p = lc.K + (i * 7) % (100 - lc.K)                  # K .. 99: interior positions and the tail, the last character included
    r = r[:p] + lc._other(r[p]) + r[p + 1:]
    return r if i % 2 else PW.rc(r)


def turned_away(i):
    """candidates the walk (or the scan) turns away: an insertion, a substitution on a SNP site, two substitutions k apart"""
    G = lc.main_world()[1]
    lo = lc.CLEAN[0] + 5 * (i % 40)
    r = lc.plain(lo)
    kind = i % 3
    if kind == 0:
        return r[:50] + lc._other(r[50], r[49]) + r[50:99]
    if kind == 1:
        s = lc.SNP_TIE
        third = lc._other(G[s], lc._other(G[s]))
        return G[s - 60:s] + third + G[s + 1:s + 40]
    return r[:30] + lc._other(r[30]) + r[31:30 + lc.K] + lc._other(r[30 + lc.K]) + r[31 + lc.K:]


def mixed_batch(n):
    """tests/lane_exact_path_worlds.mixed_batch(n) with every fifth read a class read and every eleventh one the walk turns away
    -> (case, reads)"""
    c, reads, _ = PW.mixed_batch(n)
    reads = list(reads)
    for i in range(2, n, 5):
        reads[i] = class_read(i)
    for i in range(7, n, 11):
        reads[i] = turned_away(i)
    if n == 1:
        reads[0] = class_read(1)
    return c, reads


def run_twice(A, reads, want, counts):
    for _ in range(2):                                            # (and again through the same handle: cursors and counters start afresh)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        st = A.stats()
        for q in range(len(reads)):
            assert got[q] == want[q], (q, reads[q], got[q], want[q])
        assert (st["n_lane_exact_reads"], st["n_lane_exact_path_reads"], st["n_lane_exact_sub_reads"]) == counts, (st, counts)
        assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    return got, st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_batches_at_level_3(n):
    c, reads = mixed_batch(n)
    cls = SW.classes(c.graph, c.config, reads)
    want = cls.run.results()
    every = set(cls.span) | set(cls.path) | set(cls.sub)
    # all three classes, and outside them reads that finish in the DP and reads that leave
    assert cls.sub and (n == 1 or (cls.span and cls.path and len(every) < n))
    A = aligner.Aligner(gpu_graph(c.graph), c.config, c.limits)
    for opt in ("lane=1", "multi_pass=0", "exact=3"):
        A.set_pipeline(opt)
    got, st = run_twice(A, reads, want, (len(cls.span), len(cls.path), len(cls.sub)))
    assert st["extend_kernels"] & capi.KERNEL_LANE
    A.set_pipeline("exact=0")
    got0, st0 = run_twice(A, reads, want, (0, 0, 0))
    assert got0 == got
    # the reads outside the classes leave for the reasons they leave for with the exit off; class reads that left then are finished now
    assert all(st["lane_bail_reads"].get(code, 0) <= v for code, v in st0["lane_bail_reads"].items())
    A.set_pipeline("exact=2")
    run_twice(A, reads, want, (len(cls.span), len(cls.path), 0))


@pytest.mark.parametrize("n_cand", [0, 1, 64, 65])
def test_candidate_lists_at_the_edges_of_a_wavefront(n_cand):
    """n_cand candidates among perfect reads: every second one a class read, the others turned away by the walk"""
    reads = [r for r, _ in lc.plain_reads(70)]
    for j in range(n_cand):
        reads.insert(j, class_read(j) if j % 2 == 0 else turned_away(3 * j))      # (insertions: k zeros, listed, turned away)
    g, cfg = lc.main_world()[0], lc.cli()
    cls = SW.classes(g, cfg, reads)
    assert len(cls.sub) == (n_cand + 1) // 2 and len(cls.span) == 70
    A = aligner.Aligner(gpu_graph(g), cfg)
    for opt in ("lane=1", "multi_pass=0", "exact=3"):
        A.set_pipeline(opt)
    run_twice(A, reads, cls.run.results(), (70, 0, len(cls.sub)))


@pytest.mark.parametrize("cname", ["cli", "ti_tv"])
def test_two_snps_less_than_k_apart_in_the_tail(cname):
    """reads that recombine two SNPs d < k apart: with the second one in the last k characters there are two alignments with one
    mismatch (under ti_tv the other one scores more for some): the exit leaves them to the DP; results are the oracle's"""
    g, rows = SW.recombinant_world(21)
    reads = [r[1] for r in rows]
    cfg = SW.configurations(21, 100)[cname]
    cls = SW.classes(g, cfg, reads)
    assert all(q not in cls.sub for q, r in enumerate(rows) if r[2] == "out")
    A = aligner.Aligner(gpu_graph(g), cfg)
    for opt in ("lane=1", "multi_pass=0", "exact=3"):
        A.set_pipeline(opt)
    run_twice(A, reads, cls.run.results(), (len(cls.span), len(cls.path), len(cls.sub)))


def test_every_read_of_a_batch_leaves_through_the_exit_at_level_3():
    """class reads only (and a few perfect ones): k_lane is not launched at all"""
    g, cfg = lc.main_world()[0], lc.cli()
    reads = [class_read(i) for i in range(90)] + [r for r, _ in lc.plain_reads(10)]
    cls = SW.classes(g, cfg, reads)
    assert len(cls.sub) == 90 and len(cls.span) == 10
    A = aligner.Aligner(gpu_graph(g), cfg)
    for opt in ("lane=1", "exact=3"):
        A.set_pipeline(opt)
    before = lane_launches()
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == cls.run.results()
    assert st["n_lane_exact_sub_reads"] == 90 and st["n_lane_exact_reads"] == 10 and st["n_lane_reads"] == 100 and not st["lane_bail_reads"]
    assert st["n_lane_columns"] == 0 and st["n_extensions"] == 0 and lane_launches() == before
    A.set_pipeline("exact=2")
    got2, _ = A.align_batch(reads)
    assert got2 == got and lane_launches() == before + 1


def test_the_batch_just_above_the_automatic_threshold_with_default_options():
    """level 3 is the automatic default for unlabeled batches: the three counters match the predicate; exact=3 gives the same"""
    g, reads = bench_like_world(31, 40000, genome_len=50000, read_len=100, snp_every=490)
    cfg = capi.config_cli(31)
    A = aligner.Aligner(gpu_graph(g), cfg)
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and st["extend_kernels"] & capi.KERNEL_LANE
    cls = SW.classes(g, cfg, reads, orc.AlignRun(g, cfg, reads, threads=min(16, os.cpu_count() or 8), validate=False))
    print("first class", len(cls.span), "path class", len(cls.path), "substitution class", len(cls.sub), "of", len(reads))
    assert len(cls.sub) > 1000
    assert st["n_lane_exact_sub_reads"] == len(cls.sub), (st["n_lane_exact_sub_reads"], len(cls.sub))      # (the default is level 3)
    assert st["n_lane_exact_path_reads"] == len(cls.path) and st["n_lane_exact_reads"] == len(cls.span)
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    assert got == cls.run.results()
    A.set_pipeline("exact=3")
    got3, status3 = A.align_batch(reads)
    st3 = A.stats()
    assert all(s == 0 for s in status3) and got3 == got
    assert (st3["n_lane_exact_reads"], st3["n_lane_exact_path_reads"], st3["n_lane_exact_sub_reads"]) == (len(cls.span), len(cls.path), len(cls.sub))
    assert st3["n_lane_reads"] + sum(st3["lane_bail_reads"].values()) == len(reads)
