"""The lane-per-read seeder on the GPU (mgx_seedlane.hip, seed_by_lanes in mgx.hip) at its leave reasons, buffer limits and batch
shapes: the directed worlds of tests/seed_lane_cases.py, whose per-read fates tests/test_seed_lane_edges.py pins in the host
model.  Per case: seeds, num_matching and alignments of every read against the oracle, and the kernel's histogram of leave reasons
against the case's, key for key — the leave list filled from both ends, the second pass reading it, the seed-stream space handed
out per wavefront, the cursors between passes and batches are all in the way of those numbers."""
import collections

import pytest

import orc
import seed_lane_cases as slc
from emu_drv import oracle_seeds_as_tuples
from labeled_worlds import labeled_world, with_labels
from metagraph_amd import aligner, capi
from test_gpu_parity import gpu_graph

pytestmark = pytest.mark.gpu

SEEDER_STATS = ("n_seed_lane_reads", "seed_lane_left_reads", "n_seeds")


def histogram(expected):
    return {k: v for k, v in collections.Counter(expected).items() if k}


def check_batch(A, o, reads, expected):
    """one batch through handle A against the oracle run o and the expected fates -> (results, the seeder's statistics)"""
    got, status = A.align_batch(reads)
    assert all(s == 0 for s in status), status
    st = A.stats()
    info = A.seed_info(len(reads))
    for strand in (0, 1):
        for q, (ss, nm) in enumerate(o.seeds(strand)):
            assert info[q]["num_matches"][strand] == nm, (q, strand, reads[q])
            assert info[q]["seeds"][strand] == oracle_seeds_as_tuples(ss), (q, strand, reads[q])
    want = o.results()
    for q in range(len(reads)):
        assert got[q] == want[q], (q, reads[q], got[q], want[q])
    if expected is not None:
        assert st["seed_lane_left_reads"] == histogram(expected), (st["seed_lane_left_reads"], histogram(expected))
        assert st["n_seed_lane_reads"] + sum(st["seed_lane_left_reads"].values()) == len(reads)
    return got, {k: st[k] for k in SEEDER_STATS}


@pytest.mark.parametrize("name", list(slc.CASES))
def test_case(name):
    c = slc.CASES[name]()
    o = orc.AlignRun(c.graph, c.config, c.reads, threads=8, validate=False)
    assert o.error == "", o.error
    G = gpu_graph(c.graph)
    seeds = []
    for options in (("seed_lane=1",), ("seed_lane=1", "lane=1"), ("seed_lane=0",)):
        A = aligner.Aligner(G, c.config, c.limits)
        for opt in options:
            A.set_pipeline(opt)
        A.keep_seeds(True)
        _, st = check_batch(A, o, c.reads, c.expected if options[0] == "seed_lane=1" else None)
        seeds.append(st["n_seeds"])
        if options[0] == "seed_lane=0":
            assert st["n_seed_lane_reads"] == 0 and not st["seed_lane_left_reads"]
    assert seeds[0] == seeds[2] and seeds[1] == seeds[2], seeds        # the seeds counter: with and without the lane seeder


def test_one_handle_batches_of_different_shape():
    """all leave, none leave, 65 mixed, then the first again through one handle: results and every seeder statistic of the
    fourth call equal those of the first (cursors, lists and histogram start afresh per batch)"""
    cases = [slc.shape_all_leave_both(), slc.shape_none_leave(), slc.shape_n(65)]
    A = aligner.Aligner(gpu_graph(cases[0].graph), cases[0].config)
    A.set_pipeline("seed_lane=1")
    A.keep_seeds(True)
    runs = [orc.AlignRun(c.graph, c.config, c.reads, threads=8, validate=False) for c in cases]
    first = None
    for x in (0, 1, 2, 0):
        out = check_batch(A, runs[x], cases[x].reads, cases[x].expected)
        if first is None:
            first = out
    assert out == first


def test_label_aware_batch():
    """label-aware alignment runs one seed per k-mer (max_seed_length == k: the "many" buffer sizes): the same answers with and
    without the lane seeder, every read accounted for"""
    k = 15
    g, anno, reads = labeled_world(23, k, n_strains=3, genome_len=3000, n_reads=200)
    cfg = capi.config_cli(k)
    want = with_labels(orc.LabeledAlignRun(g, cfg, anno, reads))
    W, last, F, valid = g.export()
    G = aligner.Graph(k, W, last, F, valid)
    AN = aligner.Annotation(g.n_edges, [anno.column_words(j) for j in range(anno.n_labels)])
    stats = []
    for opt in ("seed_lane=1", "seed_lane=0"):
        A = aligner.Aligner(G, cfg, annotation=AN)
        A.set_pipeline(opt)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        assert got == want
        stats.append(A.stats())
    assert stats[0]["n_seed_lane_reads"] > 0
    assert stats[0]["n_seed_lane_reads"] + sum(stats[0]["seed_lane_left_reads"].values()) == len(reads)
    assert stats[1]["n_seed_lane_reads"] == 0
    assert stats[0]["n_seeds"] == stats[1]["n_seeds"]
