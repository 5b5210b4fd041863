"""The lane extender's exact exit on label-aware batches on the GPU (k_lane_exact_labeled in mgx_lane.hip; lane_read.hpp
lane_exact_class(): the one-label seed filter, the conditions of the two classes, every node of the path with the row { L }).
Small batches with lane=1, multi_pass=0 and exact=2 on the directed world of tests/lane_exact_label_worlds.py — reads of both
classes, reads refused for each row reason (another label, two labels with L among them, none), reads with substitutions, without
seeds, across a segment boundary and reads the lane hands over share wavefronts, on both strands, at 1, 63, 64, 65 and 129 reads —
against the oracle's LabeledAligner (alignments and label lists), against exact=0 on the same handle, both counters against the
predicate's counts and the hand-over histogram against the host model's per-read codes at level 0 (which exact=0 must show in
full, exact=2 restricted to the reads outside the classes).  Then: a batch that leaves through the exit entirely (k_lane is not
launched); an annotation with a label on a dummy node's row (lane and exit off); one batch just above the lane's automatic
threshold with segment labels, exact=2 against exact=0 array by array and against the oracle on a sample.
Every counter assertion for exact=2 fails where label-aware batches never take the exit.
(tests/test_lane_exact_labels.py runs the same per-read functions in the host model.)"""
import collections
import ctypes as C

import numpy as np
import pytest

import emu_drv
import lane_exact_label_worlds as LW
import orc
from labeled_worlds import with_labels
from metagraph_amd import aligner, capi
from test_gpu_labels import gpu_annotation
from test_gpu_parity import gpu_graph

pytestmark = pytest.mark.gpu


def lane_launches():
    """launches of k_lane since the library was loaded"""
    out = (C.c_uint64 * 5)()
    capi.lib().mgx_kernel_launch_counts(out)           # grp8, grp8_prim, grp8_alt, ext64, lane
    return int(out[4])


def histogram(codes):
    return {k: v for k, v in collections.Counter(codes).items() if k}


def model_codes(g, anno, cfg, reads, monkeypatch):
    """per read: the hand-over code of the lane with the exit off, from the host model (0: the lane finishes the read)"""
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", "0")
    e = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads, annotation=emu_drv.EmuAnnotation(anno))
    assert e.error == "" and e.lane_stats()[0], e.error
    return e.lane_reasons()


def labeled_handle(g, anno, cfg, *options):
    A = aligner.Aligner(gpu_graph(g), cfg, annotation=gpu_annotation(anno))
    for opt in options:
        A.set_pipeline(opt)
    return A


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_label_aware_batches_at_level_2(n, monkeypatch):
    g, anno, named = LW.mixed_batch(n)
    names, reads = [x[0] for x in named], [x[1] for x in named]
    cfg = capi.config_cli(g.k)
    cls, want = LW.check_closed_form(g, anno, cfg, reads)
    both = set(cls.span) | set(cls.path)
    expected = model_codes(g, anno, cfg, reads, monkeypatch)
    outside = histogram(expected[q] for q in range(n) if q not in both)
    if n == 1:
        assert len(cls.path) == 1
    else:
        # both classes; outside them reads refused for each row reason, reads the DP finishes and reads it hands over
        assert cls.span and cls.path and len(both) < n and outside
        assert any(expected[q] == 0 for q in range(n) if q not in both)
        for kind in ("alt_other", "alt_two", "alt_none", "boundary", "substitution", "random"):
            assert any(nm.startswith(kind) and q not in both for q, nm in enumerate(names)), kind
        assert {0, 1} <= set(cls.path.values())
    A = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=2")
    for _ in range(2):                                        # (and again through the same handle: cursors and counters start afresh)
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        st = A.stats()
        for q in range(n):
            assert got[q] == want[q], (q, names[q], reads[q], got[q], want[q])
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
        assert st0["lane_bail_reads"] == histogram(expected), (st0["lane_bail_reads"], histogram(expected))
        assert st0["n_lane_reads"] + sum(st0["lane_bail_reads"].values()) == n
    # level 1: the span class alone
    A.set_pipeline("exact=1")
    got1, _ = A.align_batch(reads)
    st1 = A.stats()
    assert got1 == got and st1["n_lane_exact_reads"] == len(cls.span) and st1["n_lane_exact_path_reads"] == 0


def test_every_read_of_a_label_aware_batch_leaves_through_the_exit():
    """k_lane is not launched at all (its item count would be 0) and no column is computed"""
    g, anno, rows = LW.directed_world(21)
    cfg = capi.config_cli(21)
    reads = [r for name, r, kind in rows if kind == "in"]
    cls, want = LW.check_closed_form(g, anno, cfg, reads)
    assert len(cls.span) + len(cls.path) == len(reads) and cls.span and cls.path
    A = labeled_handle(g, anno, cfg, "lane=1", "multi_pass=0", "exact=2")
    before = lane_launches()
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == want
    assert st["n_lane_exact_reads"] == len(cls.span) and st["n_lane_exact_path_reads"] == len(cls.path)
    assert st["n_lane_reads"] == len(reads) and not st["lane_bail_reads"]
    assert st["n_lane_columns"] == 0 and st["n_extensions"] == 0 and lane_launches() == before
    A.set_pipeline("exact=0")
    got0, _ = A.align_batch(reads)
    assert got0 == got and lane_launches() == before + 1 and A.stats()["n_lane_columns"] > 0


def test_a_label_on_a_dummy_nodes_row_keeps_the_lane_and_the_exit_off():
    g, anno, rows = LW.directed_world(21)
    cfg = capi.config_cli(21)
    reads = [r[1] for r in rows]
    o = orc.LabeledAlignRun(g, cfg, anno, reads, validate=False)
    assert o.error == "", o.error
    W = g.export()[0]
    dummy = next(v for v in range(1, g.n_edges + 1) if W[v] == 0)
    cols = [anno.column_words(j) for j in range(anno.n_labels)]
    cols[2][(dummy - 1) >> 6] |= np.uint64(1) << np.uint64((dummy - 1) & 63)         # (the oracle never looks at a dummy node's row)
    A = aligner.Aligner(gpu_graph(g), cfg, annotation=aligner.Annotation(g.n_edges, cols))
    for opt in ("lane=1", "multi_pass=0", "exact=2"):
        A.set_pipeline(opt)
    got, status = A.align_batch(reads)
    st = A.stats()
    assert all(s == 0 for s in status) and got == with_labels(o)
    assert not (st["extend_kernels"] & capi.KERNEL_LANE)
    assert st["n_lane_reads"] == 0 and st["n_lane_exact_reads"] == 0 and st["n_lane_exact_path_reads"] == 0


def segment_batch(n, k=31, genome_len=50000, n_labels=50, read_len=100, snp_every=490, seed=31):
    """the benchmark's label-aware batch in small: one label per genome segment, widened by 15 positions; unlabeled SNP alleles;
    two thirds of the reads perfect"""
    import random
    from test_emu_vs_oracle import mutate, rand_seq, rc
    rng = random.Random(seed)
    G = rand_seq(rng, genome_len)
    seqs = [G]
    for p in range(k + rng.randrange(snp_every), genome_len - k, snp_every):
        seqs.append(G[p - k + 1:p] + rng.choice([c for c in "ACGT" if c != G[p]]) + G[p + 1:p + k])
    g = orc.Graph.build(k, seqs, 0, False)
    anno = orc.Annotation(g, n_labels)
    seg = genome_len // n_labels
    for j in range(n_labels):
        anno.annotate(G[max(0, j * seg - 15):min(genome_len, (j + 1) * seg + 15 + k - 1)], j)
    reads = []
    for i in range(n):
        p = rng.randrange(0, genome_len - read_len)
        r = G[p:p + read_len]
        if i % 3 == 2:
            r = mutate(rng, r, 0.01)
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return g, anno, reads


# whether the automatic default of the exit (no option exact) takes label-aware batches: lane_types.hpp LANE_EXACT_AUTO_LABELED, the
# decision the README's result paragraph records
AUTO_TAKES_LABEL_AWARE_BATCHES = True


def run_arrays(A, blob, offs, n, sample):
    """one batch -> (every array of the result as a copy, the decoded lists of the reads in `sample`)"""
    res = capi.Results()
    assert capi.lib().mgx_align_batch(A.h, blob, offs.ctypes.data, n, 0, C.byref(res)) == 0
    a = capi.results_arrays(res)
    out = {key: np.array(a[key], copy=True) for key in ("aln_begin", "alns", "nodes", "cigar", "seqs", "status")}
    n_lab = int(out["alns"]["n_labels"].sum()) if len(out["alns"]) else 0
    out["labels"] = np.ctypeslib.as_array(res.labels, shape=(n_lab,)).copy() if n_lab else np.zeros(0, np.uint32)
    decoded = []
    for q in sample:
        alns = []
        for x in out["alns"][int(out["aln_begin"][q]):int(out["aln_begin"][q + 1])]:
            cig = out["cigar"][int(x["cigar_begin"]):int(x["cigar_begin"]) + int(x["n_cigar"])]
            alns.append({"score": int(x["score"]), "offset": int(x["offset"]), "clipping": int(x["clipping"]),
                         "end_clipping": int(x["end_clipping"]), "num_matches": int(x["num_matches"]),
                         "nodes": [int(v) for v in out["nodes"][int(x["nodes_begin"]):int(x["nodes_begin"]) + int(x["n_nodes"])]],
                         "cigar": "".join("%d%s" % (int(c["len"]), capi.OP_CHARS[int(c["op"])]) for c in cig),
                         "sequence": out["seqs"][int(x["seq_begin"]):int(x["seq_begin"]) + int(x["seq_len"])].tobytes().decode(),
                         "orientation": int(x["orientation"]),
                         "labels": [int(v) for v in out["labels"][int(x["labels_begin"]):int(x["labels_begin"]) + int(x["n_labels"])]]})
        decoded.append(alns)
    return out, decoded


def same_arrays(a, b):
    return all(np.array_equal(a[key], b[key]) for key in a)


def test_the_label_aware_batch_just_above_the_automatic_threshold():
    g, anno, reads = segment_batch(40000)
    cfg = capi.config_cli(31)
    A = labeled_handle(g, anno, cfg, "exact=2")
    blob, offs = aligner.pack_queries(reads)
    sample = list(range(0, len(reads), len(reads) // 300))
    arr, got = run_arrays(A, blob, offs, len(reads), sample)
    st = A.stats()
    assert not arr["status"].any() and st["extend_kernels"] & capi.KERNEL_LANE
    print("path class:", st["n_lane_exact_path_reads"], "span class:", st["n_lane_exact_reads"], "lane:", st["n_lane_reads"], "of", len(reads))
    assert st["n_lane_exact_path_reads"] > 0 and st["n_lane_exact_reads"] == 0, st      # (reads of 100 characters: one seed per k-mer)
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    A.set_pipeline("exact=0")
    arr0, got0 = run_arrays(A, blob, offs, len(reads), sample)
    st0 = A.stats()
    assert st0["n_lane_exact_path_reads"] == 0 and st0["n_lane_exact_reads"] == 0
    assert same_arrays(arr0, arr) and got0 == got
    assert st0["n_lane_reads"] + sum(st0["lane_bail_reads"].values()) == len(reads)
    # the exit takes reads the DP would have finished or handed over; no other read's fate moves
    assert all(st["lane_bail_reads"].get(c, 0) <= v for c, v in st0["lane_bail_reads"].items())
    assert set(st["lane_bail_reads"]) <= set(st0["lane_bail_reads"])
    # the oracle runs label-aware batches on one thread: the sample
    cls, want = LW.check_closed_form(g, anno, cfg, [reads[q] for q in sample])
    for i, q in enumerate(sample):
        assert got[i] == want[i], (q, reads[q], got[i], want[i])
    assert cls.path
    # the automatic default
    A.set_pipeline("exact=-1")
    arr_a, _ = run_arrays(A, blob, offs, len(reads), [])
    st_a = A.stats()
    assert same_arrays(arr_a, arr)
    if AUTO_TAKES_LABEL_AWARE_BATCHES:
        assert st_a["n_lane_exact_path_reads"] == st["n_lane_exact_path_reads"] > 0
    else:
        assert st_a["n_lane_exact_path_reads"] == 0 and st_a["n_lane_exact_reads"] == 0
