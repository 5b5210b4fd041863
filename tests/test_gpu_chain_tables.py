"""The chain stage of LabeledAligner's coordinate mode on the device (mgx_seed_chainer_create / mgx_chain_tables_batch,
csrc/mgx_chaintab.hip) against the judge of coord_chain_worlds.py: every array of mgx_chain_tables — the seeds filter_seeds keeps
with their nodes and num_matching, the sorted anchors with their final chain scores, the back pointers, the statuses.
Needs a real MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import coord_chain_worlds as ccw
import orc
from metagraph_amd import aligner, capi

pytestmark = pytest.mark.gpu

N_WORLDS = 20
NID = 0xFFFFFFFF


class World:
    """an oracle graph + annotation with their device copies"""

    def __init__(self, g, anno, reads, mode=0):
        self.g, self.anno, self.reads = g, anno, reads
        W, last, F, valid = g.export()
        self.G = aligner.Graph(g.k, W, last, F, valid, mode=mode)
        self.A = ccw.device_annotation(g, anno)

    def chainer(self, cfg, *options):
        S = aligner.SeedChainer(self.G, cfg, self.A)
        for opt in options:
            S.set_pipeline(opt)
        return S


@pytest.fixture(scope="module")
def worlds():
    return [World(*ccw.make_world(seed)) for seed in range(N_WORLDS)]


def flatten(lists):
    """judge lists -> the arrays of aligner.SeedChainer.chain_tables (nodes in seed order)"""
    seeds = [s for l in lists for s in l["seeds"]]
    anchors = [a for l in lists for a in l["anchors"]]
    return {"seed_count": np.array([len(l["seeds"]) for l in lists], dtype=np.uint64),
            "anchor_count": np.array([len(l["anchors"]) for l in lists], dtype=np.uint64),
            "seed_meta": np.array([(s[0], s[1], s[2], len(s[3])) for s in seeds], dtype=np.uint32).reshape(-1, 4),
            "seed_nodes": np.array([v for s in seeds for v in s[3]], dtype=np.uint64),
            "num_matching": np.array([l["num_matching"] for l in lists], dtype=np.uint64),
            "anchors": np.array(anchors, dtype=np.int64).reshape(-1, 6),
            "backtrace": np.array([b for l in lists for b in l["backtrace"]], dtype=np.uint32)}


def tiled(flat, reps):
    return {key: np.concatenate([v] * reps) if reps else v[:0] for key, v in flat.items()}


def device_flat(arrays):
    s = arrays["seeds"]
    cnt, starts = s["n_nodes"].astype(np.int64), s["nodes_begin"].astype(np.int64)
    idx = np.repeat(starts - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
    a = arrays["anchors"]
    return {"seed_count": np.diff(arrays["seed_begin"]), "anchor_count": np.diff(arrays["list_begin"]),
            "seed_meta": np.stack([s["clipping"], s["length"], s["offset"], s["n_nodes"]], axis=1).astype(np.uint32).reshape(-1, 4),
            "seed_nodes": arrays["nodes"][idx] if len(idx) else np.zeros(0, dtype=np.uint64),
            "num_matching": arrays["num_matching"],
            "anchors": np.stack([a["label"].astype(np.int64), a["coordinate"], a["seed_clipping"].astype(np.int64), a["seed_end"].astype(np.int64),
                                 a["chain_score"].astype(np.int64), a["seed_index"].astype(np.int64)], axis=1).reshape(-1, 6),
            "backtrace": arrays["backtrace"]}


def check(got, want_lists, reps=1, what=""):
    """every array of the device's tables against the judge's lists (repeated reps times)"""
    arrays, status = got
    assert status == [0] * (len(want_lists) // 2 * reps), (what, status[:16])
    assert arrays["n"] == len(status) and int(arrays["seed_begin"][0]) == 0 and int(arrays["list_begin"][0]) == 0
    dev, want = device_flat(arrays), tiled(flatten(want_lists), reps)
    for key in ("seed_count", "anchor_count", "num_matching", "seed_meta", "seed_nodes", "anchors", "backtrace"):
        if dev[key].shape == want[key].shape and np.array_equal(dev[key], want[key]):
            continue
        # the first list that differs, spelled out
        got_lists = aligner.chain_lists(arrays)
        for l, (x, y) in enumerate(zip(got_lists, want_lists * reps)):
            assert x == y, (what, key, "list", l, "device", x, "judge", y)
        raise AssertionError((what, key, dev[key].shape, want[key].shape))


@pytest.mark.parametrize("config", sorted(ccw.CONFIGS))
def test_worlds_match_the_judge(worlds, config):
    cfg = ccw.make_config(config)
    stats = {}
    for i, w in enumerate(worlds):
        check(w.chainer(cfg).chain_tables(w.reads), ccw.judge(w.g, cfg, w.anno, w.reads, stats), what=(config, i))
    assert stats["duplicate_sort_keys"] == 0 and stats["lists_with_a_back_pointer"] > 0, stats
    if config == "exact_match":
        assert stats["labels_dropped_with_one_kept"] > 0 and stats["lists_without_seeds"] > 0, stats
    if config == "one_per_locus":
        assert stats["tuples_cut"] > 0, stats
    if config == "recipe":
        assert stats["sub_k_seeds"] > 0 and stats["multi_coordinate_pairs"] >= 20, stats


@pytest.mark.parametrize("kat", ccw.kat_worlds(), ids=lambda w: w[0])
def test_kat_worlds(kat):
    name, g, anno, cfg, reads = kat
    w = World(g, anno, reads)
    check(w.chainer(cfg).chain_tables(reads), ccw.judge(g, cfg, anno, reads), what=name)


def test_the_handles_config_is_what_labeled_aligner_leaves(worlds):
    w = worlds[0]
    cfg = ccw.make_config("recipe")
    assert cfg.global_xdrop == 1 and cfg.chain_alignments == 0 and cfg.max_seed_length == 0
    c = w.chainer(cfg).get_config()
    assert (c.global_xdrop, c.chain_alignments, c.min_seed_length, c.max_seed_length) == (0, 1, 7, ccw.K)


@pytest.mark.parametrize("seed_lane", [1, 0])
def test_both_seeding_paths(worlds, seed_lane):
    w = worlds[1]
    cfg = ccw.make_config("recipe")
    S = w.chainer(cfg, "seed_lane=%d" % seed_lane)
    got = S.chain_tables(w.reads)
    st = S.stats()
    assert (st["n_seed_lane_reads"] > 0) == bool(seed_lane), st
    assert st["n_reads"] == len(w.reads)
    check(got, ccw.judge(w.g, cfg, w.anno, w.reads), what="seed_lane=%d" % seed_lane)


def test_batch_shapes(worlds):
    w = worlds[2]
    cfg = ccw.make_config("recipe")
    want = ccw.judge(w.g, cfg, w.anno, w.reads)
    S = w.chainer(cfg)
    # an empty batch
    arrays, status = S.chain_tables([])
    assert status == [] and arrays["n"] == 0 and arrays["seed_begin"].tolist() == [0] and arrays["list_begin"].tolist() == [0]
    assert len(arrays["seeds"]) == 0 and len(arrays["anchors"]) == 0
    # one read, then 65 on the same handle (the buffers grow)
    check(S.chain_tables(w.reads[:1]), want[:2], what="one read")
    reads65 = (w.reads * 3)[:65]
    check(S.chain_tables(reads65), (want * 3)[:130], what="65 reads")
    # a permuted batch gives permuted results
    perm = list(range(len(w.reads)))
    random.Random(4).shuffle(perm)
    check(S.chain_tables([w.reads[p] for p in perm]), [want[2 * p + s] for p in perm for s in (0, 1)], what="permuted")
    # ... and a smaller batch after a larger one
    check(S.chain_tables(w.reads[:3]), want[:6], what="three reads after 65")


def test_three_thousand_reads(worlds):
    w = worlds[3]
    cfg = ccw.make_config("recipe")
    check(w.chainer(cfg).chain_tables(w.reads * 125), ccw.judge(w.g, cfg, w.anno, w.reads), reps=125, what="3000 reads")


def test_reads_without_seeds_among_the_others(worlds):
    """reads shorter than k, all-N reads and lower-case reads next to ordinary ones"""
    w = worlds[4]
    cfg = ccw.make_config("recipe")
    reads = [w.reads[0], "ACGTA", "N" * 100, w.reads[1].lower(), "", "A" * ccw.K, w.reads[2], "n" * 30 + w.reads[4][30:], "ACGTACGTAC"]
    want = ccw.judge(w.g, cfg, w.anno, reads)
    assert not want[2]["seeds"] and not want[4]["seeds"] and want[6]["seeds"] == ccw.judge(w.g, cfg, w.anno, [w.reads[1]])[0]["seeds"]
    check(w.chainer(cfg).chain_tables(reads), want, what="odd reads")
    # a batch of nothing but reads shorter than k
    short = ["ACGT", "", "ACGTACGTAC"]
    check(w.chainer(cfg).chain_tables(short), ccw.judge(w.g, cfg, w.anno, short), what="short reads")


def test_labels_on_rows_of_dummy_nodes():
    """The device annotation carries labels and coordinates on the rows of the graph's dummy nodes (W == 0), which the reference's
    AnnotationBuffer never hands out (annotation_buffer.cpp:64-68) and the oracle's annotation does not have.  "No dummy node's row
    holds a label" is then false for this annotation, so every row a seed reads goes through the W test — and the tables are the
    judge's all the same.  (No seed can start at such a node: its k-mer ends in '$'.  What this covers is the test itself running
    on the real nodes' rows; with the flag set, as in every other world, the kernels skip it.)"""
    g, anno, reads = ccw.make_world(8)
    W, last, F, valid = g.export()
    dummies = [i for i in range(1, len(W)) if W[i] == 0]
    assert dummies and all(not ccw.row_tuples(anno, i - 1, {}) for i in dummies)
    w = World.__new__(World)
    w.g, w.anno, w.reads = g, anno, reads
    w.G = aligner.Graph(g.k, W, last, F, valid)
    w.A = ccw.device_annotation(g, anno, extra=[(i - 1, lab, [7 + i, 5000 + i]) for i in dummies for lab in (0, 2)])
    assert [t for t in w.A.get_row_tuples([i - 1 for i in dummies]) if t] != []
    for config in ("recipe", "exact_match"):
        cfg = ccw.make_config(config)
        check(w.chainer(cfg).chain_tables(reads), ccw.judge(g, cfg, anno, reads), what=("dummy rows", config))


def test_a_list_beyond_the_lds_limit_of_chain_seeds():
    """one error-free 2000-bp read of a 2600-bp genome that four labels carry, k = 17: 1984 forward seeds, 7936 anchors in one
    list — more than the 6144 mgx_chain_seeds keeps in LDS"""
    rng = random.Random(11)
    k = 17
    genome = ccw.rand_seq(rng, 2600)
    g, anno = ccw.annotated(k, [genome] * 4, [0, 1, 2, 3], [0, 10000, 20000, 30000])
    read = genome[300:2300]
    cfg = orc.make_config({}, ccw.MATRIX)
    want = ccw.judge(g, cfg, anno, [read])
    assert len(want[0]["seeds"]) == 1984 and len(want[0]["anchors"]) == 7936
    assert sum(1 for b in want[0]["backtrace"] if b != NID) > 7000
    check(World(g, anno, [read]).chainer(cfg).chain_tables([read]), want, what="7936 anchors")


def test_on_device_then_fetch_equals_the_host_form(worlds):
    w = worlds[5]
    cfg = ccw.make_config("recipe")
    S = w.chainer(cfg)
    host_arrays, host_status = S.chain_tables(w.reads)
    t = S.chain_tables(w.reads, on_device=True)
    assert t.n_queries == len(w.reads)
    dev_arrays, dev_status = S.fetch_chain_tables()
    assert dev_status == host_status
    for key, v in host_arrays.items():
        assert np.array_equal(v, dev_arrays[key]), key


def test_launches_do_not_depend_on_the_batch(worlds):
    """kernel launches, device buffers and device-to-host bytes of the chain stage with MGX_CHAIN_TABLES_ON_DEVICE: the same for 24
    and for 3000 reads (fresh handles: each takes its buffers once)"""
    w = worlds[6]
    cfg = ccw.make_config("recipe")
    deltas = []
    for reads in (w.reads, w.reads * 125):
        S = w.chainer(cfg)
        before = aligner.chain_tables_kernel_launch_counts()
        S.chain_tables(reads, on_device=True)
        after = aligner.chain_tables_kernel_launch_counts()
        deltas.append(tuple(a - b for a, b in zip(after, before)))
    assert deltas[0][0] > 0 and deltas[0][1] > 0
    assert deltas[0][0] == deltas[1][0] and deltas[0][1] == deltas[1][1], deltas
    assert deltas[0][3] == deltas[1][3] == 4 * 8, deltas              # four totals travel, nothing else


def test_refusals(worlds):
    w = worlds[7]
    lib = capi.lib()
    cfg = ccw.make_config("recipe")
    out = C.c_void_p()
    # a CANONICAL graph
    W, last, F, valid = w.g.export()
    Gc = aligner.Graph(w.g.k, W, last, F, valid, mode=1)
    assert lib.mgx_seed_chainer_create(Gc.h, C.byref(cfg), None, w.A.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED
    assert b"mode" in lib.mgx_last_error()
    # an annotation without coordinates
    plain = aligner.Annotation(w.g.n_edges, [w.anno.column_words(j) for j in range(w.anno.n_labels)])
    assert lib.mgx_seed_chainer_create(w.G.h, C.byref(cfg), None, plain.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED
    assert b"coordinates" in lib.mgx_last_error()
    # one strand only
    one = ccw.make_config("recipe")
    one.forward_and_reverse_complement = 0
    assert lib.mgx_seed_chainer_create(w.G.h, C.byref(one), None, w.A.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED
    assert b"forward_and_reverse_complement" in lib.mgx_last_error()
    # chain_alignments set by the caller
    ch = ccw.make_config("recipe")
    ch.chain_alignments = 1
    assert lib.mgx_seed_chainer_create(w.G.h, C.byref(ch), None, w.A.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED
    assert b"chain_alignments" in lib.mgx_last_error()
    # the align / fetch calls on the handle
    S = w.chainer(cfg)
    S.chain_tables(w.reads[:2])
    with pytest.raises(aligner.MgxError) as e:
        S.align_batch(w.reads[:2])
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED
    with pytest.raises(aligner.MgxError) as e:
        S.fetch()
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED
    # the chain calls on an ordinary aligner
    t = capi.ChainTables()
    plain_aligner = aligner.Aligner(w.G, capi.config_cli(w.g.k))
    blob, offs = aligner.pack_queries(w.reads[:2])
    assert lib.mgx_chain_tables_batch(plain_aligner.h, blob, offs.ctypes.data, 2, 0, 0, C.byref(t)) == capi.MGX_ERR_INVALID
    assert lib.mgx_chain_tables_fetch(plain_aligner.h, C.byref(t)) == capi.MGX_ERR_INVALID
    # LabeledAligner itself with the same annotation stays refused
    assert lib.mgx_labeled_aligner_create(w.G.h, C.byref(cfg), None, w.A.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED
