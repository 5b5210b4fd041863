"""The structured results of a batch decoded by HIP kernels (csrc/results_decode.hpp, csrc/mgx_decode.hip) against the host
decode: mgx_fetch_results with the pipeline option decode_on_device=1 must return, array by array and byte by byte, what it
returns with the option off (capacity retries and post-chaining included), and mgx_decode_results_device must leave in device
memory what mgx_results_from_raw_labeled makes of the records and the stream of mgx_device_results.  The worlds are those of the
formatter and chain tests.  Needs a real MI355X."""
import ctypes as C
import functools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import orc
from metagraph_amd import aligner, capi
from test_emu_vs_oracle import make_world, rand_seq, KATS
from test_oracle_canonical import CANONICAL
from test_oracle_primary_goldens import PRIMARY
from test_gpu_format_batch import format_world, gpu_graph, align_host, _bytes, BASIC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ARRAYS = ("aln_begin", "status", "alns", "nodes", "cigar", "seqs", "labels")
ALN_DT = np.dtype([("score", "<i4"), ("offset", "<u4"), ("clipping", "<u4"), ("end_clipping", "<u4"), ("num_matches", "<u4"),
                   ("n_nodes", "<u4"), ("n_cigar", "<u4"), ("seq_len", "<u4"), ("nodes_begin", "<u8"), ("cigar_begin", "<u8"),
                   ("seq_begin", "<u8"), ("orientation", "u1"), ("_pad", "u1", (3,)), ("n_labels", "<u4"), ("labels_begin", "<u8")])
assert ALN_DT.itemsize == 72


def _addr(ptr):
    return C.cast(ptr, C.c_void_p).value


def snapshot(res):
    """numpy copies of the seven arrays of a Results view in host memory (alignment records and CIGAR runs as raw bytes, padding
    included; labels: None for a NULL pointer)"""
    a = capi.results_arrays(res)
    alns = a["alns"]
    s = {"aln_begin": a["aln_begin"].copy(), "status": a["status"].copy(), "alns": np.frombuffer(alns.tobytes(), dtype=np.uint8),
         "nodes": a["nodes"].copy(), "cigar": np.frombuffer(a["cigar"].tobytes(), dtype=np.uint8), "seqs": a["seqs"].copy(), "labels": None}
    if res.labels:
        nl = int(alns["n_labels"].sum()) if len(alns) else 0
        s["labels"] = np.ctypeslib.as_array(res.labels, shape=(nl,)).copy()
    return s


def assert_same(a, b):
    for name in ARRAYS:
        if a[name] is None or b[name] is None:
            assert a[name] is None and b[name] is None, "labels: one view has none"
        else:
            assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name


def records_of(s):
    return np.frombuffer(s["alns"].tobytes(), dtype=ALN_DT)


def fetch_off_then_on(A):
    """the staged batch fetched with the host decode, then again with the kernels: both snapshots, which must be equal"""
    A.set_pipeline("decode_on_device=0")
    off = snapshot(A.fetch())
    before = aligner.decode_kernel_launch_counts()
    A.set_pipeline("decode_on_device=1")
    on = snapshot(A.fetch())
    after = aligner.decode_kernel_launch_counts()
    A.set_pipeline("decode_on_device=0")
    # the kernels served it (and the fetches of the capacity retry's own aligner, which inherits the option, where there is one)
    assert after[3] > before[3] and after[0] > before[0] and after[1] > before[1]
    assert_same(off, on)
    return off, on


_hip = None


def d2h(ptr, dtype, count):
    """count elements of dtype from device memory (hipMemcpy through ctypes)"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    out = np.zeros(count, dtype=dtype)
    if count:
        assert ptr, "a NULL device pointer for %d elements" % count
        rc = _hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2)
        assert rc == 0, "hipMemcpy: %d" % rc
    return out


def device_snapshot(A):
    """mgx_decode_results_device -> (snapshot of the device arrays copied back by the reported sizes, sizes)"""
    res, sizes = A.decode_device()
    n = int(res.n_queries)
    s = {"aln_begin": d2h(_addr(res.aln_begin), np.uint64, n + 1), "status": d2h(_addr(res.status), np.int32, n),
         "alns": d2h(_addr(res.alignments), np.uint8, 72 * sizes["n_alignments"]), "nodes": d2h(_addr(res.nodes), np.uint64, sizes["n_nodes"]),
         "cigar": d2h(_addr(res.cigar), np.uint8, 8 * sizes["n_cigar"]), "seqs": d2h(_addr(res.seqs), np.uint8, sizes["n_seq_bytes"]),
         "labels": d2h(_addr(res.labels), np.uint32, sizes["n_labels"]) if res.labels else None}
    assert bool(res.labels) == (sizes["n_labels"] > 0)
    return s, sizes


def raw_snapshot(A, labeled=False):
    """the yardstick of the device form: records and stream of mgx_device_results copied back and decoded by the host"""
    L = capi.lib()
    headers, stream = C.c_void_p(), C.c_void_p()
    hb, n, words = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.mgx_device_results(A.h, C.byref(headers), C.byref(hb), C.byref(n), C.byref(stream), C.byref(words)) == 0
    assert hb.value == 64
    rec = d2h(headers.value, np.uint8, 64 * n.value)
    st = d2h(stream.value, np.uint32, words.value)
    store, res = C.c_void_p(), capi.Results()
    rc = L.mgx_results_from_raw_labeled(rec.ctypes.data, n.value, st.ctypes.data if st.size else None, st.size, int(labeled), C.byref(store), C.byref(res))
    assert rc == 0, L.mgx_last_error()
    try:
        return snapshot(res)
    finally:
        L.mgx_raw_store_free(store)


def align_on_device(A, reads):
    """the reads uploaded by the caller -> the tensors (to be kept alive until the last fetch)"""
    import torch
    blob, offs = aligner.pack_queries(reads)
    d_seqs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    A.align_device(d_seqs.data_ptr(), d_offs.data_ptr(), len(reads))
    return d_seqs, d_offs


# ---- 1. the reference's CLI goldens and the random worlds ------------------------------------------------------------------------
def test_cli_goldens():
    from test_oracle_kats import read_fasta, read_fastq
    cli = KATS["cli"]
    g = orc.Graph.build(cli["k"], read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])), 0, False)
    G = gpu_graph(g)
    reads = [r[1] for r in read_fastq(os.path.join(HERE, "golden", cli["reads_fastq"]))]
    for spec in cli["runs"]:
        cfg = capi.config_cli(cli["k"])
        for key, val in spec["flags"].items():
            setattr(cfg, key, val)
        A = aligner.Aligner(G, cfg)
        align_host(A, reads)
        off, _ = fetch_off_then_on(A)
        assert len(off["alns"]) > 0
        dev, _ = device_snapshot(A)
        assert_same(dev, raw_snapshot(A))


@functools.lru_cache(maxsize=None)
def _world(mode):
    g, reads = format_world(mode)
    return g, tuple(reads)


def _random_world(mode, num_alt, on_device):
    g, reads = _world(mode)
    reads = list(reads)
    cfg = capi.config_cli(21)
    cfg.num_alternative_paths = num_alt
    A = aligner.Aligner(gpu_graph(g, {"basic": BASIC, "canonical": CANONICAL, "primary": PRIMARY}[mode]), cfg)
    keep = align_on_device(A, reads) if on_device else align_host(A, reads)
    off, _ = fetch_off_then_on(A)
    per_query = np.diff(off["aln_begin"].astype(np.int64))
    rec = records_of(off)
    assert (per_query == 0).any() and (per_query > 0).any() and off["labels"] is None
    if num_alt > 1:
        assert (per_query >= 2).any()
    if mode == "basic":
        assert set(int(x) for x in rec["orientation"]) == {0, 1}
    del keep


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reads", "device_reads"])
@pytest.mark.parametrize("num_alt", [1, 4])
def test_random_world_basic(num_alt, on_device, kernels):
    _random_world("basic", num_alt, on_device)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reads", "device_reads"])
@pytest.mark.parametrize("num_alt", [1, 4])
@pytest.mark.parametrize("mode", ["canonical", "primary"])
def test_random_worlds(mode, num_alt, on_device):
    _random_world(mode, num_alt, on_device)


# ---- 2. edge queries (the read list of test_edge_queries_and_headers) -----------------------------------------------------------
def test_edge_queries():
    k = 21
    g, reads = make_world(9200, k, genome_len=4000, n_reads=30, read_len=150)
    edge = [reads[0].lower(), reads[1][:60].lower() + reads[1][60:], reads[2][:40] + "N" * 30 + reads[2][70:], "N" * 90, "n" * 25,
            _bytes(reads[3][:70]) + b"\x80\xff\xc3\xa9" + _bytes(reads[3][74:]), b"\x80" * 40, b"\xfe", "", reads[4][:k - 1], reads[5][:3],
            "acgtnACGTN" * 9, reads[6][:k], "R" + reads[7][1:], reads[8].lower()[:80] + "~{|}" + reads[8][84:]]
    reads = [_bytes(r) for r in edge + reads[9:]]
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, reads)
    off, _ = fetch_off_then_on(A)
    per_query = np.diff(off["aln_begin"].astype(np.int64))
    assert per_query[0] > 0 and per_query[8] == 0 and per_query[10] == 0          # lower case aligns; the empty read and three characters do not
    dev, _ = device_snapshot(A)
    assert_same(dev, raw_snapshot(A))


# ---- 3. label-aware ------------------------------------------------------------------------------------------------------------
def test_labeled():
    from labeled_worlds import labeled_world
    g, anno, reads = labeled_world(21, 15, n_strains=3, n_reads=40)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(15),
                        annotation=aligner.Annotation(g.n_edges, [anno.column_words(j) for j in range(anno.n_labels)]))
    align_host(A, reads)
    off, on = fetch_off_then_on(A)
    assert on["labels"] is not None and len(on["labels"]) > 0
    rec = records_of(on)
    assert (rec["n_labels"] >= 2).any()
    assert np.array_equal(rec["labels_begin"], np.concatenate([[0], np.cumsum(rec["n_labels"].astype(np.uint64))[:-1]]).astype(np.uint64))
    dev, sizes = device_snapshot(A)
    assert_same(dev, raw_snapshot(A, labeled=True))
    assert sizes["n_labels"] == len(on["labels"])


# ---- 4. long paths: the chunk loops of the write pass ---------------------------------------------------------------------------
def test_long_paths():
    g, reads = make_world(9500, 21, genome_len=5000, n_reads=24, read_len=600)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, reads)
    off, _ = fetch_off_then_on(A)
    rec = records_of(off)
    assert (rec["n_nodes"] > 256).any() and int(rec["n_nodes"].max()) > 500


# ---- 5. capacity statuses: retried behind either decode, handed out by the device form --------------------------------------------
def test_capacity_statuses():
    g, reads = make_world(4242, 21, genome_len=6000, n_reads=200, read_len=150)
    lim = capi.Limits()
    lim.cell_arena_bytes = 1600
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21), lim)
    align_host(A, reads)
    off, on = fetch_off_then_on(A)
    assert not on["status"].any()
    assert A.stats()["n_capacity_retried"] > 0
    # the device form is pre-retry: those queries have their status and no alignments
    dev, _ = device_snapshot(A)
    cap = dev["status"] == capi.MGX_ERR_CAPACITY
    assert int(cap.sum()) >= A.stats()["n_capacity_retried"] > 0 and not dev["status"][~cap].any()
    assert not np.diff(dev["aln_begin"].astype(np.int64))[cap].any()
    assert_same(dev, raw_snapshot(A))


# ---- 6. post-chaining (the seed-900 world of test_chaining_stitched_reads_on_gpu) ----------------------------------------------
def test_post_chaining():
    from test_emu_vs_oracle import mutate, rc
    from test_oracle_chain import chain_config
    rng = random.Random(900)
    k = rng.choice([12, 15, 21])
    genome = rand_seq(rng, 6000)
    g = orc.Graph.build(k, [genome], 0, False)
    cfg = chain_config(k, (2, -3, -3), None)
    cfg.min_seed_length = 10
    queries = []
    for _ in range(300):
        a, b = rng.randrange(0, 5800), rng.randrange(0, 5800)
        la, lb = rng.randrange(25, 90), rng.randrange(25, 90)
        q = genome[a:a + la] + rand_seq(rng, rng.choice([0, 0, 1, 3, 8])) + genome[b:b + lb]
        if rng.random() < 0.5:
            q = mutate(rng, q)
        if rng.random() < 0.4:
            q = rc(q)
        queries.append(q)
    assert cfg.post_chain_alignments
    A = aligner.Aligner(gpu_graph(g), cfg)
    align_host(A, queries)
    off, on = fetch_off_then_on(A)
    assert (on["nodes"] == 0).any()                                   # a chain: node 0 where the path has no graph node
    # the device form holds the unchained alignments
    dev, _ = device_snapshot(A)
    assert_same(dev, raw_snapshot(A))
    assert not (dev["nodes"] == 0).any()


# ---- 7., 8. what runs and what travels -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _traffic_world():
    g, reads = make_world(9400, 21, genome_len=5000, n_reads=300, read_len=150)
    return g, tuple(reads)


def test_device_form_kernels_and_traffic():
    g, reads = _traffic_world()
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, list(reads))
    before = aligner.decode_kernel_launch_counts()
    res, sizes = A.decode_device()
    after = aligner.decode_kernel_launch_counts()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[3] == before[3]
    assert after[2] - before[2] == 40                                  # the five totals
    dev, sizes2 = device_snapshot(A)
    assert sizes == sizes2 and sizes["n_alignments"] > 50 and sizes["n_labels"] == 0, sizes
    assert_same(dev, raw_snapshot(A))


def test_host_form_traffic():
    g, reads = _traffic_world()
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, list(reads))
    A.set_pipeline("decode_on_device=1")
    before = aligner.decode_kernel_launch_counts()
    on = snapshot(A.fetch())
    after = aligner.decode_kernel_launch_counts()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[3] == before[3] + 1
    n = len(reads)
    assert on["labels"] is None and not on["status"].any()
    want = 40 + 8 * (n + 1) + on["alns"].nbytes + on["nodes"].nbytes + on["cigar"].nbytes + on["seqs"].nbytes + 4 * n
    assert after[2] - before[2] == want
    assert len(on["alns"]) == 72 * int(on["aln_begin"][-1]) and int(on["aln_begin"][-1]) > 50
    # mgx_fetch_seed_info after such a fetch reads the records itself
    info = A.seed_info(n)
    assert len(info) == n and any(i["num_matches"][0] or i["num_matches"][1] for i in info)
    A.set_pipeline("decode_on_device=0")
    assert_same(snapshot(A.fetch()), on)
    assert A.seed_info(n) == info


# ---- 9. no alignments at all -----------------------------------------------------------------------------------------------------
def test_no_alignments_and_no_queries():
    g, _ = make_world(9600, 21, genome_len=3000, n_reads=2, read_len=100)
    rng = random.Random(9601)
    reads = [rand_seq(rng, 120) for _ in range(70)]
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, reads)
    off, on = fetch_off_then_on(A)
    dev, sizes = device_snapshot(A)
    for s in (on, dev):
        assert s["labels"] is None and len(s["status"]) == 70 and not s["status"].any()
        assert len(s["aln_begin"]) == 71 and not s["aln_begin"].any()
        assert len(s["alns"]) == len(s["nodes"]) == len(s["cigar"]) == len(s["seqs"]) == 0
    assert not any(sizes.values())
    # a batch without queries
    align_host(A, [])
    res, sizes = A.decode_device()
    assert res.n_queries == 0 and not any(sizes.values()) and not res.labels
    assert int(d2h(_addr(res.aln_begin), np.uint64, 1)[0]) == 0
    A.set_pipeline("decode_on_device=1")
    assert A.fetch().n_queries == 0


# ---- 10. the staging rule --------------------------------------------------------------------------------------------------------
def test_staging_rule():
    g, reads = make_world(9700, 21, genome_len=3000, n_reads=20, read_len=100)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    with pytest.raises(aligner.MgxError) as e:
        A.decode_device()                                              # before any batch
    assert e.value.code == capi.MGX_ERR_INVALID
    align_host(A, reads)
    A.decode_device()
    A.map_batch(reads[:5])
    with pytest.raises(aligner.MgxError) as e:
        A.decode_device()                                              # the aligned batch is no longer the staged one
    assert e.value.code == capi.MGX_ERR_INVALID and "staged" in str(e.value)
    # The option is ignored then: the fetch is the host decode's, as it always was.  (Staging clears the stream's cursor, so such a
    # fetch is defined only for a batch none of whose records has an alignment: reads from nowhere, the same number mapped.)
    rng = random.Random(9701)
    nowhere = [rand_seq(rng, 110) for _ in range(30)]
    B = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(B, nowhere)
    assert not np.diff(snapshot(B.fetch())["aln_begin"].astype(np.int64)).any()
    B.map_batch(nowhere)
    B.set_pipeline("decode_on_device=0")
    off = snapshot(B.fetch())
    before = aligner.decode_kernel_launch_counts()
    B.set_pipeline("decode_on_device=1")
    on = snapshot(B.fetch())
    assert aligner.decode_kernel_launch_counts() == before
    assert_same(off, on)
    assert len(on["status"]) == 30 and len(on["aln_begin"]) == 31


# ---- 11. the driver --------------------------------------------------------------------------------------------------------------
def test_driver_kernel_option(tmp_path):
    from test_oracle_kats import read_fasta
    cli = KATS["cli"]
    g = orc.Graph.build(cli["k"], read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])), 0, False)
    W, last, F, _ = g.export()
    dump = tmp_path / "mt.boss"
    with open(dump, "wb") as f:
        f.write(struct.pack("<7Q", g.k, g.n_edges, *[int(x) for x in F]))
        f.write(W.tobytes())
        f.write(last.tobytes())
    exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
    reads = os.path.join(HERE, "golden", cli["reads_fastq"])
    for extra in ([], ["--json"]):
        base = [exe, str(dump), reads, "--align-min-exact-match", "0.0"] + extra
        ref = subprocess.run(base, capture_output=True, timeout=120)
        assert ref.returncode == 0, ref.stderr
        r = subprocess.run(base + ["--kernel-option", "decode_on_device=1"], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == ref.stdout and len(r.stdout) > 0
