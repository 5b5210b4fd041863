"""`.dbg` files decoded by kernels (mgx_graph_load_dbg_device, the hook mgx_boss_file_decode_device; csrc/mgx_dbgload.hip) against the
host decoder (mgx_boss_file_read / mgx_graph_load_dbg): the same tables byte for byte, the same graphs, the same refusals.  Only
well-formed files and files the HOST part refuses reach the device here; what a damaged payload does to the kernel bodies is
tested on the CPU (tests/test_dbg_decode_model.py).  Needs a real MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dbg_decode_cases as cases
import orc
import sdsl_writer as sw
from metagraph_amd import aligner, capi
from test_boss_files import GOLD, read_fasta
from test_emu_primary import primary_world
from test_gpu_parity import compare_gpu

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metagraph_amd", "_build", "mgx_align")
DNA = os.path.join(GOLD, "test_DNA_graph.dbg")
PROTEIN = os.path.join(GOLD, "test_Protein_graph.dbg")


def counts():
    out = (C.c_uint64 * 4)()
    capi.lib().mgx_dbg_decode_kernel_launch_counts(out)
    return [int(x) for x in out]


def same_table(path):
    h, d = aligner.read_boss_file(path), aligner.read_boss_file(path, on_device=True)
    for key in ("k", "sigma", "mode", "state", "n_edges", "F"):
        assert h[key] == d[key], (path, key)
    assert np.array_equal(h["W"], d["W"]), (path, "W", np.flatnonzero(h["W"] != d["W"])[:8])
    assert np.array_equal(h["last"], d["last"]), (path, "last", np.flatnonzero(h["last"] != d["last"])[:8])
    return h


def test_reference_written_files():
    assert same_table(DNA)["n_edges"] == 25
    assert same_table(PROTEIN)["sigma"] > 5               # decode only: the device index holds DNA graphs


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """one table of 10 000 - 36 000 edges in the four readable layouts, the three modes among them"""
    rng = np.random.default_rng(21)
    genome = ["".join(rng.choice(list("ACGT"), size=6000)) for _ in range(3)]
    g = orc.Graph.build(15, genome, 0, False)
    assert 10000 <= g.n_edges <= 36000
    W, last, F, _ = g.export()
    d = tmp_path_factory.mktemp("written")
    paths = {}
    for name, state, last_code, mode in [("small_rrr", sw.STATE_SMALL, sw.CODE_RRR, 0), ("small_sd", sw.STATE_SMALL, sw.CODE_SD, 1),
                                         ("stat", sw.STATE_STAT, sw.CODE_RRR, 2), ("fast", sw.STATE_FAST, sw.CODE_RRR, 0)]:
        paths[name] = d / (name + ".dbg")
        paths[name].write_bytes(sw.dbg_file(15, W, last, [int(x) for x in F], mode=mode, state=state, last_code=last_code))
    return g, paths


@pytest.mark.parametrize("name,mode", [("small_rrr", 0), ("small_sd", 1), ("stat", 2), ("fast", 0)])
def test_written_graphs(written, name, mode):
    g, paths = written
    before = counts()
    h = same_table(paths[name])
    after = counts()
    assert (h["n_edges"], h["mode"]) == (g.n_edges, mode)
    n = g.n_edges + 1
    assert (after[0] > before[0]) == name.startswith("small")                  # the rrr kernels ran where the file has rrr vectors
    assert after[1] > before[1]
    size = os.path.getsize(paths[name])
    assert 0 < after[2] - before[2] <= size + 64 * 1024                        # up: the payloads as they stand in the file (+ tables)
    assert 2 * n <= after[3] - before[3] <= 2 * n + 64                        # down: W and last in the hook, totals and the error record


def test_boundary_shapes(tmp_path):
    for i, (name, data) in enumerate(cases.boundary_cases()):
        p = tmp_path / ("%03d_%s.dbg" % (i, name))
        p.write_bytes(data)
        same_table(p)


def test_load_moves_no_table_to_the_host(written):
    g, paths = written
    for name in ("small_rrr", "small_sd", "stat", "fast"):
        before = counts()
        L = capi.lib()
        h = C.c_void_p()
        assert L.mgx_graph_load_dbg_device(str(paths[name]).encode(), 0, C.byref(h)) == 0, L.mgx_last_error()
        after = counts()
        assert L.mgx_graph_num_edges(h) == g.n_edges
        L.mgx_graph_destroy(h)
        assert after[1] > before[1]
        assert after[3] - before[3] <= 16, name                               # a scan total (sd) and the error record


def test_golden_graph_aligns_the_same():
    g = orc.Graph.build(20, read_fasta(os.path.join(GOLD, "test_DNA_sequences.fa")), 0, False)
    reads = read_fasta(os.path.join(GOLD, "test_DNA_query.fa"))
    cfg = capi.config_cli(20)
    cfg.min_exact_match = 0.0
    got = []
    for on_device in (False, True):
        G = aligner.Graph.load(DNA, on_device=on_device)
        assert (G.k, G.n_edges, G.mode) == (20, 25, 0)
        compare_gpu(g, G, cfg, reads)
        got.append(aligner.Aligner(G, cfg).align_batch(reads))
    assert got[0] == got[1]


def test_written_primary_graph_aligns_the_same(tmp_path):
    k = 15
    g, reads = primary_world(31, k, genome_len=6000, n_reads=100)
    W, last, F, _ = g.export()
    path = tmp_path / "primary.dbg"
    path.write_bytes(sw.dbg_file(k, W, last, [int(x) for x in F], mode=2, state=sw.STATE_SMALL, last_code=sw.CODE_RRR))
    cfg = capi.config_cli(k)
    cfg.min_exact_match = 0.0
    got = []
    for on_device in (False, True):
        G = aligner.Graph.load(path, on_device=on_device)
        assert (G.k, G.n_edges, G.mode) == (k, g.n_edges, 2)
        compare_gpu(g, G, cfg, reads)
        got.append(aligner.Aligner(G, cfg).align_batch(reads))
    assert got[0] == got[1]


def both_fail(path, device_call):
    """the host path's error and the device path's: the same code, the same words behind the path"""
    errs = []
    for call in (device_call.replace("_device", "") if device_call == "mgx_graph_load_dbg_device" else "mgx_boss_file_read", device_call):
        with pytest.raises(aligner.MgxError) as e:
            if call.startswith("mgx_graph_load"):
                aligner.Graph.load(path, on_device=call.endswith("_device"))
            else:
                aligner.read_boss_file(path, on_device=call.endswith("_device"))
        errs.append(e.value)
    assert errs[0].code == errs[1].code and str(errs[0]) == str(errs[1]), (str(errs[0]), str(errs[1]))
    return errs[0]


@pytest.mark.parametrize("call", ["mgx_graph_load_dbg_device", "mgx_boss_file_decode_device"])
def test_refusals_and_header_errors(tmp_path, call):
    data = open(DNA, "rb").read()
    dyn = bytearray(data)
    dyn[cases.HEADER - 1] = sw.STATE_DYN
    p = tmp_path / "dyn.dbg"
    p.write_bytes(bytes(dyn))
    e = both_fail(p, call)
    assert e.code == capi.MGX_ERR_UNSUPPORTED and "DYN" in str(e)
    if call == "mgx_graph_load_dbg_device":
        e = both_fail(PROTEIN, call)
        assert e.code == capi.MGX_ERR_UNSUPPORTED and "alphabet" in str(e)
    e = both_fail(tmp_path / "does_not_exist.dbg", call)
    assert e.code == capi.MGX_ERR_INVALID and "cannot open" in str(e)
    for cut, field in ((20, "F"), (cases.HEADER + 4, "W"), (cases.HEADER + 30, "W (rrr levels)")):
        p = tmp_path / ("cut%d.dbg" % cut)
        p.write_bytes(data[:cut])
        e = both_fail(p, call)
        assert e.code == capi.MGX_ERR_INVALID and ("inside " + field) in str(e), str(e)


def test_driver_flag_prints_the_same_bytes(tmp_path):
    reads = read_fasta(os.path.join(GOLD, "test_DNA_query.fa"))
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    out = []
    for flags in ([], ["--load-on-device"]):
        r = subprocess.run([EXE, DNA, str(fa), "--align-min-exact-match", "0.0"] + flags, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out.append(r.stdout)
    assert out[0] == out[1] and out[0].count(b"\n") == len(reads)
    r = subprocess.run([EXE, PROTEIN, str(fa), "--load-on-device"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "alphabet" in r.stderr
