"""The on-device result decode's logic (metagraph_amd/csrc/results_decode.hpp: the size pass and the write pass behind
mgx_decode_results_device and the option decode_on_device) compiled for the host against the wave model (tests/emu/wave.hpp) and
compared, byte for byte, with the existing host decode: tests/emu/results_decode_check.cpp generates random records and streams
(plain and labeled), runs the size pass, a plain exclusive sum and the write pass and dumps the inputs and the seven arrays; here
the same records are decoded with mgx_results_from_raw_labeled (host code, no GPU).  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("results_decode")
    exe = str(d / "results_decode_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + emu, "-o", exe, os.path.join(emu, "results_decode_check.cpp")], check=True)
    out = subprocess.run([exe, str(d / "dump")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    return str(d / "dump")


def _read(path):
    raw = open(path, "rb").read()
    hdr = [int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=8)]
    n, labeled, words = hdr[:3]
    totals = hdr[3:8]
    at = [64]

    def take(nbytes):
        b = raw[at[0]:at[0] + nbytes]
        assert len(b) == nbytes
        at[0] += nbytes
        return b
    d = {"n": n, "labeled": labeled, "totals": totals}
    d["records"] = take(64 * n)
    d["stream"] = take(4 * words)
    d["aln_begin"] = take(8 * (n + 1))
    d["status"] = take(4 * n)
    d["alns"] = take(72 * totals[0])
    d["nodes"] = take(8 * totals[1])
    d["cigar"] = take(8 * totals[2])
    d["seqs"] = take(totals[3])
    d["labels"] = take(4 * totals[4])
    assert at[0] == len(raw)
    return d


def _host_decode(d):
    """the seven arrays as raw bytes, and numpy views for the coverage checks, by mgx_results_from_raw_labeled"""
    L = capi.lib()
    n = d["n"]
    rec = np.frombuffer(d["records"], dtype=np.uint8).copy()
    stream = np.frombuffer(d["stream"], dtype=np.uint32).copy()
    store, res = C.c_void_p(), capi.Results()
    rc = L.mgx_results_from_raw_labeled(rec.ctypes.data, n, stream.ctypes.data, stream.size, d["labeled"], C.byref(store), C.byref(res))
    assert rc == 0, L.mgx_last_error()
    try:
        a = capi.results_arrays(res)
        alns = a["alns"].copy()
        nl = int(alns["n_labels"].sum()) if len(alns) else 0
        assert bool(res.labels) == (nl > 0)
        labels = np.ctypeslib.as_array(res.labels, shape=(nl,)).copy() if nl else np.zeros(0, dtype=np.uint32)
        return {"aln_begin": a["aln_begin"].tobytes(), "status": a["status"].tobytes(), "alns": alns.tobytes(), "nodes": a["nodes"].tobytes(),
                "cigar": a["cigar"].tobytes(), "seqs": a["seqs"].tobytes(), "labels": labels.tobytes(),
                "np_alns": alns, "np_cigar": a["cigar"].copy(), "np_begin": a["aln_begin"].copy(), "np_status": a["status"].copy()}
    finally:
        L.mgx_raw_store_free(store)


@pytest.mark.parametrize("variant", ["plain", "labeled"])
def test_model_arrays_equal_the_host_decode(dumps, variant):
    d = _read("%s.%s.bin" % (dumps, variant))
    h = _host_decode(d)
    for name in ("aln_begin", "status", "alns", "nodes", "cigar", "seqs", "labels"):
        assert d[name] == h[name], name
    assert d["totals"] == [len(h["alns"]) // 72, len(h["nodes"]) // 8, len(h["cigar"]) // 8, len(h["seqs"]), len(h["labels"]) // 4]

    # the batch covers what the decode has to get right
    alns, cigar, begin, status = h["np_alns"], h["np_cigar"], h["np_begin"], h["np_status"]
    per_query = np.diff(begin.astype(np.int64))
    rec = np.frombuffer(d["records"], dtype=np.int32).reshape(-1, 16)
    cap = rec[:, 0] == capi.MGX_ERR_CAPACITY
    assert cap.any() and (status[cap] == capi.MGX_ERR_CAPACITY).all() and (per_query[cap] == 0).all()      # a capacity-status record ...
    assert (rec[cap, 1] > 0).any()                                                                        # ... whose alignments are not read
    assert ((rec[:, 0] == 0) & (rec[:, 1] == 0)).any()                                                    # an OK record without alignments
    assert {2, 3, 4} <= set(int(x) for x in per_query)
    assert (alns["n_nodes"] > 64).any() and (alns["n_cigar"] > 64).any()                                  # the chunk loops
    assert {0, 1, 2, 3} <= set(int(x) for x in alns["seq_len"]) and (alns["seq_len"] % 4 != 0).any()
    assert {0, 1, 2, 3} == set(int(x) for x in alns["seq_begin"] % 4)
    assert set(int(x) for x in cigar["op"]) == {0, 1, 2, 3, 4, 5}
    with_runs = alns[alns["n_cigar"] > 0]
    assert (with_runs["clipping"] > 0).any() and (with_runs["end_clipping"] > 0).any()
    assert ((with_runs["clipping"] == 0) & (with_runs["end_clipping"] == 0)).any()
    assert ((with_runs["clipping"] > 0) & (with_runs["end_clipping"] > 0)).any()
    assert int(cigar["len"].max()) == 2**29 - 1
    assert (alns["score"] < 0).any()
    assert set(int(x) for x in alns["orientation"]) == {0, 1}
    assert not alns["_pad"].any() and not cigar["_pad"].any()
    if d["labeled"]:
        assert (alns["n_labels"] > 64).any() and (alns["n_labels"] == 0).any()                            # a labeled alignment with no label
        # labels_begin is the running label count, also where an alignment has no label
        assert np.array_equal(alns["labels_begin"], np.concatenate([[0], np.cumsum(alns["n_labels"].astype(np.uint64))[:-1]]).astype(np.uint64))
    else:
        assert not alns["n_labels"].any() and not alns["labels_begin"].any() and d["labels"] == b""
