"""The batched TSV formatter's logic (metagraph_amd/csrc/tsv_format.hpp: the size pass and the write pass of
mgx_format_tsv_batch) compiled for the host against the wave model (tests/emu/wave.hpp) and compared, byte for byte, with the
existing host formatter: tests/emu/tsv_format_check.cpp generates random records and streams (plain and labelled, 0 - 4
alignments per query, both orientations, negative scores, run lengths of 1 - 9 digits, more than 64 runs / labels, label numbers
below and above the name count, queries with lower case, N, bytes >= 0x80 and length 0, empty and 1 000-byte headers, one
capacity-status record), runs both passes and dumps everything; here the same records are decoded with
mgx_results_from_raw_labeled and every query is formatted with mgx_format_tsv_labeled (host code, no GPU).  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [b"strain_A", b"", b"x", b"a-rather-long-label-name/with.punctuation", b"B2", b"sample;7", b"q", b"zz"]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsv_format")
    exe = str(d / "tsv_format_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + emu, "-o", exe, os.path.join(emu, "tsv_format_check.cpp")], check=True)
    out = subprocess.run([exe, str(d / "dump")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    return str(d / "dump")


def _read(path):
    raw = open(path, "rb").read()
    hdr = np.frombuffer(raw, dtype=np.uint64, count=10)
    n, labeled, words, seq_bytes, hdr_bytes, n_names, name_bytes, text_bytes, n_cap = (int(x) for x in hdr[:9])
    min_path_score = int(hdr[9:10].view(np.int64)[0])
    at = [80]

    def take(nbytes):
        b = raw[at[0]:at[0] + nbytes]
        assert len(b) == nbytes
        at[0] += nbytes
        return b
    d = {"n": n, "labeled": labeled, "n_names": n_names, "min_path_score": min_path_score}
    d["records"] = take(64 * n)
    d["stream"] = take(4 * words)
    d["offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["seqs"] = take(seq_bytes)
    d["header_offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["headers"] = take(hdr_bytes)
    d["name_begin"] = np.frombuffer(take(4 * (n_names + 1)), dtype=np.uint32)
    d["names"] = take(name_bytes)
    d["line_begin"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["text"] = take(text_bytes)
    d["cap_list"] = np.frombuffer(take(4 * n_cap), dtype=np.uint32)
    assert at[0] == len(raw)
    return d


def _host_lines(d):
    """every query's line by the existing host code: mgx_results_from_raw_labeled + mgx_format_tsv_labeled"""
    L = capi.lib()
    n = d["n"]
    rec = np.frombuffer(d["records"], dtype=np.uint8).copy()
    stream = np.frombuffer(d["stream"], dtype=np.uint32).copy()
    store, res = C.c_void_p(), capi.Results()
    rc = L.mgx_results_from_raw_labeled(rec.ctypes.data, n, stream.ctypes.data, stream.size, d["labeled"], C.byref(store), C.byref(res))
    assert rc == 0, L.mgx_last_error()
    names = [d["names"][d["name_begin"][i]:d["name_begin"][i + 1]] for i in range(d["n_names"])]
    assert names == NAMES[:d["n_names"]]
    arr = (C.c_char_p * max(1, len(names)))(*names) if names else None
    lines = []
    try:
        for q in range(n):
            h = d["headers"][int(d["header_offsets"][q]):int(d["header_offsets"][q + 1])]
            s = d["seqs"][int(d["offsets"][q]):int(d["offsets"][q + 1])]
            need = L.mgx_format_tsv_labeled(C.byref(res), q, h, s, len(s), d["min_path_score"], arr, len(names), None, 0)
            buf = C.create_string_buffer(need + 1)
            L.mgx_format_tsv_labeled(C.byref(res), q, h, s, len(s), d["min_path_score"], arr, len(names), buf, need + 1)
            lines.append(buf.raw[:need])
    finally:
        L.mgx_raw_store_free(store)
    return lines


@pytest.mark.parametrize("variant", ["plain", "labeled", "labeled_numbers"])
def test_model_text_equals_the_host_formatter(dumps, variant):
    d = _read("%s.%s.bin" % (dumps, variant))
    lines = _host_lines(d)
    cap = sorted(int(q) for q in d["cap_list"])
    # the capacity-status record is marked for the host and takes no room in the device text
    status = np.frombuffer(d["records"], dtype=np.int32).reshape(-1, 16)[:, 0]
    assert cap == [int(q) for q in np.nonzero(status == capi.MGX_ERR_CAPACITY)[0]] and len(cap) == 1
    lb = d["line_begin"]
    assert int(lb[0]) == 0 and int(lb[-1]) == len(d["text"])
    running, spliced = 0, []
    for q in range(d["n"]):
        assert int(lb[q]) == running, "line_begin[%d]" % q
        got = d["text"][int(lb[q]):int(lb[q + 1])]
        if q in cap:
            assert got == b""
            spliced.append(lines[q])                    # (its line is the host formatter's)
        else:
            assert got == lines[q], "query %d" % q
            spliced.append(got)
            running += len(lines[q])
    assert b"".join(spliced) == b"".join(lines)
    # the batch covers what the formatter has to get right
    text = d["text"]
    assert b"\t-\t" in text and b"\t+\t" in text and (b"\t*\t*\t%d\t*\t*\t*\n" % d["min_path_score"]) in text
    assert any(l.count(b"\t+\t") + l.count(b"\t-\t") >= 2 for l in lines)
    assert b"\x7f" in text and b"\t-" in text
    if d["labeled"] and d["n_names"]:
        assert b"strain_A" in text and b";" in text
