"""The batched JSON formatter's logic (metagraph_amd/csrc/json_format.hpp: the one walk behind the size pass and the write pass of
mgx_format_json_batch) compiled for the host against the wave model (tests/emu/wave.hpp) and compared, byte for byte, with the
existing host formatter mgx_format_json, which the reference's own goldens pin.  tests/emu/json_format_check.cpp generates
records and streams (plain and labelled; 0 - 4 alignments per query; both orientations; negative scores; paths of 1, 2, 63, 64, 65
and more than 128 nodes; more than 64 CIGAR runs; clips at both ends; insertions in front of, inside and longer than the rest of
the first node's k characters and directly before a later node; deletions; a CIGAR that ends inside the first node; offset > 0;
circular paths; no path spelling; an unmapped read; queries with lower case, N, IUPAC letters, bytes >= 0x80, quotes, backslashes and
control bytes, in mismatch and insertion positions of both strands; a query of length 0; empty, 1 000-byte and hostile headers; node
ids of 1 and 10 digits; one capacity-status record), asserts that all of that occurs, runs both passes over the whole batch and
over three slices, checks the slices against the whole and a sentinel-filled buffer with guard regions for bytes not written or
written outside, and dumps everything; here the same records are decoded with mgx_results_from_raw_labeled and every query is
formatted with mgx_format_json (host code, no GPU).  The identity text ("%.17g" in integer arithmetic) has a run of its own against
snprintf.  A second build of the check program with -fsanitize=address,undefined runs as the stand-alone binary it is.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
VARIANTS = ["plain", "labeled", "small_k"]


def _compile(exe, extra):
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + EMU] + extra + ["-o", exe, os.path.join(EMU, "json_format_check.cpp")], check=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("json_format")
    path = str(d / "json_format_check")
    _compile(path, [])
    return path


@pytest.fixture(scope="module")
def dumps(exe):
    prefix = os.path.join(os.path.dirname(exe), "dump")
    out = subprocess.run([exe, prefix], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    return prefix


def _read(path):
    raw = open(path, "rb").read()
    n, labeled, words, seq_bytes, hdr_bytes, k, text_bytes, n_cap = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=8))
    at = [64]

    def take(nbytes):
        b = raw[at[0]:at[0] + nbytes]
        assert len(b) == nbytes
        at[0] += nbytes
        return b
    d = {"n": n, "labeled": labeled, "k": k}
    d["records"] = take(64 * n)
    d["stream"] = take(4 * words)
    d["offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["seqs"] = take(seq_bytes)
    d["header_offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["headers"] = take(hdr_bytes)
    d["line_begin"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["text"] = take(text_bytes)
    d["cap_list"] = np.frombuffer(take(4 * n_cap), dtype=np.uint32)
    assert at[0] == len(raw)
    return d


def _host_lines(d):
    """every query's lines by the existing host code: mgx_results_from_raw_labeled + mgx_format_json"""
    L = capi.lib()
    n = d["n"]
    rec = np.frombuffer(d["records"], dtype=np.uint8).copy()
    stream = np.frombuffer(d["stream"], dtype=np.uint32).copy()
    store, res = C.c_void_p(), capi.Results()
    rc = L.mgx_results_from_raw_labeled(rec.ctypes.data, n, stream.ctypes.data, stream.size, d["labeled"], C.byref(store), C.byref(res))
    assert rc == 0, L.mgx_last_error()
    lines = []
    try:
        for q in range(n):
            h = d["headers"][int(d["header_offsets"][q]):int(d["header_offsets"][q + 1])]
            s = d["seqs"][int(d["offsets"][q]):int(d["offsets"][q + 1])]
            assert b"\0" not in h
            lines.append(capi.format_json(res, q, h, s, d["k"]).encode("latin-1"))
    finally:
        L.mgx_raw_store_free(store)
    return lines


@pytest.mark.parametrize("variant", VARIANTS)
def test_model_text_equals_the_host_formatter(dumps, variant):
    d = _read("%s.%s.bin" % (dumps, variant))
    lines = _host_lines(d)
    cap = sorted(int(q) for q in d["cap_list"])
    status = np.frombuffer(d["records"], dtype=np.int32).reshape(-1, 16)[:, 0]
    assert cap == [int(q) for q in np.nonzero(status == capi.MGX_ERR_CAPACITY)[0]] and len(cap) == 1
    lb = d["line_begin"]
    assert int(lb[0]) == 0 and int(lb[-1]) == len(d["text"])
    running = 0
    for q in range(d["n"]):
        assert int(lb[q]) == running, "line_begin[%d]" % q
        got = d["text"][int(lb[q]):int(lb[q + 1])]
        if q in cap:
            assert got == b""                               # (its lines are the host formatter's)
        else:
            assert got == lines[q], "query %d" % q
            running += len(lines[q])
    # what the check program says it generated shows in the text
    text = d["text"]
    for piece in (b'"is_secondary":true', b'"read_on_reverse_strand":true', b'"is_circular":true', b'"read_mapped":false', b'"soft_clipped":true',
                  b'"query_position":', b',"offset":', b'{"name":"', b'"sequence":""}\n', b"\\u007F", b"\\u0001", b'\\"', b"\\\\", b"\\t",
                  b'"score":-', b'"identity":0.0', b'"identity":1.0', b'"length":1,', b'"length":2,', b'"length":63,', b'"length":64,',
                  b'"length":65,', b'"length":130,', b'"length":200,', b'{"from_length":1}', b'"name":"",', b"\\u00E9"):
        assert piece in text, piece


def test_identity_text_equals_snprintf(exe):
    out = subprocess.run([exe, "identity"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok identity"), out.stdout + out.stderr


def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """the same program, instrumented, run as the stand-alone binary it is (nothing preloaded): generation, both passes, the slices"""
    path = str(tmp_path / "json_format_check_san")
    _compile(path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([path, str(tmp_path / "dump")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr[-4000:]
