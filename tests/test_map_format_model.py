"""The batched `align --map` formatter's logic (metagraph_amd/csrc/map_format.hpp: the size pass and the write pass of
mgx_format_map_batch) compiled for the host against the wave model (tests/emu/wave.hpp) and compared, byte for byte, with the
per-query host formatter: tests/emu/map_format_check.cpp builds count records (up to 2^32 - 1), node arrays (0, 9 / 10, 99 / 100,
... 10^19, 2^64 - 1), reads with 0, 1, 63, 64, 65, 256, 257 and about 5000 windows of 3, 11, 21 and 31 characters (lower case, N,
bytes >= 0x80; some with more node slots than windows fit), headers of 0 .. 7 and of 1000 bytes, an empty batch and a
FILTER_PRESENT batch with nothing present, runs both passes for all four formats and dumps everything; here every query of the
same data is formatted with mgx_format_map.  Presence: every (n_discovered, n_kmers) up to 40 and the boundary set of
test_map_format.py up to 300, seven fractions, both formulas and the query_len < k case, against mgx_map_present.  CPU only."""
import ctypes as C
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

from metagraph_amd import capi
from test_map_format import FRACTIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {"nodes": capi.MGX_MAP_FMT_NODES, "count": capi.MGX_MAP_FMT_COUNT_KMERS, "presence": capi.MGX_MAP_FMT_QUERY_PRESENCE,
           "filter": capi.MGX_MAP_FMT_FILTER_PRESENT}
SHAPES = ["k31_l0", "k31_l21", "k31_l11", "k31_l3", "k11_l11", "k21_l0"]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_format")
    exe = str(d / "map_format_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + emu, "-o", exe, os.path.join(emu, "map_format_check.cpp")], check=True)
    out = subprocess.run([exe, str(d / "dump")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert len(glob.glob(str(d / "dump.*.bin"))) == int(out.stdout.split()[1]) == 4 * len(SHAPES) + 4 + 1 + 2 * len(FRACTIONS)
    return str(d / "dump")


def _read(path):
    raw = open(path, "rb").read()
    n, fmt, k, map_length, n_nodes, seq_bytes, hdr_bytes, text_bytes, fbits = struct.unpack_from("<9Q", raw)
    at = [96]

    def take(nbytes):
        b = raw[at[0]:at[0] + nbytes]
        assert len(b) == nbytes
        at[0] += nbytes
        return b
    d = {"n": n, "format": fmt, "k": k, "map_length": map_length, "fraction": struct.unpack("<d", struct.pack("<Q", fbits))[0]}
    d["counts"] = np.frombuffer(take(12 * n), dtype=np.uint32).reshape(-1, 3)
    d["node_begin"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["nodes"] = np.frombuffer(take(8 * n_nodes), dtype=np.uint64)
    d["offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["seqs"] = take(seq_bytes)
    d["header_offsets"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["headers"] = take(hdr_bytes)
    d["line_begin"] = np.frombuffer(take(8 * (n + 1)), dtype=np.uint64)
    d["text"] = take(text_bytes)
    assert at[0] == len(raw)
    return d


def _host_texts(d):
    """every query's text by the per-query host code: mgx_format_map on a view of the dumped arrays"""
    L = capi.lib()
    n = d["n"]
    counts = np.ascontiguousarray(d["counts"]).copy()
    nb = d["node_begin"].copy()
    nodes = np.concatenate([d["nodes"], np.zeros(1, dtype=np.uint64)])
    m = capi.MapSummary()
    m.n_queries = n
    m.counts = C.cast(counts.ctypes.data, C.POINTER(capi.MapCounts))
    m.node_begin = C.cast(nb.ctypes.data, C.POINTER(C.c_uint64))
    m.nodes = C.cast(nodes.ctypes.data, C.POINTER(C.c_uint64))
    out = []
    for q in range(n):
        h = d["headers"][int(d["header_offsets"][q]):int(d["header_offsets"][q + 1])]
        s = d["seqs"][int(d["offsets"][q]):int(d["offsets"][q + 1])]
        args = (C.byref(m), q, h, s, len(s), d["k"], d["map_length"], d["format"], d["fraction"])
        need = L.mgx_format_map(*args, None, 0)
        buf = C.create_string_buffer(need + 1)
        L.mgx_format_map(*args, buf, need + 1)
        out.append(buf.raw[:need])
    return out


def _check_against_host(d):
    want = _host_texts(d)
    lb = d["line_begin"]
    assert int(lb[0]) == 0 and int(lb[-1]) == len(d["text"])
    running = 0
    for q in range(d["n"]):
        assert int(lb[q]) == running, "line_begin[%d]" % q
        assert d["text"][int(lb[q]):int(lb[q + 1])] == want[q], "query %d" % q
        running += len(want[q])
    assert d["text"] == b"".join(want)
    return want


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("shape", SHAPES)
def test_model_text_equals_the_host_formatter(dumps, shape, fmt):
    d = _read("%s.%s.%s.bin" % (dumps, shape, fmt))
    assert d["format"] == FORMATS[fmt] and d["n"] > 200
    want = _check_against_host(d)
    text = d["text"]
    window = d["map_length"] if 0 < d["map_length"] < d["k"] else d["k"]
    if fmt == "nodes":
        # the batch covers what the formatter has to get right: every digit count, the extremes, unnormalised bytes, the guard
        widths = {len(l.rsplit(b": ", 1)[1]) for l in text.split(b"\n")[:-1]}
        assert widths == set(range(1, 21))
        assert b": 0\n" in text and b": 18446744073709551615\n" in text and b": 10000000000000000000\n" in text
        assert b"\x80" in text and b"\xff" in text and b"a" in text and b"N" in text
        per_query = [w.count(b"\n") for w in want]
        assert {0, 1, 63, 64, 65, 256, 257, 5003} <= set(per_query)
        fit = [max(0, int(d["offsets"][q + 1] - d["offsets"][q]) - window + 1) for q in range(d["n"])]
        declared = [int(d["node_begin"][q + 1] - d["node_begin"][q]) for q in range(d["n"])]
        assert per_query == [min(a, b) for a, b in zip(fit, declared)] and any(a < b for a, b in zip(fit, declared))
    elif fmt == "count":
        assert b"\t4294967295/" in text and b"/4294967295\n" in text and b"\t0/" in text
        hl = {int(d["header_offsets"][q + 1] - d["header_offsets"][q]) for q in range(d["n"])}
        assert hl == set(range(8)) | {1000}
    elif fmt == "presence":
        assert len(text) == 2 * d["n"] and b"0\n" in text and b"1\n" in text
    else:
        assert any(w == b"" for w in want) and any(w.startswith(b">") for w in want)
        assert b"\x80" in text and b"a" in text          # the query as it came


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_model_empty_batch(dumps, fmt):
    d = _read("%s.empty.%s.bin" % (dumps, fmt))
    assert d["n"] == 0 and d["text"] == b"" and [int(x) for x in d["line_begin"]] == [0]


def test_model_filter_with_nothing_present(dumps):
    d = _read("%s.nothing.filter.bin" % dumps)
    assert d["n"] > 200 and d["text"] == b"" and not d["line_begin"].any()
    assert all(w == b"" for w in _check_against_host(d))


@pytest.mark.parametrize("map_length", [0, 7])
@pytest.mark.parametrize("fi", range(len(FRACTIONS)))
def test_model_presence_equals_mgx_map_present(dumps, fi, map_length):
    d = _read("%s.present_f%d_l%d.presence.bin" % (dumps, fi, map_length))
    f = FRACTIONS[fi]
    assert d["fraction"] == f and d["k"] == 11 and d["map_length"] == map_length
    L = capi.lib()
    want = bytearray()
    pairs = set()
    for q in range(d["n"]):
        c = capi.MapCounts(*[int(x) for x in d["counts"][q]])
        qlen = int(d["offsets"][q + 1] - d["offsets"][q])
        want += b"1\n" if L.mgx_map_present(C.byref(c), qlen, d["k"], map_length, f) else b"0\n"
        pairs.add((c.n_discovered, c.n_kmers))
    assert d["text"] == bytes(want)
    assert all((nd, nk) in pairs for nk in range(41) for nd in range(nk + 1)) and (150, 300) in pairs and (210, 300) in pairs
    # the queries shorter than k that carry counts: absent under the full-k formula whatever the counts say
    if map_length == 0:
        assert d["text"].endswith(b"0\n0\n0\n")
