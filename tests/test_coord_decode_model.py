"""The kernel bodies behind mgx_annotation_load_coord_columns_device and mgx_annotation_set_coordinates_device
(metagraph_amd/csrc/coord_decode.hpp over the plans and batch layouts of col_plan.hpp / coord_plan.hpp) compiled for the host and
run by tests/emu/coord_decode_check.cpp, a stand-alone program built with -fsanitize=address,undefined in which every array has
exactly the size the driver gives its device buffer.  It decodes the files of tests/coord_decode_cases.py, transposes the result
(comparing with the tables mgx_annotation_set_coordinates builds) and dumps the tables; here the dumps are compared with the host
reader (mgx_column_coord_file_read).  Damaged files: whatever the host reader answers the model answers too, and the sanitizers
stay silent.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import coord_decode_cases as cases
import coord_writer as cw
from metagraph_amd import aligner as A
from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("coord_decode")
    out = str(d / "coord_decode_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + emu,
                    "-o", out, os.path.join(emu, "coord_decode_check.cpp")], check=True)
    return out


def run_model(exe, groups):
    """groups: [[paths of one load]] -> [(status, message or (n_rows, labels, col_begin, rows, coord_begin, coords))]"""
    res = []
    for at in range(0, len(groups), 300):
        part = groups[at:at + 300]
        args = [exe]
        for g in part:
            args += [str(g[0]) + ".out"] + [str(p) for p in g] + ["--"]
        r = subprocess.run(args[:-1], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(part), r.stdout[-2000:]
        for g, line in zip(part, lines):
            status, _, rest = line.partition(" ")
            if status != "ok":
                res.append((status, rest))
                continue
            raw = open(str(g[0]) + ".out", "rb").read()
            n_rows, n_labels, n_entries, n_coords = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=4))
            at_byte, labels = 32, []
            for _ in range(n_labels):
                ln = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=at_byte)[0])
                labels.append(raw[at_byte + 8:at_byte + 8 + ln].decode())
                at_byte += 8 + ln
            tail = np.frombuffer(raw[at_byte:], dtype=np.uint64)
            assert len(tail) == n_labels + 1 + n_entries + n_entries + 1 + n_coords
            cb, tail = tail[:n_labels + 1], tail[n_labels + 1:]
            rows, tail = tail[:n_entries], tail[n_entries:]
            cob, co = tail[:n_entries + 1], tail[n_entries + 1:].view(np.int64)
            res.append(("ok", (n_rows, labels, cb.tolist(), rows.tolist(), cob.tolist(), co.tolist())))
    return res


def host(paths):
    """the host reader's answer in the model's terms"""
    try:
        n_rows, names, cb, rows, cob, co = A.read_column_files(paths, coordinates=True)
    except A.MgxError as e:
        assert e.code in (capi.MGX_ERR_INVALID, capi.MGX_ERR_UNSUPPORTED)
        return ("invalid" if e.code == capi.MGX_ERR_INVALID else "unsupported", str(e))
    return ("ok", (n_rows, names, cb.tolist(), rows.tolist(), cob.tolist(), co.tolist()))


def same_answer(h, m, what):
    assert h[0] == m[0], (what, h[0], m[0], h[1] if h[0] != "ok" else "", m[1] if m[0] != "ok" else "")
    if h[0] == "ok":
        for x, key in enumerate(("n_rows", "labels", "col_begin", "rows", "coord_begin", "coords")):
            assert h[1][x] == m[1][x], (what, key)


def test_well_formed_cases(exe, tmp_path):
    groups = [cw.write_case(tmp_path, case) for case in cases.well_formed()]
    for case, g, m in zip(cases.well_formed(), groups, run_model(exe, groups)):
        h = host(g)
        assert h[0] == "ok", (case["name"], h)
        same_answer(h, m, case["name"])


def test_damaged_files_get_the_host_readers_answer(exe, tmp_path):
    groups, want = [], []
    for name, form, files, code, words in cases.damaged():
        groups.append(cw.write_case(tmp_path, {"name": name, "form": form, "files": files}))
        want.append(("invalid" if code == "MGX_ERR_INVALID" else "unsupported", words))
    for g, m, (status, words) in zip(groups, run_model(exe, groups), want):
        h = host(g)
        same_answer(h, m, g)
        assert h[0] == status and words in h[1] and words in m[1], (g, h, m)


def test_bit_flips_and_truncations(exe, tmp_path):
    """every truncation of a small side file and of a small `.column_coord.annodbg`, and 300 random single-bit flips in each, one
    delimiter representation per column: the model's verdict (these tables / invalid / unsupported) is the host reader's on every one"""
    rng = np.random.default_rng(99)
    n, labels, cols = 70, ["p", "q", "r", "s"], [[1, 5, 64], [2, 69], list(range(0, 70, 3)), [7]]
    tuples = [[[10, 20], [], [1, 2, 3]], [[4], [8, 9]], [[r, r + 1] for r in range(0, 70, 3)], [list(range(100, 166))]]
    colfile, side = cw.coord_pair(n, labels, cols, tuples, kinds=cw.KINDS, widths=[7, 33, 8, 63])
    whole = cw.column_coord_file(n, labels, cols, tuples, kinds=cw.KINDS[::-1])
    groups, what = [], []

    def add(name, a_side=None, b_whole=None):
        i = len(groups)
        if b_whole is None:
            groups.append(cw.write_case(tmp_path, {"name": "m%05d" % i, "form": "a", "files": [(colfile, a_side)]}))
        else:
            groups.append(cw.write_case(tmp_path, {"name": "m%05d" % i, "form": "b", "files": [b_whole]}))
        what.append(name)

    for cut in range(len(side)):
        add("side cut at %d" % cut, a_side=side[:cut])
    for cut in range(0, len(whole), 3):
        add("whole cut at %d" % cut, b_whole=whole[:cut])
    for _ in range(300):
        bad = bytearray(side)
        at = int(rng.integers(0, len(bad)))
        bad[at] ^= 1 << int(rng.integers(0, 8))
        add("side flip in byte %d" % at, a_side=bytes(bad))
        bad = bytearray(whole)
        at = int(rng.integers(0, len(bad)))
        bad[at] ^= 1 << int(rng.integers(0, 8))
        add("whole flip in byte %d" % at, b_whole=bytes(bad))
    refused = kept = 0
    for name, g, m in zip(what, groups, run_model(exe, groups)):
        h = host(g)
        same_answer(h, m, name)
        refused += h[0] != "ok"
        kept += h[0] == "ok"
    assert refused > 500 and kept > 20, (refused, kept)      # (a flipped value bit passes everywhere and gives the same changed tables)
