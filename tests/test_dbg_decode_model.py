"""The kernel bodies behind mgx_graph_load_dbg_device (metagraph_amd/csrc/dbg_decode.hpp over the plan of dbg_plan.hpp) compiled
for the host against the wave model and run by tests/emu/dbg_decode_check.cpp, a stand-alone program built with
-fsanitize=address,undefined in which every array has exactly the size the driver gives its device buffer.  It decodes files
written by tests/sdsl_writer.py (and the two reference-written ones) and dumps W / last; here the dumps are compared, byte for
byte, with the host decoder (aligner.read_boss_file = mgx_boss_file_read).  Malformed files: whatever the host decoder answers
(an error of which class, or a table) the model answers too, and the sanitizers stay silent.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import dbg_decode_cases as cases
import sdsl_writer as sw
from metagraph_amd import aligner as A
from metagraph_amd import capi
from test_boss_files import GOLD, random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = cases.HEADER


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("dbg_decode")
    out = str(d / "dbg_decode_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + emu,
                    "-o", out, os.path.join(emu, "dbg_decode_check.cpp")], check=True)
    return out


def run_model(exe, paths):
    """[(status, message or the dump's fields)] per file; the sanitizers must have had nothing to say"""
    res = []
    for at in range(0, len(paths), 400):
        part = paths[at:at + 400]
        args = [exe]
        for p in part:
            args += [str(p), str(p) + ".out"]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(part), r.stdout[-2000:]
        for p, line in zip(part, lines):
            status, _, rest = line.partition(" ")
            if status != "ok":
                res.append((status, rest))
                continue
            raw = open(str(p) + ".out", "rb").read()
            k, sigma, mode, state, n_edges = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=5))
            F = [int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=sigma, offset=40)]
            body = raw[40 + 8 * sigma:]
            assert len(body) == 2 * (n_edges + 1)
            res.append(("ok", {"k": k, "sigma": sigma, "mode": mode, "state": state, "n_edges": n_edges, "F": F,
                               "W": body[:n_edges + 1], "last": body[n_edges + 1:]}))
    return res


def host(path):
    """the host decoder's answer in the model's terms"""
    try:
        f = A.read_boss_file(path)
    except A.MgxError as e:
        assert e.code in (capi.MGX_ERR_INVALID, capi.MGX_ERR_UNSUPPORTED)
        return ("invalid" if e.code == capi.MGX_ERR_INVALID else "unsupported", str(e))
    f["W"], f["last"] = f["W"].tobytes(), f["last"].tobytes()
    return ("ok", f)


def same_answer(h, m, what):
    assert h[0] == m[0], (what, h[:1], m[:1], h[1] if h[0] != "ok" else "", m[1] if m[0] != "ok" else "")
    if h[0] == "ok":
        for key in ("k", "sigma", "mode", "state", "n_edges", "F", "W", "last"):
            assert h[1][key] == m[1][key], (what, key)


def check_files(exe, paths):
    for p, m in zip(paths, run_model(exe, paths)):
        h = host(p)
        assert h[0] == "ok", (p, h)
        same_answer(h, m, p)


def check_cases(exe, tmp_path, shapes):
    paths = []
    for name, data in shapes:
        p = tmp_path / (name + ".dbg")
        p.write_bytes(data)
        paths.append(p)
    check_files(exe, paths)


def test_rrr_shapes(exe, tmp_path):
    check_cases(exe, tmp_path, cases.rrr_cases())


@pytest.mark.parametrize("state", [sw.STATE_SMALL, sw.STATE_STAT])
def test_wavelet_tree_shapes(exe, tmp_path, state):
    check_cases(exe, tmp_path, cases.wt_cases(state))


def test_sd_last_shapes(exe, tmp_path):
    shapes = cases.sd_cases()
    check_cases(exe, tmp_path, shapes)
    for name, data in shapes:
        if name.startswith("sd_wl0"):
            assert A.read_boss_file(tmp_path / (name + ".dbg"))["last"].tolist() == [int(name[-1])] * 100


def test_fast_state_lengths(exe, tmp_path):
    check_cases(exe, tmp_path, cases.fast_cases())


def test_whole_files(exe, tmp_path):
    """the two reference-written graphs (the protein graph: decode only) and the writer's files in every state, `last` code and
    mode that test_gpu_files.py loads"""
    rng = np.random.default_rng(5)
    paths = [os.path.join(GOLD, "test_DNA_graph.dbg"), os.path.join(GOLD, "test_Protein_graph.dbg")]
    copies = []
    for p in paths:                                           # (the model writes its dump next to its input)
        c = tmp_path / os.path.basename(p)
        c.write_bytes(open(p, "rb").read())
        copies.append(c)
    for state, last_code, mode in [(sw.STATE_SMALL, sw.CODE_RRR, 0), (sw.STATE_SMALL, sw.CODE_SD, 1), (sw.STATE_STAT, None, 2), (sw.STATE_FAST, None, 0)]:
        W, last, F = random_table(rng, 11, 3, 700, mode=min(mode, 1))
        c = tmp_path / ("w_%d_%d.dbg" % (state, mode))
        c.write_bytes(sw.dbg_file(11, W, last, F, mode=mode, state=state, last_code=last_code or sw.CODE_RRR))
        copies.append(c)
    check_files(exe, copies)
    assert host(copies[1])[1]["sigma"] > 5


def test_malformed_files(exe, tmp_path):
    """truncations of a small file in every state (every cut, which takes in every container boundary), a flipped bit in each
    byte-sized piece the kernels' checks guard — a block type, a block number, a child index, a stored count of ones, wl — and
    300 random single-bit flips per file; a one-element file and a DYN-state file.  The model gives the host decoder's answer
    (MGX_ERR_INVALID, MGX_ERR_UNSUPPORTED, or the same table where the damage passes the checks)"""
    rng = np.random.default_rng(6)
    W, last, F = random_table(rng, 6, 2, 60)
    n = len(W)
    kinds = {"rrr": (sw.STATE_SMALL, sw.CODE_RRR), "sd": (sw.STATE_SMALL, sw.CODE_SD), "stat": (sw.STATE_STAT, sw.CODE_RRR), "fast": (sw.STATE_FAST, sw.CODE_RRR)}
    files = {name: sw.dbg_file(6, W, last, F, state=st, last_code=lc) for name, (st, lc) in kinds.items()}
    wt_rrr, wt_plain = sw.wt_huff(W.tolist(), True), sw.wt_huff(W.tolist(), False)
    n_nodes = 2 * len(set(W.tolist())) - 1
    levels = int(np.frombuffer(wt_rrr[16:24], dtype=np.uint64)[0])
    bt_words = (6 * (levels // 63 + 1) + 63) // 64
    targets = {                                               # name -> (file, first byte, bytes)
        "bt": ("rrr", HEADER + 16 + 8 + 9, 1),
        "btnr": ("rrr", HEADER + 16 + 8 + 9 + 8 * bt_words + 8, 8),
        "child": ("rrr", HEADER + len(wt_rrr) - 2560 - 22 * n_nodes + 18, 4),
        "child (plain levels)": ("stat", HEADER + len(wt_plain) - 2560 - 22 * n_nodes + 18, 4),
        "ones": ("stat", HEADER + len(wt_plain) + 8 + 8 + 8 * ((n + 63) // 64) + 7, 1),
        "wl": ("sd", HEADER + len(wt_rrr) + 8 + 8 + 8, 1),
    }
    damaged = []                                                # (what, bytes)
    for name, data in files.items():
        damaged += [("%s cut at %d" % (name, cut), data[:cut]) for cut in range(len(data))]
        for _ in range(300):
            bad = bytearray(data)
            at = int(rng.integers(0, len(bad)))
            bad[at] ^= 1 << int(rng.integers(0, 8))
            damaged.append(("%s flip in byte %d" % (name, at), bytes(bad)))
    for what, (name, at, nbytes) in targets.items():
        for bit in range(8 * nbytes):
            bad = bytearray(files[name])
            bad[at + bit // 8] ^= 1 << (bit % 8)
            damaged.append(("%s bit %d" % (what, bit), bytes(bad)))
    damaged.append(("one element", sw.dbg_file(6, [0], [1], [0, 0, 0, 0, 0])))
    dyn = bytearray(files["rrr"])
    dyn[HEADER - 1] = sw.STATE_DYN
    damaged.append(("DYN state", bytes(dyn)))
    paths = []
    for i, (what, data) in enumerate(damaged):
        p = tmp_path / ("m%05d.dbg" % i)
        p.write_bytes(data)
        paths.append(p)
    answers = run_model(exe, paths)
    invalid = set()
    for (what, _), p, m in zip(damaged, paths, answers):
        h = host(p)
        same_answer(h, m, what)
        if h[0] == "invalid":
            invalid.add(what.split(" bit ")[0].split(" cut ")[0])
    # every family of damage is one the host decoder does refuse somewhere (the flips are in the right bytes)
    assert {"bt", "btnr", "child", "child (plain levels)", "ones", "wl", "rrr", "sd", "stat", "fast", "one element"} <= invalid, invalid
    assert host(paths[-1])[0] == "unsupported"
