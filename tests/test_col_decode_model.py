"""The kernel bodies behind mgx_annotation_load_columns_device (metagraph_amd/csrc/col_decode.hpp over the plan and batch layout of
col_plan.hpp) compiled for the host and run by tests/emu/col_decode_check.cpp, a stand-alone program built with
-fsanitize=address,undefined in which every array has exactly the size the driver gives its device buffer.  It decodes the files of
tests/col_decode_cases.py (and the two reference-written ones) and dumps n_rows, labels, col_begin and rows; here the dumps are
compared with the host reader (aligner.read_column_files = mgx_column_file_read).  Damaged files: whatever the host reader answers
(an error of which class, or these tables) the model answers too, and the sanitizers stay silent.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import col_decode_cases as cases
import sdsl_writer as sw
from metagraph_amd import aligner as A
from metagraph_amd import capi
from test_boss_files import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = [os.path.join(GOLD, "test_DNA_graph.column.annodbg"), os.path.join(GOLD, "test_Protein_graph.column.annodbg")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("col_decode")
    out = str(d / "col_decode_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + emu,
                    "-o", out, os.path.join(emu, "col_decode_check.cpp")], check=True)
    return out


def run_model(exe, groups):
    """groups: [[paths of one load]] -> [(status, message or (n_rows, labels, col_begin, rows))]; the sanitizers must have had
    nothing to say"""
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
            n_rows, n_labels = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=2))
            at_byte, labels = 16, []
            for _ in range(n_labels):
                ln = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=at_byte)[0])
                labels.append(raw[at_byte + 8:at_byte + 8 + ln].decode())
                at_byte += 8 + ln
            tail = np.frombuffer(raw[at_byte:], dtype=np.uint64)
            cb, rows = tail[:n_labels + 1], tail[n_labels + 1:]
            assert len(rows) == int(cb[-1])
            res.append(("ok", (n_rows, labels, cb.tolist(), rows.tolist())))
    return res


def host(paths):
    """the host reader's answer in the model's terms"""
    try:
        n_rows, names, cb, rows = A.read_column_files(paths)
    except A.MgxError as e:
        assert e.code in (capi.MGX_ERR_INVALID, capi.MGX_ERR_UNSUPPORTED)
        return ("invalid" if e.code == capi.MGX_ERR_INVALID else "unsupported", str(e))
    return ("ok", (n_rows, names, cb.tolist(), rows.tolist()))


def same_answer(h, m, what):
    assert h[0] == m[0], (what, h[0], m[0], h[1] if h[0] != "ok" else "", m[1] if m[0] != "ok" else "")
    if h[0] == "ok":
        for x, key in enumerate(("n_rows", "labels", "col_begin", "rows")):
            assert h[1][x] == m[1][x], (what, key)


def write_case(d, case):
    paths = []
    for i, data in enumerate(case["files"]):
        p = d / ("%s_%d.column.annodbg" % (case["name"], i))
        p.write_bytes(data)
        paths.append(p)
    return paths


def test_writer_and_host_reader_agree(tmp_path):
    """the case list itself: the host reader accepts every well-formed case and returns the rows it was written from"""
    for case in cases.well_formed():
        n_rows, names, cb, rows = A.read_column_files(write_case(tmp_path, case))
        assert (n_rows, names) == (case["n_rows"], case["labels"]), case["name"]
        assert [rows[int(cb[j]):int(cb[j + 1])].tolist() for j in range(len(names))] == case["columns"], case["name"]
    case = next(c for c in cases.well_formed() if c["name"] == "rows129")
    by = dict(zip(case["labels"], case["columns"]))
    assert len(by["sd_half"]) == 64 and len(by["sd_half1"]) == 65 and len(by["sd_full"]) == 129      # not inverted / inverted / nothing stored


def test_well_formed_cases(exe, tmp_path):
    groups = [write_case(tmp_path, case) for case in cases.well_formed()]
    for case, g, m in zip(cases.well_formed(), groups, run_model(exe, groups)):
        h = host(g)
        assert h[0] == "ok", (case["name"], h)
        same_answer(h, m, case["name"])


def test_reference_written_files(exe, tmp_path):
    groups = []
    for p in GOLDEN:                                            # (the model writes its dump next to its input)
        c = tmp_path / os.path.basename(p)
        c.write_bytes(open(p, "rb").read())
        groups.append([c])
    for g, m in zip(groups, run_model(exe, groups)):
        h = host(g)
        assert h[0] == "ok" and len(h[1][3]) > 0
        same_answer(h, m, g[0])


def test_files_that_do_not_go_together(exe, tmp_path):
    groups, want = [], []
    for name, files, code, words in cases.bad_merges():
        groups.append(write_case(tmp_path, {"name": name, "files": files}))
        want.append(("invalid" if code == "MGX_ERR_INVALID" else "unsupported", words))
    for g, m, (status, words) in zip(groups, run_model(exe, groups), want):
        h = host(g)
        same_answer(h, m, g)
        assert h[0] == status and words in h[1] and words in m[1]


def test_damaged_files(exe, tmp_path):
    """every truncation of four small files (one per code and a mixed one; the sd file with a plain and an inverted column, both
    label encoders among them), a flipped bit in each piece the kernels' checks guard — a block type, a block number, a stored count of ones, the
    tail of the plain bits, wl, a low part, a high part, the inverted flag, a representation code, num_rows — and 400 random
    single-bit flips per file.  The model's verdict (these tables / invalid / unsupported) is the host reader's on every one"""
    rng = np.random.default_rng(77)
    n = 150
    sparse = sorted(int(r) for r in rng.choice(n, size=40, replace=False))
    dense = sorted(int(r) for r in rng.choice(n, size=120, replace=False))
    files = {"sd": sw.column_file(n, ["s", "d"], [sparse, dense], codes=[sw.CODE_SD, sw.CODE_SD]),
             "stat": sw.column_file(n, ["s", "d"], [sparse, dense], codes=[sw.CODE_STAT, sw.CODE_STAT], v2=True),
             "rrr": sw.column_file(n, ["s", "d"], [sparse, dense], codes=[sw.CODE_RRR, sw.CODE_RRR]),
             "mixed": sw.column_file(n, ["a", "b", "c"], [dense, sparse, dense], codes=[sw.CODE_RRR, sw.CODE_SD, sw.CODE_STAT])}
    head1 = len(sw.be(n) + sw.label_encoder_v1(["s", "d"]))
    head2 = len(sw.be(n) + sw.label_encoder_v2(["s", "d"]))
    sd0 = sw.bit_vector_sd([1 if r in set(sparse) else 0 for r in range(n)])
    low_words = (40 * sd0[8] + 63) // 64
    stat_words = (n + 63) // 64
    bt_words = (6 * (n // 63 + 1) + 63) // 64
    targets = {                                                 # name -> (file, first byte, bytes)
        "num_rows": ("sd", 0, 8),
        "code": ("sd", head1, 8),
        "sd size": ("sd", head1 + 8, 8),
        "wl": ("sd", head1 + 16, 1),
        "low": ("sd", head1 + 16 + 1 + 9, 8 * low_words),
        "high": ("sd", head1 + 16 + 1 + 9 + 8 * low_words + 8, 16),
        "inverted flag": ("sd", head1 + 8 + len(sd0) - 1, 1),
        "second sd column": ("sd", head1 + 8 + len(sd0) + 8 + 16 + 1 + 9, 24),
        "stat bits": ("stat", head2 + 8 + 8, 8 * stat_words),
        "stat ones": ("stat", head2 + 8 + 8 + 8 * stat_words, 8),
        "rrr size": ("rrr", head1 + 8, 8),
        "bt": ("rrr", head1 + 8 + 8 + 9, 8 * bt_words),
        "btnr": ("rrr", head1 + 8 + 8 + 9 + 8 * bt_words + 8, 16),
    }
    damaged = []                                                # (what, bytes)
    for name, data in files.items():
        damaged += [("%s cut at %d" % (name, cut), data[:cut]) for cut in range(len(data))]
        for _ in range(400):
            bad = bytearray(data)
            at = int(rng.integers(0, len(bad)))
            bad[at] ^= 1 << int(rng.integers(0, 8))
            damaged.append(("%s flip in byte %d" % (name, at), bytes(bad)))
    for what, (name, at, nbytes) in targets.items():
        for bit in range(8 * nbytes):
            bad = bytearray(files[name])
            bad[at + bit // 8] ^= 1 << (bit % 8)
            damaged.append(("%s bit %d" % (what, bit), bytes(bad)))
    assert len(damaged) > 4000
    groups = []
    for i, (what, data) in enumerate(damaged):
        p = tmp_path / ("m%05d.column.annodbg" % i)
        p.write_bytes(data)
        groups.append([p])
    answers = run_model(exe, groups)
    refused, kept = set(), set()
    for (what, _), g, m in zip(damaged, groups, answers):
        h = host(g)
        same_answer(h, m, what)
        (refused if h[0] != "ok" else kept).add(what.split(" bit ")[0].split(" cut ")[0].split(" flip ")[0])
    # every family of damage is one the host reader does refuse somewhere (the flips are in the right bytes), and some damage
    # passes the checks (a changed row) and gives the same changed tables
    # (any non-zero flag byte means inverted, and a low part may be changed into another ascending one: both can pass everywhere)
    must = (set(targets) | set(files)) - {"inverted flag", "low"}
    assert must <= refused, sorted(must - refused)
    assert {"inverted flag", "low"} <= kept, kept
