"""The lane extender's exact exit on label-aware batches (metagraph_amd/csrc/lane_read.hpp lane_exact_class(), DESIGN.md 3.4
"label-aware batches"): a read that keeps one label all along — the one-label seed filter leaves a label L, every mapped node of
the strand aligned has the row { L } — and meets the conditions of one of the exit's two classes is finished in closed form: the
all-match alignment over the strand's mapped nodes with the label list [L].  CPU only.

(a) The argument, on the oracle alone: for every read that meets the predicate (tests/lane_exact_label_worlds.py: from the
    oracle's seeds, mapping() and Annotation.get_rows()), the oracle's LabeledAligner result IS the closed form — on directed
    worlds (bubbles whose alternative path carries the same label, another label, two labels, none; reads across a segment
    boundary) and on random worlds with the benchmark's annotation in small, at k = 15, 21 and 31.
(b) The host model at level 2 (MGX_EMU_LANE_EXACT=2 with MGX_EMU_LANE=1), read by read against the oracle and against level 0:
    alignments, label lists, the label filter's seed lists and num_matching (which pins the exit's copy of the filter to
    lane_read_dp()'s); the reads with an alignment and no extension are exactly the predicate's; every other read's hand-over
    code is what it is at level 0.
(c) Level 1 leaves the path class to the DP.
(d) The row scan at the ends of the node array and of the annotation, the filter, and the output stream's capacity, in a
    stand-alone program (tests/emu/lane_exact_label_check.cpp) built with the address and undefined-behaviour sanitizers.

The label-aware seeder makes one seed per k-mer (min_seed_length and max_seed_length are clamped to k), so the span class is the
reads of k characters and the path class the longer ones; every world must hold both."""
import os
import re
import subprocess

import pytest

import emu_drv
import lane_exact_label_worlds as LW
from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_worlds = {}


def world(name):
    """name -> (graph, annotation, reads, directed rows or None), built once"""
    if name not in _worlds:
        kind, a, k = name.split("_")
        if kind == "directed":
            g, anno, rows = LW.directed_world(int(k))
            _worlds[name] = (g, anno, [r[1] for r in rows], rows)
        elif kind == "segment":
            _worlds[name] = LW.segment_directed(int(a), int(k)) + (None,)
        else:
            _worlds[name] = LW.random_world(int(a), int(k)) + (None,)
    return _worlds[name]


_checked = {}


def checked(name):
    """the classes of a world with the CLI's configuration and the oracle's results (with label lists), computed once and shared"""
    if name not in _checked:
        g, anno, reads, _ = world(name)
        _checked[name] = LW.check_closed_form(g, anno, capi.config_cli(g.k), reads)
    return _checked[name]


DIRECTED = ["directed_0_15", "directed_0_21", "directed_0_31", "segment_2_21", "segment_3_21", "segment_4_15"]
RANDOM = ["random_%d_%d" % (s, k) for s, k in ((1, 15), (2, 21), (3, 31), (4, 15), (5, 21), (6, 31))]


# ---- (a) the oracle alone ----
@pytest.mark.parametrize("name", DIRECTED + RANDOM)
def test_oracle_result_of_a_class_read_is_the_closed_form(name):
    c, _ = checked(name)                                     # (check_closed_form asserts it read by read)
    g, anno, reads, rows = world(name)
    print(name, "span class:", len(c.span), "path class:", len(c.path), "of", len(reads))
    assert c.span and c.path, (len(c.span), len(c.path))
    assert all(len(reads[q]) == g.k for q in c.span)
    both = set(c.span) | set(c.path)
    assert len(both) < len(reads)
    if rows is not None:
        got = {rows[q][0]: ("in" if q in both else "out") for q in range(len(rows))}
        for q, (rname, r, kind) in enumerate(rows):
            # what must stay out stays out whatever the seeder does; what is meant to be in is in where every seed is a k-mer
            # (k = 31: min_seed_length 19 < k adds sub-k seeds on the other strand, whose rows decide)
            if kind == "out" or g.k < 31:
                assert got[rname] == kind, (rname, kind, got[rname])
        for bubble in ("same", "other", "two", "none"):
            assert got["main_%s_100" % bubble] == "in" or g.k == 31
            assert got["alt_%s_100" % bubble] == ("in" if bubble == "same" else "out")


def test_random_worlds_hold_reads_refused_for_each_row_reason():
    """a read that passes the seed filter and the unlabeled conditions and fails on a row of its path alone: another label, two
    labels with L among them, no label"""
    seen = set()
    for name in RANDOM + DIRECTED[:3]:
        c, _ = checked(name)
        g, anno, reads, _ = world(name)
        both = set(c.span) | set(c.path)
        for q in range(len(reads)):
            if q in both or len(reads[q]) < g.k:
                continue
            for s in (0, 1):
                mapped = c.nodes[q][s]
                if not mapped or 0 in mapped:
                    continue
                rows = [[int(x) for x in anno.get_rows([v - 1])[0]] for v in mapped]
                first = rows[0]
                if len(first) != 1:
                    continue
                for r in rows:
                    if r != first:
                        seen.add("none" if not r else "two" if len(r) > 1 and first[0] in r else "other" if len(r) == 1 else "several")
    assert {"none", "two", "other"} <= seen, seen


# ---- (b) the host model ----
def run_model(g, anno, cfg, reads, level, monkeypatch):
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", str(level))
    r = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads, annotation=emu_drv.EmuAnnotation(anno))
    assert r.error == "", r.error
    got, status = r.results()
    assert all(s == 0 for s in status), status
    assert r.lane_stats()[0]
    info = r.seed_info()
    exact_reads = {q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0}
    return r, got, exact_reads, info


def check_model(name, monkeypatch):
    g, anno, reads, _ = world(name)
    cfg = capi.config_cli(g.k)
    c, want = checked(name)
    both = set(c.span) | set(c.path)
    r2, got2, exact2, info2 = run_model(g, anno, cfg, reads, 2, monkeypatch)
    for q in range(len(reads)):
        assert got2[q] == want[q], (q, reads[q], got2[q], want[q])
    assert exact2 == both, sorted(exact2 ^ both)
    reasons2 = r2.lane_reasons()
    assert all(reasons2[q] == 0 for q in both)
    r0, got0, exact0, info0 = run_model(g, anno, cfg, reads, 0, monkeypatch)
    assert got0 == got2 and not exact0
    reasons0 = r0.lane_reasons()
    assert all(reasons2[q] == reasons0[q] for q in range(len(reads)) if q not in both)
    assert r2.lane_stats()[1] == r0.lane_stats()[1] + sum(1 for q in both if reasons0[q])
    # the record and the seed dump: what lane_read_dp() (or, for a read it hands over, the group kernel) writes — the oracle's
    # filtered seed lists and num_matching; only the extension and column counts of a class read differ
    seeds = (c.run.seeds(0), c.run.seeds(1))
    for q in range(len(reads)):
        for s in (0, 1):
            assert info2[q]["num_matches"][s] == info0[q]["num_matches"][s] == seeds[s][q][1], (q, s, info2[q], info0[q])
            assert info2[q]["seeds"][s] == info0[q]["seeds"][s] == emu_drv.oracle_seeds_as_tuples(seeds[s][q][0]), (q, s)
        if q in both:
            assert info2[q]["n_extensions"] == 0 and info2[q]["n_columns"] == 0
            # (the predicate's own recount against the device's)
            assert info2[q]["num_matches"] == (c.filtered[q][0][1], c.filtered[q][1][1])
        else:
            assert (info2[q]["n_extensions"], info2[q]["n_columns"]) == (info0[q]["n_extensions"], info0[q]["n_columns"])
    return c, reasons0


@pytest.mark.parametrize("name", DIRECTED + RANDOM)
def test_host_model_at_level_2_equals_the_oracle_and_level_0(name, monkeypatch):
    c, reasons0 = check_model(name, monkeypatch)
    assert c.span and c.path
    # some class reads the DP finishes too, and reads outside the classes that it finishes or hands over
    both = set(c.span) | set(c.path)
    assert any(reasons0[q] == 0 for q in both)
    assert any(q not in both for q in range(len(reasons0)))


def test_host_model_level_1_leaves_the_path_class_to_the_dp(monkeypatch):
    name = "directed_0_21"
    g, anno, reads, _ = world(name)
    c, want = checked(name)
    _, got, exact1, _ = run_model(g, anno, capi.config_cli(21), reads, 1, monkeypatch)
    assert exact1 == set(c.span) and c.path and got == want


def test_rows_of_dummy_nodes_keep_the_exit_and_the_lane_off(monkeypatch):
    """MGX_EMU_LAB_WCHECK=1 keeps AlignParams::labeled at 1 (as an annotation whose dummy rows hold labels does): lane_enabled()
    and lane_exact_config() both refuse, results are the oracle's"""
    name = "directed_0_15"
    g, anno, reads, _ = world(name)
    _, want = checked(name)
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", "2")
    monkeypatch.setenv("MGX_EMU_LAB_WCHECK", "1")
    r = emu_drv.EmuRun(emu_drv.EmuGraph(g), capi.config_cli(15), reads, annotation=emu_drv.EmuAnnotation(anno))
    assert r.error == "" and r.results()[0] == want
    assert not r.lane_stats()[0]


# ---- (d) the row scan, the filter and the capacity, stand-alone under the sanitizers ----
def test_row_scan_filter_and_emit_at_the_capacity_of_the_stream(tmp_path):
    exe = str(tmp_path / "lane_exact_label_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DMGX_MAX_ALT=4", "-DMGX_WITH_PRIMARY=1", "-DMGX_WITH_LABELS=1", "-w",
                    "-I" + emu, "-I" + os.path.join(ROOT, "metagraph_amd", "csrc"), "-o", exe,
                    os.path.join(emu, "lane_exact_label_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.match(r"ok (\d+) cases, (\d+) refusals", r.stdout)
    # 13 lengths x 2 strands x 4 alignments of the node array; per case at least: three wrong rows at the first node, the last and
    # every node in turn
    assert m and int(m.group(1)) == 13 * 2 * 4 and int(m.group(2)) >= 13 * 2 * 4 * 9, r.stdout
