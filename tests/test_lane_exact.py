"""The exact exit of the lane-per-read extender (metagraph_amd/csrc/lane_read.hpp lane_exact(); lane_types.hpp
lane_exact_config()): a read whose first seed — of the strand aligned first — spans the query is finished in closed
form, without DP.  CPU only.

(a) The argument, on the oracle alone: for every read that meets the predicate (evaluated from the oracle's seeds,
    tests/lane_exact_worlds.py), the oracle's result IS the closed form.
(b) The host model with the lane path and the exit on (MGX_EMU_LANE_EXACT=1, read where lane_enabled() fills the parameter
    block), read by read against the oracle and against the exit off; the reads that left through the exit — the host model's
    n_lane_exact_reads: its reads with an alignment and no extension — are exactly the predicate's.
(c) The output stream's capacity and the headers that must stay with the DP, in a stand-alone program (tests/emu/
    lane_exact_check.cpp: the host model's driver sizes its stream generously), built with the address and undefined-behaviour
    sanitizers.

The minimum class counts are what the oracle gives for these seeded worlds (in brackets), less a margin; a world or
configuration that is meant to have class reads and finds none fails."""
import os
import re
import subprocess

import pytest

import emu_drv
import lane_exact_worlds as W
from metagraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# world -> (builder, minimum number of class reads with the CLI's configuration)
WORLDS = {
    "bench_like": (W.world_bench, 60),               # [76 of 600]
    "snp_every_60": (W.world_snp60, 100),            # [of 400, 45-bp reads]
    "three_alleles": (W.world_three_alleles, 70),    # [95 of 211]
    "tandem_repeat": (W.world_tandem, 20),           # [27 of 120]
    "both_strands": (lambda: W.world_both_strands()[:2], 45),     # [60 of 120: none of the 40 reads of the two-strand segment]
    "lengths": (W.world_lengths, 48),                # [48 of 53: every perfect read, both strands, every length]
}
CONFIGS = ["cli", "no_end_bonus", "rel0", "min_path_at_full", "min_path_above_full", "max_seed_length_k"]
_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = WORLDS[name][0]()
    return _worlds[name]


def config(name, cname):
    g, reads = world(name)
    return W.configurations(g.k, len(reads[0]))[cname]


@pytest.mark.parametrize("cname", CONFIGS)
@pytest.mark.parametrize("name", list(WORLDS))
def test_oracle_result_of_a_class_read_is_the_closed_form(name, cname):
    g, reads = world(name)
    cfg, has_class = config(name, cname)
    n = W.check_closed_form(g, cfg, reads)
    print(name, cname, "class reads:", n, "of", len(reads))
    if name == "lengths" and not has_class:
        # (the configurations that empty the class do so for reads of ONE length: here that of the world's first reads, L = k)
        cls, _ = W.class_reads(g, cfg, reads)
        assert all(len(reads[q]) != len(reads[0]) for q in cls) or cname == "max_seed_length_k"
        if cname == "max_seed_length_k":
            assert all(len(reads[q]) == g.k for q in cls) and n == 6        # (a read of k characters IS one k-mer)
        return
    if has_class:
        assert n >= WORLDS[name][1], (n, WORLDS[name][1])
    else:
        assert n == 0


def test_reads_of_a_segment_on_both_strands_are_never_in_the_class():
    g, reads, n_x = W.world_both_strands()
    cls, o = W.class_reads(g, capi.config_cli(g.k), reads)
    assert n_x == 40 and not any(q < n_x for q in cls) and len(cls) >= 45
    # (they have a spanning first seed on either strand: it is the second-strand rule that keeps them out)
    sf, sr = o.seeds(0), o.seeds(1)
    assert all(sf[q][0] and sr[q][0] and sf[q][0][0]["length"] == 100 and sr[q][0][0]["length"] == 100 for q in range(n_x))


def test_configurations_outside_the_predicate():
    g, reads = world("lengths")
    for change in ("mismatch_equals_match", "gap_open_0", "right_end_bonus_negative", "two_paths"):
        cfg = capi.config_cli(g.k)
        if change == "mismatch_equals_match":
            capi.set_dna_matrix(cfg, 2, 2, -3)
        elif change == "gap_open_0":
            cfg.gap_opening_penalty = 0
        elif change == "right_end_bonus_negative":
            cfg.right_end_bonus = -1
        else:
            cfg.num_alternative_paths = 2
        assert not W.config_allows(cfg), change


# ---- (b) the host model ----
def run_model(g, cfg, reads, exact, monkeypatch):
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", "1" if exact else "0")
    r = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads)
    assert r.error == "", r.error
    got, status = r.results()
    assert all(s == 0 for s in status), status
    assert r.lane_stats()[0]
    info = r.seed_info()
    exact_reads = {q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0}
    return r, got, exact_reads


@pytest.mark.parametrize("cname", CONFIGS)
@pytest.mark.parametrize("name", list(WORLDS))
def test_host_model_with_the_exit_on_equals_the_oracle_and_the_exit_off(name, cname, monkeypatch):
    g, reads = world(name)
    cfg, _ = config(name, cname)
    cls, o = W.class_reads(g, cfg, reads)
    want = o.results()
    r1, got1, exact1 = run_model(g, cfg, reads, True, monkeypatch)
    for q in range(len(reads)):
        assert got1[q] == want[q], (q, reads[q], got1[q], want[q])
    # the counter: the reads that left through the exit are the predicate's, all of them finished in the lane path
    assert exact1 == set(cls), (sorted(exact1 ^ set(cls)))
    reasons1 = r1.lane_reasons()
    assert all(reasons1[q] == 0 for q in cls)
    r0, got0, exact0 = run_model(g, cfg, reads, False, monkeypatch)
    assert got0 == got1 and not exact0
    # the fate of every other read is what it was; a class read that the DP handed on (a later seed that lives, a fork, a tie)
    # no longer is
    reasons0 = r0.lane_reasons()
    assert all(reasons1[q] == reasons0[q] for q in range(len(reads)) if q not in cls)
    assert r1.lane_stats()[1] == r0.lane_stats()[1] + sum(1 for q in cls if reasons0[q])


def test_host_model_takes_the_exit_on_either_strand_and_at_every_length(monkeypatch):
    g, reads = world("lengths")
    cfg = capi.config_cli(g.k)
    cls, _ = W.class_reads(g, cfg, reads)
    _, got, exact = run_model(g, cfg, reads, True, monkeypatch)
    assert exact == set(cls)
    seen = {(len(reads[q]), got[q][0]["orientation"]) for q in exact}
    assert seen == {(L, s) for L in (g.k, g.k + 1, 32, 33, 64, 65, 150, 256) for s in (0, 1)}
    # the read with an N, the reads shorter than k, the random read, the empty read: not through the exit
    assert not any(q in exact for q in range(len(reads) - 5, len(reads)))


def test_the_exit_is_off_where_the_configuration_is_outside_the_predicate(monkeypatch):
    g, reads = world("lengths")
    for change in ("transition_equals_match", "right_end_bonus_negative"):
        cfg = capi.config_cli(g.k)
        if change == "transition_equals_match":
            capi.set_dna_matrix(cfg, 2, 2, -3)
        else:
            cfg.right_end_bonus = -1
        assert not W.config_allows(cfg)
        _, got, exact = run_model(g, cfg, reads, True, monkeypatch)
        assert not exact, change


# ---- (c) capacity and refusals, stand-alone under the sanitizers ----
def test_exact_emit_at_the_capacity_of_the_stream_and_headers_that_stay(tmp_path):
    exe = str(tmp_path / "lane_exact_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DMGX_MAX_ALT=4", "-DMGX_WITH_PRIMARY=1", "-DMGX_WITH_LABELS=1", "-w",
                    "-I" + emu, "-I" + os.path.join(ROOT, "metagraph_amd", "csrc"), "-o", exe,
                    os.path.join(emu, "lane_exact_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.match(r"ok (\d+) cases, (\d+) refusals", r.stdout)
    assert m and int(m.group(1)) == 32 and int(m.group(2)) >= 8 * 32, r.stdout
