"""The substitution class of the lane extender's exact exit on label-aware batches (level 3: metagraph_amd/csrc/lane_read.hpp
lane_exact_class<true>(), lane_exact_sub<true>(); DESIGN.md 3.4 "the substitution class, label-aware"): a label-aware read with one
substitution behind its first k characters whose seeds leave one label L and whose path — mapped and walked nodes — carries the
row { L } all along is finished in closed form, the alignment with one mismatch and the label list [L].  CPU only.

(a) The argument, on the oracle alone: for every read that meets the predicate (tests/lane_exact_sub_label_worlds.py) the oracle's
    LabeledAligner result IS the closed form, on the directed world (every refusal kind by name) and on random worlds with the
    benchmark's annotation in small, which must hold class reads, reads refused by a row alone and reads refused by the walk alone.
(b) The host model at level 3 (MGX_EMU_LANE=1, MGX_EMU_LANE_EXACT=3), read by read against the oracle and against level 0; the
    reads with an alignment and no extension are exactly span + path + sub; the record's seed counts and num_matching are the
    filter's; at level 2 the substitution reads run the DP.  Under the CLI's configuration, with the sub-k seeder reaching further
    down, and under ti_tv (transitions -2, transversions -3).
Before label-aware batches took level 3, MGX_EMU_LANE_EXACT=3 meant 2 for them: every "exact3 == every" below failed."""
import pytest

import emu_drv
import lane_exact_sub_label_worlds as SLW
import lane_exact_sub_worlds as SW
from metagraph_amd import capi

K = 21
_worlds, _checked = {}, {}


def config(cname, k):
    if cname == "later":
        return SLW.later_seed_config(k)
    return SW.configurations(k, 100)[cname]


def world(name):
    """name -> (graph, annotation, reads, directed rows or None), built once"""
    if name not in _worlds:
        if name == "directed":
            g, anno, rows = SLW.directed_world(K)
            _worlds[name] = (g, anno, [r[1] for r in rows], rows)
        else:
            _worlds[name] = SLW.random_world(int(name.split("_")[1])) + (None,)
    return _worlds[name]


def checked(name, cname):
    """the classes of a world under a configuration and the oracle's results, computed once, shared and never changed"""
    if (name, cname) not in _checked:
        g, anno, reads, _ = world(name)
        _checked[(name, cname)] = SLW.check_closed_form(g, anno, config(cname, g.k), reads)
    return _checked[(name, cname)]


RANDOM = ["random_1", "random_2", "random_3"]
CASES = [("directed", "cli"), ("directed", "later"), ("directed", "ti_tv")] + [(n, "cli") for n in RANDOM] + [("random_1", "ti_tv")]


# ---- (a) the oracle alone ----
@pytest.mark.parametrize("cname", ["cli", "later", "ti_tv"])
def test_oracle_on_the_directed_world(cname):
    c, want = checked("directed", cname)                     # (check_closed_form asserts the closed form read by read)
    g, anno, reads, rows = world("directed")
    got = {rows[q][0]: ("sub" if q in c.sub else "out") for q in range(len(rows))}
    at = {rows[q][0]: q for q in range(len(rows))}
    print(cname, "path:", len(c.path), "sub:", len(c.sub), "row:", len(c.refused_row), "walk:", len(c.refused_walk),
          "later seed:", len(c.refused_seed), "of", len(reads))
    for name, r, kind in rows:
        if kind is not None:
            assert got[name] == kind, (name, kind, got[name])
    # (a) the mismatch positions, both strands
    for p in (K, 50, 100 - K - 1, 100 - K + 3, 98, 99):
        for name, strand in (("p_%d" % p, 0), ("p_%d_rc" % p, 1)):
            assert c.sub[at[name]][0] == strand and c.sub[at[name]][1] == p, name
    assert c.label[at["p_50"]] == 0 and c.label[at["label_1"]] == 1
    # (b), (c) refused by a row alone — the walked nodes' for (b) and the edges lo and hi; the mapped nodes next to the run are
    # seeds' first nodes as well, so the filter has turned those reads away before
    for name in ["walk_row_%s%s" % (kind, t) for kind in ("other", "two", "none") for t in ("", "_tail")] + ["edge_lo", "edge_hi"]:
        assert at[name] in c.refused_row and at[name + "_rc"] in c.refused_row, name
    for name in ("edge_lo_minus_1", "edge_hi_plus_1", "boundary", "other_strand_label"):
        q = at[name]
        assert q not in c.sub and q not in c.refused_row and q not in c.refused_walk, name
    # (d), (f) no alignment at all: two one-label rows; a strand the filter emptied
    assert want[at["boundary"]] == [] and want[at["short_under_min_exact_match"]] == []
    # (g) refused by the walk, labelled { 0 } all along
    for name in ("insertion", "snp_site", "recomb_p96", "recomb_p98"):
        assert at[name] in c.refused_walk, name
    # (h) a later sub-k seed off the path; and class reads whose sub-k seeds lie on it
    assert c.refused_seed
    seeds = (c.run.seeds(0), c.run.seeds(1))
    assert any(sd["offset"] for q in c.sub for sd in seeds[c.sub[q][0]][q][0])


@pytest.mark.parametrize("name", RANDOM)
def test_oracle_on_random_worlds(name):
    c, _ = checked(name, "cli")
    g, anno, reads, _ = world(name)
    print(name, "path:", len(c.path), "sub:", len(c.sub), "row:", len(c.refused_row), "walk:", len(c.refused_walk), "of", len(reads))
    assert len(c.sub) > 0 and len(c.refused_row) > 0 and len(c.refused_walk) > 0
    assert {s for s, _, _, _ in c.sub.values()} == {0, 1}
    assert c.path


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
    return r, got, {q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0}, info


@pytest.mark.parametrize("name,cname", CASES)
def test_host_model_at_level_3_equals_the_oracle_and_level_0(name, cname, monkeypatch):
    g, anno, reads, _ = world(name)
    cfg = config(cname, g.k)
    c, want = checked(name, cname)
    every = set(c.span) | set(c.path) | set(c.sub)
    assert c.sub
    r3, got3, exact3, info3 = run_model(g, anno, cfg, reads, 3, monkeypatch)
    for q in range(len(reads)):
        assert got3[q] == want[q], (q, reads[q], got3[q], want[q])
    assert exact3 == every, sorted(exact3 ^ every)
    reasons3 = r3.lane_reasons()
    assert all(reasons3[q] == 0 for q in every)
    r0, got0, exact0, info0 = run_model(g, anno, cfg, reads, 0, monkeypatch)
    assert got0 == got3 and not exact0
    reasons0 = r0.lane_reasons()
    assert all(reasons3[q] == reasons0[q] for q in range(len(reads)) if q not in every)
    assert r3.lane_stats()[1] == r0.lane_stats()[1] + sum(1 for q in every if reasons0[q])
    # the record and the seed dump: the oracle's filtered seed lists and num_matching at both levels
    seeds = (c.run.seeds(0), c.run.seeds(1))
    for q in range(len(reads)):
        for s in (0, 1):
            assert info3[q]["num_matches"][s] == info0[q]["num_matches"][s] == seeds[s][q][1], (q, s, info3[q], info0[q])
            assert info3[q]["seeds"][s] == info0[q]["seeds"][s] == emu_drv.oracle_seeds_as_tuples(seeds[s][q][0]), (q, s)
        if q in every:
            assert info3[q]["n_extensions"] == 0 and info3[q]["n_columns"] == 0
            assert info3[q]["num_matches"] == (c.filtered[q][0][1], c.filtered[q][1][1])
        else:
            assert (info3[q]["n_extensions"], info3[q]["n_columns"]) == (info0[q]["n_extensions"], info0[q]["n_columns"])
    # level 2: the substitution class runs the DP
    _, got2, exact2, _ = run_model(g, anno, cfg, reads, 2, monkeypatch)
    assert got2 == got3 and exact2 == set(c.span) | set(c.path)


def test_rows_of_dummy_nodes_keep_the_exit_and_the_lane_off_at_level_3(monkeypatch):
    g, anno, reads, _ = world("directed")
    _, want = checked("directed", "cli")
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", "3")
    monkeypatch.setenv("MGX_EMU_LAB_WCHECK", "1")
    r = emu_drv.EmuRun(emu_drv.EmuGraph(g), capi.config_cli(K), reads, annotation=emu_drv.EmuAnnotation(anno))
    assert r.error == "" and r.results()[0] == want
    assert not r.lane_stats()[0]
