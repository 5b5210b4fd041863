"""The substitution class of the lane extender's exact exit (level 3: metagraph_amd/csrc/lane_read.hpp lane_exact_sub(),
lane_types.hpp lane_exact_sub_config()): a read with one substitution behind its first k characters — one run of
zeros in the strand's node array, a graph walk across it that succeeds, every later seed on the walked path — is finished in closed
form: the alignment with one mismatch over the mapped and the walked nodes.  CPU only.

(a) The argument, on the oracle alone: for every read that meets the predicate (tests/lane_exact_sub_worlds.py: from the oracle's
    seeds, mapping() and Graph.outgoing()), the oracle's result IS the closed form — score, CIGAR, nodes, spelling, num_matches.
(b) The host model at level 3 (MGX_EMU_LANE_EXACT=3), read by read against the oracle and against level 0; the reads with an
    alignment and no extension are exactly the three classes.
(c) The class is non-empty wherever a world is meant to have it.

Worlds: bench-like batches with a SNP window every 0 / 120 / 490 bp at k = 15 / 21 / 31 and read lengths from k + 2 to 256, both
strands; directed worlds for the mismatch position, two substitutions, indels, forks around the mismatch, a k-mer that exists
elsewhere, a later sub-k seed on the other allele, two SNPs less than k apart in the read's tail (a second alignment with one
mismatch), a tandem repeat, a homopolymer next to the read's end; the configurations of
lane_exact_sub_worlds.configurations().  The minimum class counts are what the oracle gives for these seeded worlds (in
brackets), less a margin."""
import pytest

import emu_drv
import lane_exact_sub_worlds as SW
from metagraph_amd import capi
from test_lane_read import bench_like_world

# name -> (seed, reads, k, world arguments, minimum number of reads of the substitution class)
BENCH = {
    "snp490_k31_L150": (31, 1500, 31, dict(genome_len=50000, read_len=150, snp_every=490), 250),     # [328]
    "snp120_k31_L100": (77, 800, 31, dict(genome_len=30000, read_len=100, snp_every=120), 120),      # [180]
    "snp0_k31_L64": (5, 800, 31, dict(genome_len=30000, read_len=64, snp_every=0), 50),              # [86]
    "snp490_k21_L256": (11, 400, 21, dict(genome_len=30000, read_len=256, snp_every=490, k=21), 30),
    "snp120_k15_L17": (12, 400, 15, dict(genome_len=20000, read_len=17, snp_every=120, k=15), 1),
    "snp0_k15_L40": (13, 400, 15, dict(genome_len=20000, read_len=40, snp_every=0, k=15), 30),
    "snp490_k21_L23": (14, 400, 21, dict(genome_len=20000, read_len=23, snp_every=490, k=21), 1),
}
_bench, _directed, _classes = {}, {}, {}


def bench(name):
    if name not in _bench:
        seed, n, k, kw, least = BENCH[name]
        _bench[name] = bench_like_world(seed, n, **kw)
    return _bench[name]


def directed(k):
    if k not in _directed:
        _directed[k] = SW.directed_world(k)
    return _directed[k]


def checked(key, g, cfg, reads):
    """the oracle against the closed form, once per world and configuration (shared by the tests below, never changed)"""
    if key not in _classes:
        _classes[key] = SW.check_closed_form(g, cfg, reads)
    return _classes[key]


# ---- (a), (c) the oracle alone ----
@pytest.mark.parametrize("name", list(BENCH))
def test_oracle_result_of_a_class_read_is_the_closed_form_on_bench_like_batches(name):
    g, reads = bench(name)
    k = BENCH[name][2]
    assert g.k == k
    c = checked(name, g, capi.config_cli(k), reads)
    print(name, "first class:", len(c.span), "path class:", len(c.path), "substitution class:", len(c.sub), "of", len(reads))
    assert len(c.sub) >= BENCH[name][4], (len(c.sub), BENCH[name][4])
    assert {s for s, _, _, _ in c.sub.values()} == {0, 1} or len(c.sub) < 4            # both strands


CONFIGS = ["cli", "no_end_bonus", "ti_tv", "xdrop_below_mismatch", "min_path_at_class", "min_path_above_class", "max_nodes_at_edge",
           "max_nodes_above_edge", "max_ram_at_edge", "max_ram_below_edge"]


def mismatch_at(rows, c, name):
    q = [r[0] for r in rows].index(name)
    return c.sub[q][1] if q in c.sub else None


@pytest.mark.parametrize("cname", CONFIGS)
@pytest.mark.parametrize("k", [15, 21, 31])
def test_oracle_on_directed_worlds(k, cname):
    g, rows = directed(k)
    reads = [r[1] for r in rows]
    cfg = SW.configurations(k, 100)[cname]
    c = checked(("directed", k, cname), g, cfg, reads)
    got = {rows[q][0]: ("sub" if q in c.sub else "out") for q in range(len(rows))}
    print(k, cname, got)
    L100 = {rows[q][0] for q in range(len(rows)) if len(rows[q][1]) == 100}
    if cname in ("cli", "ti_tv", "min_path_at_class", "max_nodes_above_edge", "max_ram_at_edge"):
        for name, r, kind in rows:
            if kind is not None and (cname in ("cli", "ti_tv") or name in L100):
                assert got[name] == kind, (name, kind, got[name])
    if cname == "cli":
        # the mismatch positions the world was made for: p = k (lo = 1), the last interior one, the tail up to the last character
        for p in (k, 100 - k - 1, 100 - 2, 100 - 1):
            assert mismatch_at(rows, c, "p_%d" % p) == p
        # ... and the second of two substitutions, an indel, a fork at the mismatch and a shorter run keep a read out
        for name in ("two_k_apart", "two_k1_apart", "two_close", "two_tail_k_apart", "two_tail_close", "two_tail_hidden", "insertion",
                     "deletion", "fork_node_at_p_minus_1", "kmer_elsewhere", "p_first_k", "p_0"):
            assert got[name] == "out" and got[name + "_rc"] == "out", name
        q = [r[0] for r in rows].index("kmer_elsewhere")
        zeros = [v == 0 for v in c.nodes[q][0]]
        assert 0 < sum(zeros) < k
        q = [r[0] for r in rows].index("insertion")
        assert sum(v == 0 for v in c.nodes[q][0]) == k                     # (k zeros, as a substitution: the walk turns it away)
        q = [r[0] for r in rows].index("deletion")
        assert sum(v == 0 for v in c.nodes[q][0]) == k - 1
        # forks inside the walked stretch are no obstacle
        for name in ("fork_node_at_p_plus_1", "bubble_in_walk_mid", "fork3_in_walk", "merge_inside_walk", "fork_right_before_p"):
            assert got[name] == "sub", name
        # the tandem repeat's walk meets nodes the read met before
        q = [r[0] for r in rows].index("tandem")
        assert q in c.sub and len(set(c.sub[q][3])) < len(c.sub[q][3])
    elif cname == "no_end_bonus":
        # without end bonuses a mismatch at the last character scores below stopping in front of it: out by strictness
        assert got["p_99"] == "out" and got["p_98"] == "out" and got["p_mid"] == "sub"
    elif cname == "xdrop_below_mismatch":
        assert not c.sub
    elif cname in ("min_path_above_class", "max_nodes_at_edge", "max_ram_below_edge"):
        assert not any(got[name] == "sub" for name in L100)
        # the edges are set for reads of 100 characters: (4 L + 1) / L falls with L, the table's bytes grow with it
        if cname == "max_nodes_at_edge":
            assert got["L_256"] == "sub" and got["L_65"] == "out"
        elif cname == "max_ram_below_edge":
            assert got["L_65"] == "sub" and got["L_256"] == "out"


def test_a_later_seed_on_the_other_allele_keeps_a_read_out():
    g, reads, cfg = SW.later_seed_world()
    c = checked("later", g, cfg, reads)
    sf, sr = c.run.seeds(0), c.run.seeds(1)
    why = []
    for q, r in enumerate(reads):
        if q not in c.sub:
            SW.classify(g, cfg, r, sf[q], sr[q], c.nodes[q], why)
    print("class reads:", len(c.sub), "of", len(reads), "; turned away by a later seed:", len(why))
    assert why and c.sub
    # ... and class reads carry sub-k seeds (offset > 0) that do lie on the walked path
    assert any(sd["offset"] for q in c.sub for sd in (sr if c.sub[q][0] else sf)[q][0])


_recomb = {}


def recombinant(k):
    if k not in _recomb:
        _recomb[k] = SW.recombinant_world(k)
    return _recomb[k]


@pytest.mark.parametrize("cname", ["cli", "ti_tv"])
@pytest.mark.parametrize("k", [21, 31])
def test_two_snps_less_than_k_apart_in_the_tail_keep_a_read_out(k, cname):
    """a read that recombines two SNPs d < k apart has two alignments with one mismatch each when the second SNP lies in its last k
    characters (every k-mer that covers it covers the first as well): equal scores with the CLI's matrix, the OTHER one better with
    transitions at -2 and transversions at -3 for some pairs — out of the class"""
    g, rows = recombinant(k)
    reads = [r[1] for r in rows]
    cfg = SW.configurations(k, 100)[cname]
    c = checked(("recomb", k, cname), g, cfg, reads)
    want = c.run.results()
    n_other = 0
    for q, (name, r, kind) in enumerate(rows):
        if kind == "out":
            assert q not in c.sub, name
            # ... and the oracle's alignment has one mismatch, not always at the position the zeros name
            assert want[q] and want[q][0]["num_matches"] == 99, (name, want[q])
            p = int(name.split("_p")[1])
            n_other += want[q][0]["cigar"] != ("%d=1X%d=" % (p, 99 - p) if p < 99 else "99=1X")
    print(k, cname, "tail reads whose oracle alignment has its mismatch elsewhere:", n_other)
    if cname == "ti_tv":
        assert n_other > 0
    # in the interior the k-mers that cover p and begin behind the first SNP are the other haplotype's nodes: a run shorter than k
    for q, (name, r, kind) in enumerate(rows):
        if name.endswith("_p60"):
            assert q not in c.sub and 0 < sum(v == 0 for v in c.nodes[q][0]) < k, name


# ---- (b) the host model ----
def run_model(g, cfg, reads, level, monkeypatch):
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")
    monkeypatch.setenv("MGX_EMU_LANE_EXACT", str(level))
    r = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads)
    assert r.error == "", r.error
    got, status = r.results()
    assert all(s == 0 for s in status), status
    assert r.lane_stats()[0]
    info = r.seed_info()
    return r, got, {q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0}


def check_model(c, g, cfg, reads, monkeypatch):
    want = c.run.results()
    every = set(c.span) | set(c.path) | set(c.sub)
    r3, got3, exact3 = run_model(g, cfg, reads, 3, monkeypatch)
    for q in range(len(reads)):
        assert got3[q] == want[q], (q, reads[q], got3[q], want[q])
    assert exact3 == every, sorted(exact3 ^ every)
    reasons3 = r3.lane_reasons()
    assert all(reasons3[q] == 0 for q in every)
    r0, got0, exact0 = run_model(g, cfg, reads, 0, monkeypatch)
    assert got0 == got3 and not exact0
    reasons0 = r0.lane_reasons()
    assert all(reasons3[q] == reasons0[q] for q in range(len(reads)) if q not in every)
    assert r3.lane_stats()[1] == r0.lane_stats()[1] + sum(1 for q in every if reasons0[q])


@pytest.mark.parametrize("name", list(BENCH))
def test_host_model_at_level_3_equals_the_oracle_and_level_0_on_bench_like_batches(name, monkeypatch):
    g, reads = bench(name)
    cfg = capi.config_cli(BENCH[name][2])
    check_model(checked(name, g, cfg, reads), g, cfg, reads, monkeypatch)


@pytest.mark.parametrize("cname", CONFIGS)
@pytest.mark.parametrize("k", [15, 21, 31])
def test_host_model_at_level_3_on_directed_worlds(k, cname, monkeypatch):
    g, rows = directed(k)
    reads = [r[1] for r in rows]
    cfg = SW.configurations(k, 100)[cname]
    check_model(checked(("directed", k, cname), g, cfg, reads), g, cfg, reads, monkeypatch)


def test_host_model_at_level_3_with_a_later_seed_on_the_other_allele(monkeypatch):
    g, reads, cfg = SW.later_seed_world()
    check_model(checked("later", g, cfg, reads), g, cfg, reads, monkeypatch)


@pytest.mark.parametrize("cname", ["cli", "ti_tv"])
@pytest.mark.parametrize("k", [21, 31])
def test_host_model_at_level_3_with_two_snps_less_than_k_apart(k, cname, monkeypatch):
    g, rows = recombinant(k)
    reads = [r[1] for r in rows]
    cfg = SW.configurations(k, 100)[cname]
    check_model(checked(("recomb", k, cname), g, cfg, reads), g, cfg, reads, monkeypatch)


def test_host_model_level_2_leaves_the_substitution_class_to_the_dp(monkeypatch):
    g, rows = directed(21)
    reads = [r[1] for r in rows]
    cfg = capi.config_cli(21)
    c = checked(("directed", 21, "cli"), g, cfg, reads)
    _, got, exact2 = run_model(g, cfg, reads, 2, monkeypatch)
    assert exact2 == set(c.span) | set(c.path) and c.sub and got == c.run.results()
