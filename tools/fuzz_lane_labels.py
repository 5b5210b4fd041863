#!/usr/bin/env python3
"""Differential fuzzing of label-aware alignment on the lane-per-read path (lane_read.hpp, round 6) in the host model against the
oracle's LabeledAligner: segment-labelled worlds (tests/test_lane_labels.py::segment_world) with random k, read length, SNP
density, label count and configuration; alignments, label lists, the label filter's seed lists and num_matching of every read.
    python tools/fuzz_lane_labels.py N_WORLDS [FIRST_SEED]
With MGX_EMU_LANE_EXACT=1 / 2 / 3 in the environment the lane's exact exit is on at that level (lane_read.hpp lane_exact()); the
reads that left through it — an alignment and no extension — are counted.  At level 3 (the substitution class of label-aware reads)
those with a mismatch are also checked against the class's closed form and counted apart: one substitution behind the first k
characters, every other character matched, one label.
CPU only (test infrastructure)."""
import os, re, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MGX_EMU_SPLIT"] = "1"; os.environ["MGX_EMU_LANE"] = "1"
os.environ.setdefault("MGX_EMU_SEEDLANE", "1")          # (round 6: the lane-per-read seeder in front, one seed per k-mer)
import emu_drv, orc
from metagraph_amd import capi
from labeled_worlds import with_labels
from test_lane_labels import segment_world
from test_emu_vs_oracle import rc
tot = done_t = bad_t = sl_t = exact_t = sub_t = 0
LEVEL = os.environ.get("MGX_EMU_LANE_EXACT", "0")


def closed_form_of_a_substitution(k, read, alns):
    """whether a result finished without an extension whose CIGAR holds a mismatch has the shape of the substitution class's closed
    form (the oracle comparison above settles its content): p= 1X (L-1-p)= with p >= k, the path spelling equal to the strand
    everywhere but at p, L - k + 1 nodes, one label"""
    if len(alns) != 1:
        return False
    a = alns[0]
    L = len(read)
    m = re.fullmatch(r"(\d+)=1X(?:(\d+)=)?", a["cigar"])
    if not m:
        return False
    p, rest = int(m.group(1)), int(m.group(2) or 0)
    strand = rc(read) if a["orientation"] else read
    return (p >= k and p + 1 + rest == L == len(a["sequence"]) and [i for i in range(L) if a["sequence"][i] != strand[i]] == [p]
            and a["num_matches"] == L - 1 and a["clipping"] == 0 and a["end_clipping"] == 0 and a["offset"] == 0
            and len(a["nodes"]) == L - k + 1 and 0 not in a["nodes"] and len(a["labels"]) == 1)


first = int(sys.argv[2]) if len(sys.argv) > 2 else 100
for seed in range(first, first + int(sys.argv[1])):
    rng = random.Random(seed)
    k = rng.choice([11, 15, 21, 27, 31])
    g, anno, reads = segment_world(seed, k=k, genome_len=rng.choice([3000, 8000]), n_labels=rng.choice([1, 3, 8]), n_reads=120,
                                   read_len=rng.choice([60, 100, 150]), snp_every=rng.choice([0, 90, 200]) or 10**9, label_alt=bool(seed % 2))
    cfg = capi.config_cli(k)
    if seed % 5 == 0: cfg.min_seed_length = max(5, k - 6)
    if seed % 7 == 0: cfg.min_exact_match = 0.9
    if seed % 11 == 0: cfg.xdrop = 10
    o = orc.LabeledAlignRun(g, cfg, anno, reads)
    e = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads, annotation=emu_drv.EmuAnnotation(anno))
    assert e.error == "" and o.error == "", (e.error, o.error)
    got, status = e.results()
    want = with_labels(o)
    bad = [q for q in range(len(reads)) if got[q] != want[q] or status[q]]
    info = e.seed_info()
    for strand in (0, 1):
        for q, (ss, nm) in enumerate(o.seeds(strand)):
            if info[q]["num_matches"][strand] != nm or info[q]["seeds"][strand] != emu_drv.oracle_seeds_as_tuples(ss): bad.append(q)
    ran, nd = e.lane_stats()
    sl_t += e.seedlane_stats()[1]
    tot += len(reads); done_t += nd; bad_t += len(bad)
    if ran:
        exact = [q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0]
        exact_t += len(exact)
        for q in exact:
            if "X" in got[q][0]["cigar"]:
                sub_t += 1
                if LEVEL != "3" or not closed_form_of_a_substitution(k, reads[q], got[q]): bad.append(q)
    if bad: print("seed", seed, "k", k, "BAD", bad[:5])
print("worlds done: reads", tot, "seeded by the lane-per-read seeder", sl_t, "lane finished", done_t,
      "through the exact exit", exact_t, "of them in the substitution class", sub_t, "mismatches", bad_t)
