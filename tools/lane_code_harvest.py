#!/usr/bin/env python3
"""Which LANE_BAIL codes (metagraph_amd/csrc/lane_read.hpp) do undirected reads reach in the host model?  The search behind the
"NOT REACHED" entries of the table in tests/lane_cases.py: random reads of that module's main world (substitutions, insertions,
deletions, junk at either end) under nine configurations, then reads that end 0 .. K characters before or behind every SNP and
fork of the world (the tie-mode sites of code 27).  Prints the reads per code and configuration and, at the end, the codes seen.
CPU only (tests/emu); run from the repository root: python tools/lane_code_harvest.py [seed]"""
import collections
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["MGX_EMU_SPLIT"] = "1"
os.environ["MGX_EMU_LANE"] = "1"

import emu_drv  # noqa: E402
import lane_cases as lc  # noqa: E402
from test_emu_vs_oracle import mutate, rand_seq  # noqa: E402

CONFIGS = {
    "cli": {},
    "left_trim_off": dict(allow_left_trim=0),
    "xdrop_45": dict(xdrop=45),
    "no_end_bonus": dict(left_end_bonus=0, right_end_bonus=0),
    "sub_k": dict(min_seed_length=12, min_exact_match=0.0),
    "min_exact_match_0": dict(min_exact_match=0.0),
    "forward_only": dict(forward_and_reverse_complement=0, min_exact_match=0.0),
    "min_path_score_150": dict(min_path_score=150),
    "min_cell_score_-10": dict(min_cell_score=-10),
}
SHAPES = ((100, .03, .01, .01, 0), (60, .06, .0, .0, 15), (150, .02, .03, .03, 30), (40, .05, .02, .02, 10))   # L, sub, ins, del, junk


def main():
    rng = random.Random(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    g, G = lc.main_world()
    eg = emu_drv.EmuGraph(g)
    seen = collections.Counter()

    def run(tag, cfg, reads):
        e = emu_drv.EmuRun(eg, cfg, reads)
        assert e.error == "", e.error
        cnt = collections.Counter(e.lane_reasons())
        seen.update(cnt)
        print(tag, dict(sorted(cnt.items())))

    for name, kw in CONFIGS.items():
        for L, sub, ins, dele, junk in SHAPES:
            reads = []
            for i in range(300):
                p = rng.randrange(0, len(G) - L - 20)
                r = mutate(rng, G[p:p + L], sub=sub, ins=ins, dele=dele)
                if junk and i % 3 == 0:
                    r = rand_seq(rng, rng.randrange(1, junk)) + r
                if junk and i % 3 == 1:
                    r = r + rand_seq(rng, rng.randrange(1, junk))
                reads.append(r[:250])
            run("%s L=%d" % (name, L), lc.cli(**kw), reads)
    # reads that end around a fork: ties beyond the query's end, columns that stayed behind and are revived after them
    forks = lc.SNPS_ALT_FIRST + lc.SNPS_ALT_LAST + [lc.SNP_TIE, lc.FORK3]
    for name, kw in (("cli", {}), ("no_end_bonus", dict(left_end_bonus=0, right_end_bonus=0)), ("xdrop_45", dict(xdrop=45)),
                     ("nodes_per_char_1.1", dict(max_nodes_per_seq_char=1.1)), ("rel_score_cutoff_0.5", dict(rel_score_cutoff=0.5))):
        reads = []
        for p in forks:
            for d in range(-lc.K, lc.K + 1):
                for L in (60, 100):
                    r = G[p + d - L:p + d]
                    reads += [r, lc._sub(r, L - 3), lc._sub(r, L - 8)]
        run("fork ends, %s" % name, lc.cli(**kw), reads)
    print("codes seen:", sorted(k for k in seen if k), "reads:", sum(seen.values()))


if __name__ == "__main__":
    main()
