#!/usr/bin/env python3
"""Directed fuzzing of the substitution class of the lane extender's exact exit (level 3) on the CPU: worlds with
two haplotypes whose SNPs lie a few characters apart (closer than k), reads that recombine the haplotypes and carry substitutions
of their own, the CLI's scores and matrices that score substitutions differently.  Per world: the oracle's result of every read of
the class (tests/lane_exact_sub_worlds.py: the predicate from the oracle's seeds, mapping() and Graph.outgoing()) against the
closed form, the host model at MGX_EMU_LANE_EXACT=3 against the oracle read by read, and the reads the model finished without an
extension against the three classes.  Stops at the first difference.
    python tools/fuzz_exact_sub.py [--minutes M] [--seed S]"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def world(rng):
    import orc
    from test_emu_vs_oracle import rand_seq, rc
    k = rng.choice([15, 21, 31])
    n = rng.randrange(1500, 4000)
    h1 = rand_seq(rng, n)
    h2 = list(h1)
    p = k + rng.randrange(20)
    while p < n - k:
        h2[p] = rng.choice([c for c in "ACGT" if c != h1[p]])
        p += rng.choice([2, 3, 5, 7, k - 1, k, k + 1, 2 * k, 60, 200]) if rng.random() < 0.7 else rng.randrange(1, 300)
    h2 = "".join(h2)
    g = orc.Graph.build(k, [h1, h2], 0, False)
    reads = []
    for _ in range(rng.randrange(100, 300)):
        L = rng.choice([k + 2, 2 * k - 1, 2 * k, 64, 100, 150, rng.randrange(k + 2, 257)])
        a = rng.randrange(0, n - L)
        cur, out = rng.randrange(2), []
        for i in range(a, a + L):
            if rng.random() < 0.03:
                cur ^= 1                                             # recombine
            out.append((h1, h2)[cur][i])
        for _ in range(rng.choice([0, 1, 1, 1, 2])):
            i = rng.randrange(L)
            out[i] = rng.choice([c for c in "ACGT" if c != out[i]])
        r = "".join(out)
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return g, reads


def config(rng, k):
    from metagraph_amd import capi
    c = capi.config_cli(k)
    kind = rng.randrange(4)
    if kind:
        for a in "ACGT":
            for b in "ACGT":
                if a != b:
                    ti = {a, b} in ({"A", "G"}, {"C", "T"})
                    c.score_matrix[ord(a)][ord(b)] = (-2 if ti else -3) if kind == 1 else (-1 if ti else -2) if kind == 2 else -rng.randrange(1, 4)
    if rng.random() < 0.2:
        c.left_end_bonus = c.right_end_bonus = 0
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    os.environ["MGX_EMU_SPLIT"] = "1"
    os.environ["MGX_EMU_LANE"] = "1"
    os.environ["MGX_EMU_LANE_EXACT"] = "3"
    import emu_drv
    import lane_exact_sub_worlds as SW
    t0 = time.time()
    worlds = n_reads = n_sub = n_other = n_cfg_ok = 0
    while time.time() - t0 < args.minutes * 60:
        rng = random.Random(args.seed * 100003 + worlds)
        g, reads = world(rng)
        cfg = config(rng, g.k)
        c = SW.check_closed_form(g, cfg, reads)
        want = c.run.results()
        r = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads)
        assert r.error == "", r.error
        got, status = r.results()
        info = r.seed_info()
        for q in range(len(reads)):
            if got[q] != want[q]:
                sys.exit("DIFFERENCE: seed %d world %d read %d %s\n  model  %s\n  oracle %s" % (args.seed, worlds, q, reads[q], got[q], want[q]))
        every = set(c.span) | set(c.path) | set(c.sub)
        exact = {q for q in range(len(reads)) if got[q] and info[q]["n_extensions"] == 0}
        if r.lane_stats()[0] and exact != every:
            sys.exit("CLASSES DIFFER: seed %d world %d reads %s" % (args.seed, worlds, sorted(exact ^ every)))
        worlds += 1
        n_reads += len(reads)
        n_sub += len(c.sub)
        n_other += len(c.span) + len(c.path)
        n_cfg_ok += SW.config_allows(cfg)
    print("ok: %d worlds (%d with a configuration level 3 accepts), %d reads, %d in the substitution class, %d in the two perfect classes, "
          "no difference" % (worlds, n_cfg_ok, n_reads, n_sub, n_other))


if __name__ == "__main__":
    main()
