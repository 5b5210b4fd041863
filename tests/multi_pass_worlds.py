"""Worlds for the multi-pass extension (extend_multi_pass in mgx.hip, the MGX_EMU_MULTIPASS loop of the host model), shared by
tests/test_multi_pass_emu.py (CPU) and tests/test_gpu_multi_pass.py.  TEST INFRASTRUCTURE ONLY.

A pass of the multi-pass extension extends a limited number of seeds per read: 1 in passes 0 - 7, 4 in passes 8 - 15, 16 in
passes 16 - 23, and pass 24 has no limit (multi_pass_seed_limit, host_common.hpp).  A read therefore meets the limit of 4 only
with more than 8 extensions, the limit of 16 with more than 8 + 8 * 4 = 40, and the unlimited pass with more than
40 + 8 * 16 = 168.  Ordinary reads extend a handful of seeds; the `deep` world is a repeat family whose reads extend hundreds:

  genome   COPIES diverged copies (DIVERGENCE substitutions) of one random UNIT-mer, each followed by SPACER random bases
  reads    `repeat`: n copies of the unit end to end, mutated — n = 4 gives more than 168 extensions, fewer copies and shorter
           pieces the ranges below; `exact`: a window of the genome; `sub1`: a window with one substitution; `chimera`: two
           distant windows glued together; `edge`: "", a read shorter than k, a read of N's

with sub-k seeds (min_seed_length 7 at k = 15) and no cap on the seeds of a locus.  Everything is deterministic from the seed.
The expectation of every world is the oracle's result list; tests/test_multi_pass_emu.py asserts the extension counts per read
(the buckets) on the host model's seed info, so that a change of the generator that empties one fails there."""
import functools
import random

import orc
from metagraph_amd import capi
from test_emu_vs_oracle import make_world, rand_seq, rc

K = 15
UNIT, SPACER, COPIES, DIVERGENCE = 60, 20, 300, 0.12
READ_DIVERGENCE = 0.15
PRIMARY = 2

# extensions per read -> the last kind of pass it meets: the buckets of the precondition test
BUCKETS = (("unlimited", 169, 1 << 30), ("limit16", 41, 168), ("limit4", 9, 40), ("limit1", 2, 8), ("one_pass", 0, 1))
N_PASSES_DEEP = 25            # passes 0 .. 24: what a batch with a read of more than 168 extensions runs, and no batch runs more


# deep under this max_columns: some reads run out of columns in a pass after their first.  Found with the host model: which limit
# binds depends on the lanes per read (a column's record is as wide as the group).  With 8 lanes, the extension kernel's geometry,
# no read runs out at 1400; at 1200 two dozen do, most of them in pass 0 and three after some hundred extensions; with 64 lanes
# two dozen as well, one of them after ten extensions.
LATE_CAPACITY_MAX_COLUMNS = 1200


def alt_limits(n_alt):
    """deep with four alignments per read: one repeat read needs more columns than the default limit gives, multi-pass or
    not (the product's capacity retry doubles the limits for such a read); the worlds here are about the passes"""
    if n_alt < 4:
        return None
    lim = capi.Limits()
    lim.max_columns = 16000
    return lim


def bucket_of(n_extensions):
    for name, lo, hi in BUCKETS:
        if lo <= n_extensions <= hi:
            return name
    raise ValueError(n_extensions)


def substitute(rng, s, rate):
    return "".join(rng.choice([c for c in "ACGT" if c != ch]) if rng.random() < rate else ch for ch in s)


class World:
    """name, k, graph mode, the sequences the graph is built from, the reads, and per read its kind"""

    def __init__(self, name, k, mode, seqs, reads, kinds, sub_k=True):
        self.name, self.k, self.mode, self.seqs, self.reads, self.kinds, self.sub_k = name, k, mode, seqs, list(reads), list(kinds), sub_k
        self._g = None

    @property
    def g(self):
        if self._g is None:
            self._g = orc.Graph.build(self.k, self.seqs, self.mode, False)
        return self._g

    def config(self, n_alt=1):
        cfg = capi.config_cli(self.k)
        cfg.min_exact_match = 0.0
        if self.sub_k:
            cfg.min_seed_length = 7
            cfg.max_num_seeds_per_locus = 100000
        cfg.num_alternative_paths = n_alt
        return cfg

    def repeat_reads(self):
        return [i for i, kind in enumerate(self.kinds) if kind == "repeat"]


def _deep_parts(seed=2024):
    rng = random.Random(seed)
    unit = rand_seq(rng, UNIT)
    genome = "".join(substitute(rng, unit, DIVERGENCE) + rand_seq(rng, SPACER) for _ in range(COPIES))
    reads, kinds = [], []
    # repeat reads: 24 of four copies, then shorter ones for the ranges between a handful and 168 extensions
    for n_units, count in ((4, 24), (2, 6), (1, 8)):
        for _ in range(count):
            reads.append(substitute(rng, unit * n_units, READ_DIVERGENCE))
            kinds.append("repeat")
    for length, count in ((45, 6), (30, 6), (24, 6)):
        for _ in range(count):
            p = rng.randrange(0, UNIT - length + 1)
            reads.append(substitute(rng, unit[p:p + length], READ_DIVERGENCE / 2))
            kinds.append("repeat")
    # companions that need few extensions: they retire in the early passes
    def window(n):
        p = rng.randrange(0, len(genome) - n)
        return genome[p:p + n]
    for _ in range(8):
        reads.append(window(100))
        kinds.append("exact")
    for _ in range(8):
        r = window(100)
        p = rng.randrange(20, 80)
        reads.append(r[:p] + rng.choice([c for c in "ACGT" if c != r[p]]) + r[p + 1:])
        kinds.append("sub1")
    for _ in range(8):
        reads.append(window(50) + window(50))
        kinds.append("chimera")
    for r in ("", "ACGTACGTAC", "N" * 40):
        reads.append(r)
        kinds.append("edge")
    return genome, reads, kinds


@functools.lru_cache(maxsize=None)
def deep():
    genome, reads, kinds = _deep_parts()
    return World("deep", K, 0, [genome], reads, kinds)


@functools.lru_cache(maxsize=None)
def deep_primary():
    """deep's genome as a PRIMARY graph (one of each k-mer and its reverse complement, behind the CanonicalDBG wrapper), every
    other read reverse-complemented: seeds of both strands through the wrapper, the _prim build of the extension kernel"""
    from test_oracle_primary_goldens import primary_contigs
    genome, reads, kinds = _deep_parts()
    reads = [rc(r) if i % 2 else r for i, r in enumerate(reads)]
    return World("deep_primary", K, PRIMARY, primary_contigs([genome], K)[0], reads, kinds)


@functools.lru_cache(maxsize=None)
def shallow():
    """an ordinary world: every read needs at most 2 extensions (asserted by the precondition test)"""
    g, reads = make_world(4242, K, genome_len=4000, n_reads=48, read_len=100, n_variants=0)
    w = World("shallow", K, 0, None, reads, ["plain"] * len(reads), sub_k=False)
    w._g = g
    return w


WORLDS = {"deep": deep, "deep_primary": deep_primary, "shallow": shallow}
# (deep_alt is deep under config(n_alt) with n_alt = 2 and 4)


@functools.lru_cache(maxsize=None)
def oracle(name, n_alt=1):
    """the expectation: the oracle's alignment lists of world `name` with num_alternative_paths = n_alt, computed once"""
    w = WORLDS[name]()
    o = orc.AlignRun(w.g, w.config(n_alt), w.reads)
    assert o.error == "", o.error
    return o.results()


def cut(reads, length=120):
    return [r[:length] for r in reads]
