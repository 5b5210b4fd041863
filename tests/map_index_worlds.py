"""The worlds of the mapping-kernel tests (tests/test_gpu_map_index_edges.py on the GPU, tests/test_map_index_edges_model.py
through the host model): graphs, reads and the node arrays a plain k-mer dictionary (tests/kmer_dict.py) expects for them.
Every check takes a `backend` with two methods: graph(k, W, last, F, valid=None, mode=0) puts a BOSS table where the kernels
under test read it, check(G, k, reads, want, machine, forward_only) maps `reads` with one mapping machine and compares the node
arrays with `want`.  TEST INFRASTRUCTURE ONLY."""
import functools
import random

import numpy as np

import kmer_dict
import orc
from test_emu_vs_oracle import mutate, rand_seq, rc

BYTE_PATH_KS = [33, 40, 63]                     # k > 32: BASIC node arrays straight from k_map
MACHINES = ("map_pipe=0", "map_pipe=2")         # one chain step per lane and iteration / request-response (k <= 32)
BYTE_PATH = ("byte",)                           # k > 32: k_map, whatever map_pipe says


def machines_of(k):
    return MACHINES if k <= 32 else BYTE_PATH


def first_difference(got, want, reads):
    for q, (g, w) in enumerate(zip(got, want)):
        if g != w:
            for s in (0, 1):
                for i, (a, b) in enumerate(zip(g[s], w[s])):
                    if a != b:
                        return "read %d (%d bytes) strand %d k-mer %d: %d, dictionary %d: %r" % (q, len(reads[q]), s, i, a, b, reads[q][:200])
            return "read %d: %d / %d k-mers, dictionary %d / %d" % (q, len(g[0]), len(g[1]), len(w[0]), len(w[1]))
    return "%d reads, dictionary %d" % (len(got), len(want))


# ---------------------------------------------------------------------------------------------------------------------------
# a. edge-count residues and single-block graphs
# ---------------------------------------------------------------------------------------------------------------------------
def grow_until(k, accept, start_len, seed, n_variants=0):
    """lengthen a random genome one base at a time until the graph's edge count is accepted -> (oracle graph, sequences)"""
    for attempt in range(40):
        rng = random.Random(1000 * seed + attempt)
        genome = rand_seq(rng, start_len + 400)
        variants = []
        for _ in range(n_variants):
            p = rng.randrange(k, start_len - k)
            alt = rng.choice([c for c in "ACGT" if c != genome[p]])
            variants.append(genome[p - k + 1:p] + alt + genome[p + 1:p + k])
        for L in range(start_len, start_len + 400):
            seqs = [genome[:L]] + variants
            g = orc.Graph.build(k, seqs, 0, True)
            if accept(g.n_edges):
                return g, seqs
    raise AssertionError("no genome with the wanted edge count (k = %d)" % k)


def mask_with_block_edges(rng, valid, n):
    """the oracle's dummy mask thinned at random, with the slots 0 and 63 of the blocks alternately masked out and kept"""
    v = np.array(valid, dtype=np.uint8)
    v[1:] &= (np.array([rng.random() < 0.7 for _ in range(n)], dtype=np.uint8))
    for j, e in enumerate(range(63, n + 1, 64)):
        v[e] = j & 1                                 # slot 63 of block j
        if e + 1 <= n:
            v[e + 1] = (j >> 1) & 1                  # slot 0 of block j + 1
    return v


def reads_over_the_last_edges(rng, d, seqs, k, n, n_last=130):
    """every window of the sequences that touches the k-mer of one of the last n_last edges, and a mutated sample"""
    reads = []
    for s in seqs:
        ids, _, _ = d.lookup(kmer_dict.encode(s))
        for p in np.flatnonzero(ids > n - n_last):
            lo = max(0, int(p) - rng.randrange(0, 40))
            r = s[lo:int(p) + k + rng.randrange(0, 40)]
            reads.append(rc(r) if rng.random() < 0.3 else r)
    genome = seqs[0]
    for i in range(60):
        L = min(len(genome), rng.choice((k, k + 1, 40, 100, 150)))
        p = rng.randrange(0, len(genome) - L + 1)
        r = mutate(rng, genome[p:p + L])
        if i % 2:
            r = rc(r)
        if i % 7 == 3 and r:
            r = r[:len(r) // 2] + "N" + r[len(r) // 2 + 1:]
        reads.append(r if i % 10 != 9 else rand_seq(rng, L))
    return reads + ["", "A", genome[:k - 1], genome[-k:], genome]


def check_world(backend, g, seqs, k, seed, want_block_edge_masks):
    rng = random.Random(seed)
    W, last, F, valid = g.export()
    n = g.n_edges
    plain = kmer_dict.KmerDict(k, W, last, F)
    reads = reads_over_the_last_edges(rng, plain, seqs, k, n)
    mask = mask_with_block_edges(rng, valid, n)
    if want_block_edge_masks:
        for slot in (0, 63):
            at = [e for e in range(1, n + 1) if e % 64 == slot]
            assert any(mask[e] for e in at) and any(not mask[e] for e in at), "slot %d: not both masked out and kept" % slot
    for v in (None, mask):
        d = plain if v is None else kmer_dict.KmerDict(k, W, last, F, v)
        want = kmer_dict.map_reads(d, reads)
        assert sum(1 for f, _ in want for x in f if x) > (50 if n > 64 else 3)
        if v is None and n > 200:
            assert len({x for f, r in want for x in f + r if x > n - 130}) > 60, "the last edges are not mapped to"
        G = backend.graph(k, W, last, F, v)
        for machine in machines_of(k):
            backend.check(G, k, reads, want, machine)


def edge_count_residues(backend, k, residue):
    """(n_edges + 1) mod 64 = 0 (the final block exactly full), 1 (one slot in it), 2 and 63: the clips of the last block in
    incoming / succ_W_code, mask_upto, the `i > n` cut of the block build, the valid and first-character packers"""
    # (k = 3: the graph saturates near 4^3 edges, so the genome starts short and the residues are reached on the way up)
    g, seqs = grow_until(k, lambda n: (n + 1) % 64 == residue and n >= 62, 8 if k == 3 else 2000, 7 * k + residue, 0 if k == 3 else 6)
    assert (g.n_edges + 1) % 64 == residue
    check_world(backend, g, seqs, k, 31 * k + residue, want_block_edge_masks=g.n_edges >= 256)


def single_block_graphs(backend, k, full):
    """one 64-byte block is the whole index: n_edges < 64, and n_edges + 1 == 64 exactly.  (k = 63 has no such graph: the
    root edge, the 62 sentinel-prefixed edges in front of a sequence's first k-mer, one k-mer and its sink are 65 edges.)"""
    g, seqs = grow_until(k, (lambda n: n == 63) if full else (lambda n: 20 <= n < 60), k + 1, 500 + k, 0)
    assert (g.n_edges + 1 == 64) if full else (g.n_edges < 64)
    check_world(backend, g, seqs, k, 77 * k + full, want_block_edge_masks=False)


# ---------------------------------------------------------------------------------------------------------------------------
# b. read lengths and invalid characters around the 32-base words of the packed reads
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packing_world(k):
    rng = random.Random(900 + k)
    genome = rand_seq(rng, 3000)
    g = orc.Graph.build(k, [genome], 0, False)
    W, last, F, _ = g.export()
    d = kmer_dict.KmerDict(k, W, last, F)
    reads = []
    other = 0
    for L in range(0, 131):
        p0 = (37 * L) % (len(genome) - 131)
        base = genome[p0:p0 + L]
        reads.append(base)
        for pos in sorted({0, k - 1, 31, 32, 63, 64, 95, 96, L - k, L - 1}):
            if not 0 <= pos < L:
                continue
            reads.append(base[:pos] + "N" + base[pos + 1:])
            # in another copy: lower case (inside the alphabet: the same nodes), or a byte outside it
            ch = (base[pos].lower(), "x", "\xff", "-", "n", "\x00")[other % 6]
            other += 1
            reads.append(base[:pos] + ch + base[pos + 1:])
    want = kmer_dict.map_reads(d, reads)
    return (W, last, F), reads, want


def read_lengths_and_invalid_characters_at_word_edges(backend, k):
    """pack_read_word, packed_advance and kmask: one read of every length 0 .. 130, alone and with one N / lower-case /
    non-ACGT byte at 0, k - 1, 31, 32, 63, 64, 95, 96, L - k and L - 1, both strands and forward only; in one batch and in
    batches of 1, 63, 64, 65 and 257 reads (a lane's chain fetch crosses wavefront and workgroup edges).  k = 33, 40, 63: the
    byte path, as the control."""
    (W, last, F), reads, want = packing_world(k)
    assert len(reads) > 1500 and sum(1 for f, _ in want for x in f if x) > 20000
    G = backend.graph(k, W, last, F)
    for machine in machines_of(k):
        backend.check(G, k, reads, want, machine)
        for size, first, step in ((1, 1234, 1), (63, 5, 23), (64, 900, 1), (65, 17, 19), (257, 3, 5)):
            pick = list(range(first, len(reads), step))[:size]
            assert len(pick) == size
            backend.check(G, k, [reads[i] for i in pick], [want[i] for i in pick], machine)


# ---------------------------------------------------------------------------------------------------------------------------
# c. the index at size: select-anchor shifts 7 and 8
# ---------------------------------------------------------------------------------------------------------------------------
SEL_ANCHOR_MAX = 8192            # MGX_SEL_ANCHOR_MAX (kernel_units.hpp): entries of the select-anchor table k_map_pipe copies to LDS


def sel_anchor_shift(total_last):
    # graph_build.hpp: the smallest shift >= 6 with (total_last >> shift) + 2 <= 8192 entries, so the shift leaves 6 at
    # total_last >> 6 = 8191, i.e. from 8191 * 64 = 524 224 set `last` bits on, and 7 from 8191 * 128 = 1 048 448 on
    s = 6
    while (total_last >> s) + 2 > SEL_ANCHOR_MAX:
        s += 1
    return s


# genome lengths: SHIFT7 / SHIFT8 give the two shifts; SPAN0 was found offline (the lengths 540 000 +- 200 searched) as one
# whose graph has a number of nodes that is a multiple of 128 = 2^shift: no rank lies in the last anchor segment (the
# `span == 0` branch of build_sel_anchor)
BIG = {"shift7": 540000, "shift8": 1050000, "span0": 539957}
K_BIG = 31


def big_arrays(genome_len, n_snps=2000):
    """synth.build_boss of a random genome and SNP windows (numpy's MT19937 streams: the same table on every machine)"""
    import torch
    from metagraph_amd import synth
    rs = np.random.RandomState(20240917)
    genome = rs.randint(0, 4, genome_len).astype(np.uint8)
    pos = np.random.RandomState(7).randint(K_BIG - 1, 500000 - K_BIG, n_snps)
    win = genome[pos[:, None] + np.arange(-(K_BIG - 1), K_BIG)[None, :]].copy()
    win[:, K_BIG - 1] = (win[:, K_BIG - 1] + 1 + (pos % 3).astype(np.uint8)) % 4
    b = synth.build_boss([torch.from_numpy(genome)[None, :], torch.from_numpy(win)], K_BIG)
    return genome, b["W"].numpy(), b["last"].numpy(), b["F"]


@functools.lru_cache(maxsize=None)
def big_world(name):
    import torch
    from metagraph_amd import synth
    genome, W, last, F = big_arrays(BIG[name])
    d = kmer_dict.KmerDict(K_BIG, W, last, F)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[genome].tobytes().decode()
    rng = random.Random(len(genome))
    sample = synth.sample_reads(torch.from_numpy(genome), 4000, 150, 11).numpy()
    reads = [row.tobytes().decode() for row in sample]
    n = len(text)
    for lo, hi in ((n - 2000, n), (0, 2000)):
        for i in range(200):
            L = rng.choice((31, 32, 64, 100, 150))
            p = rng.randrange(lo, hi - L + 1)
            r = text[p:p + L]
            reads.append(rc(r) if i % 2 else r)
    reads += [text[n - L:] for L in (31, 32, 33, 64, 150)] + [rc(text[n - 150:])]          # ... ending in the final k-mer
    reads += [rand_seq(rng, 150) for _ in range(50)]
    for i in range(100):
        r = reads[37 * i]
        p = rng.randrange(len(r))
        reads.append(r[:p] + "N" + r[p + 1:])
    want = kmer_dict.map_reads(d, reads)
    return (W, last, F), text, reads, want


def check_big(backend, name, machine, want_shift):
    (W, last, F), text, reads, want = big_world(name)
    total_last = int(last[1:].sum())
    assert sel_anchor_shift(total_last) == want_shift, total_last
    n = len(W) - 1
    found = [x for f, r in want for x in f + r if x]
    assert len(found) > 150000 and max(found) > 0.99 * n and min(found) < 0.01 * n
    backend.check(backend.graph(K_BIG, W, last, F), K_BIG, reads, want, machine, forward_only=False)
    return total_last


class ArrayGraph:
    """what emu_drv.EmuGraph takes of an oracle graph, over plain arrays"""

    def __init__(self, k, W, last, F):
        self.k, self.arrays = k, (W, last, np.asarray(F, dtype=np.uint64), None)

    def export(self):
        return self.arrays


# ---------------------------------------------------------------------------------------------------------------------------
# d. PRIMARY graphs: the node arrays after k_canon_merge
# ---------------------------------------------------------------------------------------------------------------------------
def primary_node_arrays(backend, k, mask):
    """canon_merge_pair: a k-mer found forward keeps its id, its mirror image is id + n unless the k-mer is a palindrome
    (even k); one found only as reverse complement is id + n forward.  Even k: palindromic k-mers are planted in the genome
    and read on both strands."""
    from test_oracle_canonical_wrapper import PRIMARY
    from test_oracle_primary_goldens import primary_contigs
    assert PRIMARY == kmer_dict.PRIMARY
    rng = random.Random(4000 + k)
    half = rand_seq(rng, k // 2)
    palindromes = [] if k % 2 else [("ACGT" * k)[:k] if k % 4 == 0 else half + rc(half), half + rc(half), rc(half) + half]
    for p in palindromes:
        assert p == rc(p) and len(p) == k
    genome = rand_seq(rng, 700)
    for p in palindromes:
        genome += p + rand_seq(rng, 300)
    seqs = [genome]
    for _ in range(10):
        p = rng.randrange(k, len(genome) - k)
        alt = rng.choice([c for c in "ACGT" if c != genome[p]])
        seqs.append(genome[p - k + 1:p] + alt + genome[p + 1:p + k])
    g = orc.Graph.build(k, primary_contigs(seqs, k, "input")[0], PRIMARY, mask)
    W, last, F, valid = g.export()
    n = g.n_edges
    d = kmer_dict.KmerDict(k, W, last, F, valid)
    reads = []
    for i in range(80):
        L = rng.choice((k, k + 1, 64, 100, 150))
        p = rng.randrange(0, len(genome) - L)
        r = genome[p:p + L] if i % 3 else mutate(rng, genome[p:p + L])
        if i % 2:
            r = rc(r)
        if i % 11 == 5:
            r = r[:len(r) // 2] + "N" + r[len(r) // 2 + 1:]
        reads.append(r)
    for p in palindromes:
        at = genome.index(p)
        across = genome[at - 40:at + k + 40]
        reads += [p, across, rc(across), across[:40 + k], rc(across)[:40 + k]]
    reads += ["", "ACG", rand_seq(rng, 100)]
    want = kmer_dict.map_reads(d, reads, kmer_dict.PRIMARY)
    assert any(x > n for f, _ in want for x in f), "no k-mer found only as its reverse complement"
    if palindromes:
        n_pal = sum(1 for f, r in want for i, x in enumerate(f) if x and r[len(f) - 1 - i] == x)
        assert n_pal >= len(palindromes), "no palindromic k-mer was mapped"
    G = backend.graph(k, W, last, F, valid, mode=PRIMARY)
    for machine in machines_of(k):
        backend.check(G, k, reads, want, machine, forward_only=False)
