"""Worlds, the predicate and the closed form for the lane extender's exact exit (metagraph_amd/csrc/lane_read.hpp lane_exact(),
lane_types.hpp lane_exact_config(); TEST INFRASTRUCTURE).  A read is in the class when the first seed of the strand aligned first
spans the query; its result is then the all-match alignment over the seed's nodes.  Everything here is evaluated from the ORACLE's
seeds and a plain-Python restatement of the conditions, never from the code under test."""
import random

import orc
from metagraph_amd import capi
from test_emu_vs_oracle import rand_seq, rc
from test_lane_read import bench_like_world

LANE_MAX_L = 256


def config_allows(cfg):
    """lane_enabled() and lane_exact_config() for a BASIC graph without labels: the configurations in which the exit is exact"""
    acgt = [ord(c) for c in "ACGT"]
    m = cfg.score_matrix[acgt[0]][acgt[0]]
    if cfg.num_alternative_paths != 1 or cfg.post_chain_alignments or m <= 0:
        return False
    for a in acgt:
        for b in acgt:
            v = cfg.score_matrix[a][b]
            if (a == b and v != m) or (a != b and v >= m):
                return False
    return (cfg.gap_opening_penalty < 0 and cfg.gap_extension_penalty <= 0 and cfg.left_end_bonus >= 0 and cfg.right_end_bonus >= 0
            and 0 <= cfg.xdrop <= 30000 and 0.0 <= cfg.rel_score_cutoff <= 1.0)


def full_score(cfg, L):
    return cfg.score_matrix[ord("A")][ord("A")] * L + cfg.left_end_bonus + cfg.right_end_bonus


def class_strand(cfg, k, read, seeds_fwd, seeds_rc):
    """the strand (0 / 1) on which `read` is in the class, else None.  seeds_*: orc.AlignRun.seeds(strand)[q] = (seed list, num_matching)"""
    L = len(read)
    if not config_allows(cfg) or L < k or L > LANE_MAX_L:
        return None
    (s0, nm0), (s1, nm1) = seeds_fwd, seeds_rc
    both = bool(cfg.forward_and_reverse_complement)
    first = 0 if nm0 >= nm1 else 1
    s = first if both else 0
    if both:
        m_first, m_second = (nm1, nm0) if first else (nm0, nm1)
        n_second = len(s0) if first else len(s1)
        if float(m_second) >= float(m_first) * cfg.rel_score_cutoff and n_second > 0:
            return None                      # a second strand to align
    mine = s1 if s else s0
    if not mine:
        return None
    sd = mine[0]
    if not (sd["clipping"] == 0 and sd["length"] == L and sd["offset"] == 0):
        return None
    if full_score(cfg, L) < cfg.min_path_score or full_score(cfg, L) < cfg.min_cell_score:
        return None
    return s


def closed_form(cfg, read, strand, seed):
    L = len(read)
    return [{"score": full_score(cfg, L), "offset": 0, "clipping": 0, "end_clipping": 0, "num_matches": L,
             "nodes": list(seed["nodes"]), "cigar": "%d=" % L, "sequence": rc(read) if strand else read, "orientation": strand}]


def class_reads(g, cfg, reads, o=None):
    """-> ({read index: strand}, the oracle run)"""
    o = o or orc.AlignRun(g, cfg, reads, threads=8, validate=False)
    assert o.error == "", o.error
    sf, sr = o.seeds(0), o.seeds(1)
    k = g.k
    out = {}
    for q, r in enumerate(reads):
        s = class_strand(cfg, k, r, sf[q], sr[q])
        if s is not None:
            out[q] = s
    return out, o


def check_closed_form(g, cfg, reads):
    """every class read's oracle result is the closed form -> number of class reads"""
    cls, o = class_reads(g, cfg, reads)
    want = o.results()
    seeds = (o.seeds(0), o.seeds(1))
    for q, s in cls.items():
        assert want[q] == closed_form(cfg, reads[q], s, seeds[s][q][0][0]), (q, reads[q], want[q])
    return len(cls)


# ---- worlds: (graph, reads); every one holds perfect reads, reads with errors and reads without seeds ----
def _cut(rng, G, n, L, sub=0.004):
    """n reads of length L cut from G: two thirds perfect, the rest with substitutions; a random strand"""
    out = []
    for i in range(n):
        p = rng.randrange(0, len(G) - L)
        r = G[p:p + L]
        if i % 3 == 2:
            r = "".join(rng.choice([b for b in "ACGT" if b != c]) if rng.random() < max(sub, 1.5 / L) else c for c in r)
        out.append(rc(r) if rng.random() < 0.5 else r)
    return out


def world_bench(n=600, seed=5):
    return bench_like_world(seed, n, snp_every=490)


def world_snp60(n=400, seed=6):
    """(seeds end where the graph forks, so a read must fit between two SNP windows to be in the class: 45-bp reads, k = 31)"""
    return bench_like_world(seed, n, genome_len=20000, read_len=45, snp_every=60)


def world_three_alleles(n=200, k=21, seed=7):
    """every 97th position carries all of two further alleles: three-way forks on the reads' paths"""
    rng = random.Random(seed)
    G = rand_seq(rng, 6000)
    seqs = [G]
    for p in range(k + 13, len(G) - k, 97):
        for alt in [c for c in "ACGT" if c != G[p]][:2]:
            seqs.append(G[p - k + 1:p] + alt + G[p + 1:p + k])
    g = orc.Graph.build(k, seqs, 0, False)
    reads = _cut(rng, G, n, 40)
    # ... and short reads that carry an alternative allele themselves
    for p in range(k + 13, 3000, 97 * 3):
        alt = [c for c in "ACGT" if c != G[p]][0]
        reads.append(G[p - 5:p] + alt + G[p + 1:p + 15])
    return g, reads


def world_tandem(n=120, k=15, seed=8):
    """a 45-bp unit repeated 8 times: the strand's k-mers are nodes, many of them several times along the read"""
    rng = random.Random(seed)
    unit = rand_seq(rng, 45)
    G = rand_seq(rng, 400) + unit * 8 + rand_seq(rng, 400)
    g = orc.Graph.build(k, [G], 0, False)
    reads = [G[p:p + 110] for p in range(300, 700, 400 // (n // 2))][:n // 2]
    reads += _cut(rng, G, n - len(reads), 110)
    return g, reads


def world_both_strands(n=120, k=21, seed=9):
    """a 300-bp segment and its reverse complement both in the genome: reads from it are perfect on both strands (never in the
    class: the second-strand rule), reads from elsewhere are as in any world"""
    rng = random.Random(seed)
    X = rand_seq(rng, 300)
    G = rand_seq(rng, 1500) + X + rand_seq(rng, 1500) + rc(X) + rand_seq(rng, 1500)
    g = orc.Graph.build(k, [G], 0, False)
    in_x = [G[1500 + p:1500 + p + 100] for p in range(0, 200, 5)]
    return g, in_x + _cut(rng, G[:1400], n - len(in_x), 100), len(in_x)


def world_lengths(k=21, seed=10):
    """perfect reads at the edges of the closed form's packing: L = k, k + 1, 32, 33, 64, 65, 150, 256 (the longest read the lane
    takes), on both strands, and what must stay out: an N in a read, L < k, a random read"""
    rng = random.Random(seed)
    G = rand_seq(rng, 5000)
    g = orc.Graph.build(k, [G], 0, False)
    reads = []
    for L in (k, k + 1, 32, 33, 64, 65, 150, 256):
        for _ in range(3):
            p = rng.randrange(0, len(G) - L)
            reads += [G[p:p + L], rc(G[p:p + L])]
    p = 1234
    with_n = G[p:p + 100]
    reads += [with_n[:50] + "N" + with_n[51:], G[p:p + k - 1], G[p:p + 5], rand_seq(rng, 100), ""]
    return g, reads


def configurations(k, L):
    """name -> (config, whether reads of length L can be in the class at all)"""
    out = {}
    out["cli"] = (capi.config_cli(k), True)
    c = capi.config_cli(k); c.left_end_bonus = 0; c.right_end_bonus = 0
    out["no_end_bonus"] = (c, True)
    c = capi.config_cli(k); c.rel_score_cutoff = 0.0
    out["rel0"] = (c, True)
    c = capi.config_cli(k); c.min_path_score = full_score(c, L)
    out["min_path_at_full"] = (c, True)
    c = capi.config_cli(k); c.min_path_score = full_score(c, L) + 1
    out["min_path_above_full"] = (c, False)
    c = capi.config_cli(k); c.max_seed_length = k
    out["max_seed_length_k"] = (c, False)
    return out
