"""Worlds, the predicate and the closed form for the SUBSTITUTION class of the lane extender's exact exit (level 3; metagraph_amd/
csrc/lane_read.hpp lane_exact_sub(), lane_types.hpp lane_exact_sub_config(); TEST INFRASTRUCTURE).  A read is in the class when
the header tests of the exit hold (tests/lane_exact_path_worlds.py classify(), all but the node scan), the strand's node array has
exactly one run of zeros behind its first entry — k entries, or up to k that reach the array's end —, the graph walk across the run
succeeds, every later seed ends on the walked path, and the per-read conditions of the proof hold (DESIGN.md 3.4 "the substitution
class").  The result is the alignment with one mismatch over the mapped and the walked nodes.  Everything here is evaluated from
the ORACLE's seeds, mapping() and Graph.outgoing() and a plain-Python restatement of the conditions, never from the code under
test."""
import collections
import random

import lane_exact_path_worlds as PW
import lane_exact_worlds as W
import orc
from test_emu_vs_oracle import rand_seq, rc

ACGT = "ACGT"


def off_diagonal(cfg):
    v = [cfg.score_matrix[ord(a)][ord(b)] for a in ACGT for b in ACGT if a != b]
    return min(v), max(v)


def config_allows(cfg):
    """lane_exact_sub_config() on top of lane_exact_worlds.config_allows()"""
    if not W.config_allows(cfg):
        return False
    m = cfg.score_matrix[ord("A")][ord("A")]
    lo, hi = off_diagonal(cfg)
    return cfg.gap_opening_penalty + m < lo and 2 * hi - lo < m and hi - lo < m and lo + cfg.xdrop >= 0


def zero_run(mapped, k):
    """the one run of zeros (lo, hi) of the node array if it has the class's shape, else None"""
    z = [i for i, v in enumerate(mapped) if v == 0]
    if not z or z != list(range(z[0], z[-1] + 1)):
        return None
    lo, hi = z[0], z[-1]
    n = hi - lo + 1
    if lo < 1 or n > k or (hi != len(mapped) - 1 and n != k):
        return None
    return lo, hi


def children(g, v):
    return [(n, c) for n, c in g.outgoing(v) if c in ACGT]


def walk(g, k, strand_seq, mapped, lo, hi):
    """-> (graph character at p, walked nodes for [lo, hi]) or None"""
    p = lo + k - 1
    kids = children(g, mapped[lo - 1])
    if len(kids) != 1 or kids[0][1] == strand_seq[p]:
        return None
    cur, gch = kids[0]
    nodes = [cur]
    for x in range(1, hi - lo + 1):
        nxt = [n for n, c in children(g, cur) if c == strand_seq[p + x]]
        if not nxt:
            return None
        cur = nxt[0]
        nodes.append(cur)
    if hi < len(mapped) - 1:
        nxt = [n for n, c in children(g, cur) if c == strand_seq[p + k]]
        if not nxt or nxt[0] != mapped[hi + 1]:
            return None
    # a run shorter than k (it reaches the array's end): every k-mer that covers p also covers the positions L - k .. p - 1, so a path
    # that leaves at a fork there and takes the other allele is a second alignment with one mismatch: no such fork
    L = len(strand_seq)
    for x in range(max(L - 2 * k, 0), lo - 1):
        if len(children(g, mapped[x])) != 1:
            return None
    return gch, nodes


def classify(g, cfg, read, seeds_fwd, seeds_rc, nodes, why=None):
    """-> None, or (strand, p, graph character, path nodes) of a read of the substitution class.  why: a list that receives the
    reason where a read whose walk succeeded is turned away by a later seed"""
    k = g.k
    L = len(read)
    if not config_allows(cfg) or L < k or L > W.LANE_MAX_L or any(c not in ACGT for c in read):
        return None
    (s0, nm0), (s1, nm1) = seeds_fwd, seeds_rc
    both = bool(cfg.forward_and_reverse_complement)
    first = 0 if nm0 >= nm1 else 1
    s = first if both else 0
    if both:
        m_first, m_second = (nm1, nm0) if first else (nm0, nm1)
        n_second = len(s0) if first else len(s1)
        if float(m_second) >= float(m_first) * cfg.rel_score_cutoff and n_second > 0:
            return None
    mine = s1 if s else s0
    if not mine or not (mine[0]["clipping"] == 0 and mine[0]["offset"] == 0) or mine[0]["length"] == L:
        return None
    mapped = nodes[s]
    run = zero_run(mapped, k)
    if run is None:
        return None
    lo, hi = run
    q = rc(read) if s else read
    w = walk(g, k, q, mapped, lo, hi)
    if w is None:
        return None
    gch, walked = w
    p = lo + k - 1
    m = cfg.score_matrix[ord("A")][ord("A")]
    mm = cfg.score_matrix[ord(gch)][ord(q[p])]
    lb, rb = cfg.left_end_bonus, cfg.right_end_bonus
    core = m * (L - 1) + mm + lb
    if core + rb < cfg.min_path_score or core + rb < cfg.min_cell_score:
        return None
    if not mm + m * (L - 1 - p) + rb > 0:
        return None
    if not (4 * L + 1) / L < cfg.max_nodes_per_seq_char:
        return None
    if not (4 * L + 1) * (272 + 24 * (L + 1)) / 1e6 <= cfg.max_ram_per_alignment:
        return None
    if core < int(float(m * p + lb) * cfg.rel_score_cutoff):
        return None
    path = list(mapped[:lo]) + walked + list(mapped[hi + 1:])
    for sd in mine[1:]:
        cl, ln, so = sd["clipping"], sd["length"], sd["offset"]
        lpos = ln + cl - 1
        lscore = ln * m + (lb if cl == 0 else 0) + (rb if L - cl - ln == 0 else 0)
        prefix = m * (lpos + 1) + lb + (mm - m if lpos >= p else 0) + (rb if lpos == L - 1 else 0)
        if prefix < lscore:
            return None
        x = lpos - k + 1
        if x < 0 or sd["nodes"][-1] != path[x]:
            if why is not None:
                why.append("later seed off the path")
            return None
    return s, p, gch, path


def class_score(cfg, L, gch, qch):
    return (cfg.score_matrix[ord("A")][ord("A")] * (L - 1) + cfg.score_matrix[ord(gch)][ord(qch)]
            + cfg.left_end_bonus + cfg.right_end_bonus)


def closed_form(cfg, read, strand, p, gch, path):
    L = len(read)
    q = rc(read) if strand else read
    cigar = ("%d=" % p) + "1X" + ("%d=" % (L - 1 - p) if p < L - 1 else "")
    return [{"score": class_score(cfg, L, gch, q[p]), "offset": 0, "clipping": 0, "end_clipping": 0, "num_matches": L - 1,
             "nodes": list(path), "cigar": cigar, "sequence": q[:p] + gch + q[p + 1:], "orientation": strand}]


Classes = collections.namedtuple("Classes", "span path sub run nodes")


def classes(g, cfg, reads, o=None):
    """-> Classes: span / path {read: strand} (lane_exact_path_worlds), sub {read: (strand, p, character, path)}, the oracle run"""
    c = PW.classes(g, cfg, reads, o)
    sf, sr, mp = c.run.seeds(0), c.run.seeds(1), c.nodes
    sub = {}
    for q, r in enumerate(reads):
        if q in c.span or q in c.path:
            continue
        got = classify(g, cfg, r, sf[q], sr[q], mp[q])
        if got:
            sub[q] = got
    return Classes(c.span, c.path, sub, c.run, mp)


def check_closed_form(g, cfg, reads):
    """every read of the substitution class has the closed form as its oracle result -> Classes"""
    c = classes(g, cfg, reads)
    want = c.run.results()
    for q, (s, p, gch, path) in c.sub.items():
        assert want[q] == closed_form(cfg, reads[q], s, p, gch, path), (q, reads[q], p, want[q], closed_form(cfg, reads[q], s, p, gch, path))
    return c


# ---- directed worlds ----
def _other(c, avoid=""):
    return next(x for x in "TGCA" if x != c and x not in avoid)


def _sub(r, i, avoid=""):
    return r[:i] + _other(r[i], avoid) + r[i + 1:]


SNP = 400            # a bubble (two alleles)
FORK3 = 700          # three alleles
POLY = 1000          # 12 x A
UNIT = 41            # a tandem repeat of 5 units behind the genome


def directed_world(k, seed=5200):
    """-> (graph, [(name, read, expected with the CLI's configuration: 'sub', 'out' (not in the substitution class) or None for
    "whatever the predicate says")]).  A read G[a : a + L] with a substitution at read position p."""
    rng = random.Random(seed + k)
    G = list(rand_seq(rng, 1600))
    G[POLY:POLY + 12] = "A" * 12
    G = "".join(G)
    unit = rand_seq(rng, UNIT)
    T0 = len(G) + 50
    G = G + rand_seq(rng, 50) + unit * 5 + rand_seq(rng, 150)
    dup = 1300                                            # G[dup : dup + k] with one substitution exists elsewhere (below)

    def allele(p, alt):
        return G[p - k + 1:p] + alt + G[p + 1:p + k]

    a3 = _other(G[FORK3])
    seqs = [G, allele(SNP, _other(G[SNP])), allele(FORK3, a3), allele(FORK3, _other(G[FORK3], a3))]
    dup_kmer = _sub(G[dup:dup + k], k // 2)
    seqs.append(rand_seq(rng, 40) + dup_kmer + rand_seq(rng, 40))
    g = orc.Graph.build(k, seqs, 0, False)
    rows = []

    def add(name, r, kind, both=True):
        rows.append((name, r, kind))
        if both:
            rows.append((name + "_rc", rc(r), None))

    L = 100
    a = 100
    base = G[a:a + L]
    # the mismatch position: p = k (lo = 1), the last interior one, the first of the tail, the last two characters; p < k is out
    # (a read whose matched characters — those covered by a k-mer that is a node — fall below min_exact_match loses its seeds)
    def seeded(L, p):
        return p + (L - 1 - p if L - 1 - p >= k else 0) >= 0.7 * L + 1

    for p in (k, L - k - 1, L - k, L - 2, L - 1):
        add("p_%d" % p, _sub(base, p), "sub" if seeded(L, p) else None)
    add("p_mid", _sub(base, 50), "sub")
    add("p_first_k", _sub(base, k - 1), "out")
    add("p_0", _sub(base, 0), "out")
    # two substitutions: exactly k apart, k + 1 apart, fewer than k apart, interior and in the tail
    add("two_k_apart", _sub(_sub(base, 30), 30 + k), "out")
    add("two_k1_apart", _sub(_sub(base, 30), 31 + k), "out")
    add("two_close", _sub(_sub(base, 40), 45), "out")
    add("two_tail_k_apart", _sub(_sub(base, L - k - 2), L - 2), "out")
    add("two_tail_close", _sub(_sub(base, L - 6), L - 2), "out")
    add("two_tail_hidden", _sub(_sub(base, L - k + 2), L - 3), "out")
    # an insertion (k zeros: the walk must fail), a deletion (k - 1 zeros)
    add("insertion", base[:50] + _other(base[50], base[49]) + base[50:L - 1], "out")
    d = next(x for x in range(50, 70) if base[x] != base[x - 1] and base[x] != base[x + 1])    # (not in a run: exactly k - 1 zeros)
    add("deletion", base[:d] + base[d + 1:] + G[a + L], "out")
    # forks around the mismatch.  The fork node of the bubble at SNP is the k-mer that ends at SNP - 1.
    s = SNP
    # (read position x of G[s - c : s - c + 100] is genome position s - c + x)
    add("fork_node_at_p_minus_1", _sub(G[s - 50:s + 50], 50, avoid=_other(G[s])), "out")  # on the SNP site: v has two children
    add("merge_inside_walk", _sub(G[s - 48:s + 52], 50), None)                            # the mismatch two behind the SNP
    add("fork_right_before_p", _sub(G[s - 40:s + 60], 41), None)                          # the mismatch right behind the SNP
    add("fork_node_at_p_plus_1", _sub(G[s - 52:s + 48], 50), "sub")                       # the fork node ends at p + 1
    add("bubble_in_walk_mid", _sub(G[s - 60:s + 40], 60 - k // 2), "sub")                 # fork and SNP inside the walked stretch
    add("fork3_in_walk", _sub(G[FORK3 - 60:FORK3 + 40], 60 - k // 3), "sub")
    add("fork3_far", _sub(G[FORK3 - 20:FORK3 + 80], 70), "sub")
    # the substituted k-mer exists elsewhere in the graph: the run is shorter than k
    r = G[dup - 40:dup + 60]
    add("kmer_elsewhere", r[:40] + dup_kmer + r[40 + k:], "out")
    # low complexity: a substitution inside / next to the homopolymer; two and three characters from the read's end
    add("homopolymer_mid", _sub(G[POLY - 60:POLY + 40], 66), None)
    add("homopolymer_end2", _sub(G[POLY + 10 - L:POLY + 10], L - 2), None)
    add("homopolymer_end3", _sub(G[POLY + 10 - L:POLY + 10], L - 3), None)
    add("homopolymer_end2_plain", _sub(G[POLY + 12 - L:POLY + 12], L - 2), None)
    # a tandem repeat: the walk meets nodes the read has met before
    add("tandem", _sub(G[T0 + 5:T0 + 5 + 150], 100), None)
    add("tandem_first_unit", _sub(G[T0 - 30:T0 + 120], 60), None)
    # read lengths at the edges: L = k + 2 (p = k only, tail), the longest read
    add("L_k_plus_2", _sub(G[a:a + k + 2], k), None)
    add("L_256", _sub(G[a:a + 256], 130), "sub")
    add("L_64", _sub(G[a:a + 64], 40), "sub" if seeded(64, 40) else None)
    add("L_65", _sub(G[a:a + 65], 33), "sub")
    # and reads of the other classes, reads without seeds
    add("perfect", base, "out")
    add("perfect_fork", G[s - 50:s + 50], "out")
    rows.append(("random", rand_seq(rng, 100), "out"))
    return g, rows


def recombinant_world(k, seed=5400):
    """two SNPs d < k apart, the graph holding the haplotypes X a U b Y and X a' U b' Y only; reads of 100 characters that carry
    a at the first and b' at the second — one substitution against either haplotype, two alignments with one mismatch each — with
    the second SNP at read position p in the last k characters (a tail run: all k-mers that cover p are missing) and in the interior
    (there the k-mers that begin behind the first SNP are the other haplotype's nodes: a shorter run).
    -> (graph, [(name, read, 'out' where the read must not be in the class, else None)])"""
    rng = random.Random(seed + k)
    G = rand_seq(rng, 1400)
    rows = []
    seqs = [G]
    at = 300
    for d in (5, 6, 7, k - 1):
        for p in (94, 96, 97, 98, 99, 60):
            s2 = at + 150                      # the second SNP; the first one d in front of it
            s1 = s2 - d
            a1, b1 = _other(G[s1]), _other(G[s2])
            seqs.append(G[s1 - k + 1:s1] + a1 + G[s1 + 1:s2] + b1 + G[s2 + 1:s2 + k])
            r = G[s2 - p:s2 - p + 100]
            r = r[:p] + b1 + r[p + 1:]         # hap1 up to the second SNP, hap2's character there
            tail = p > 100 - k
            rows.append(("recomb_d%d_p%d" % (d, p), r, "out" if tail else None))
            rows.append(("recomb_d%d_p%d_rc" % (d, p), rc(r), None))
            at += 250
            if at + 400 > len(G):
                G2 = rand_seq(rng, 1400)
                seqs.append(G2)
                G, at = G2, 300
    return orc.Graph.build(k, seqs, 0, False), rows


def later_seed_world(k=21, seed=5300):
    """a read with one substitution whose later sub-k seed lies on the OTHER allele's node behind a bubble: hand-over code 19 of
    the DP, out of the class.  -> (graph, reads, config): the sub-k seeder is on (min_seed_length < k)"""
    from metagraph_amd import capi
    rng = random.Random(seed)
    G = rand_seq(rng, 1200)
    s = 600
    alt = _other(G[s])
    g = orc.Graph.build(k, [G, G[s - k + 1:s] + alt + G[s + 1:s + k]], 0, False)
    cfg = capi.config_cli(k)
    cfg.min_seed_length = k - 6
    reads = []
    for d in range(2, k):
        r = G[s - 70:s + 30]
        reads.append(_sub(r, 70 - d))                    # a substitution d in front of the SNP
        reads.append(_sub(r, 70 + d))                    # ... and behind it
        ra = r[:70] + alt + r[71:]
        reads.append(_sub(ra, 70 - d))
        reads.append(_sub(ra, 70 + d))
    return g, reads, cfg


def configurations(k, L, gch_score=None):
    """name -> config; the per-read edges are set for reads of L characters"""
    from metagraph_amd import capi
    out = {}
    out["cli"] = capi.config_cli(k)
    c = capi.config_cli(k); c.left_end_bonus = 0; c.right_end_bonus = 0
    out["no_end_bonus"] = c
    c = capi.config_cli(k)
    for a in ACGT:
        for b in ACGT:
            if a != b:
                transition = {a, b} in ({"A", "G"}, {"C", "T"})
                c.score_matrix[ord(a)][ord(b)] = -2 if transition else -3
    out["ti_tv"] = c
    c = capi.config_cli(k); c.xdrop = 2
    out["xdrop_below_mismatch"] = c
    mm = off_diagonal(capi.config_cli(k))[0]
    full = W.full_score(capi.config_cli(k), L)
    m = capi.config_cli(k).score_matrix[ord("A")][ord("A")]
    c = capi.config_cli(k); c.min_path_score = full - m + mm
    out["min_path_at_class"] = c
    c = capi.config_cli(k); c.min_path_score = full - m + mm + 1
    out["min_path_above_class"] = c
    c = capi.config_cli(k); c.max_nodes_per_seq_char = (4 * L + 1) / L
    out["max_nodes_at_edge"] = c
    c = capi.config_cli(k); c.max_nodes_per_seq_char = (4 * L + 2) / L
    out["max_nodes_above_edge"] = c
    c = capi.config_cli(k); c.max_ram_per_alignment = (4 * L + 1) * (272 + 24 * (L + 1)) / 1e6
    out["max_ram_at_edge"] = c
    c = capi.config_cli(k); c.max_ram_per_alignment = (4 * L + 1) * (272 + 24 * (L + 1) - 1) / 1e6
    out["max_ram_below_edge"] = c
    return out
