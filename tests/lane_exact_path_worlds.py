"""Worlds and the predicate for the PATH class of the lane extender's exact exit (level 2; metagraph_amd/csrc/lane_read.hpp
lane_exact_class(); TEST INFRASTRUCTURE).  A read is in the path class when the header tests of the exit hold (tests/
lane_exact_worlds.py class_strand(), all but the first seed's length), the first seed of the strand aligned first has clipping 0
and offset 0, every k-mer of that strand is a node, and the first seed does NOT span the query (then the read is in the first
class, which keeps its own counter).  The result is the same closed form, over the strand's mapped nodes.  Everything here is
evaluated from the ORACLE's seeds and mapping() and a plain-Python restatement of the conditions, never from the code under test."""
import collections
import random

import lane_cases as lc
import lane_exact_worlds as W
import orc
from test_emu_vs_oracle import rand_seq, rc


def classify(cfg, k, read, seeds_fwd, seeds_rc, nodes):
    """-> (kind, strand): kind 'span' (first seed spans the query: lane_exact_worlds.class_strand), 'path' or None.
    seeds_*: orc.AlignRun.seeds(strand)[q]; nodes: orc.AlignRun.mapping()[q] = (nodes of the forward strand, of the other)"""
    L = len(read)
    if not W.config_allows(cfg) or L < k or L > W.LANE_MAX_L:
        return None, None
    (s0, nm0), (s1, nm1) = seeds_fwd, seeds_rc
    both = bool(cfg.forward_and_reverse_complement)
    first = 0 if nm0 >= nm1 else 1
    s = first if both else 0
    if both:
        m_first, m_second = (nm1, nm0) if first else (nm0, nm1)
        n_second = len(s0) if first else len(s1)
        if float(m_second) >= float(m_first) * cfg.rel_score_cutoff and n_second > 0:
            return None, None                # a second strand to align
    mine = s1 if s else s0
    if not mine:
        return None, None
    sd = mine[0]
    if not (sd["clipping"] == 0 and sd["offset"] == 0):
        return None, None
    if W.full_score(cfg, L) < cfg.min_path_score or W.full_score(cfg, L) < cfg.min_cell_score:
        return None, None
    if sd["length"] == L:
        return "span", s
    mapped = nodes[s]
    assert len(mapped) == L - k + 1, (len(mapped), L, k)
    if any(v == 0 for v in mapped):
        return None, None
    return "path", s


Classes = collections.namedtuple("Classes", "span path run nodes num_matching")


def classes(g, cfg, reads, o=None):
    """-> Classes: span / path {read index: strand}, the oracle run, its mapping, {read: num_matching of its strand}"""
    o = o or orc.AlignRun(g, cfg, reads, threads=8, validate=False)
    assert o.error == "", o.error
    sf, sr, mp = o.seeds(0), o.seeds(1), o.mapping()
    span, path, nm = {}, {}, {}
    for q, r in enumerate(reads):
        kind, s = classify(cfg, g.k, r, sf[q], sr[q], mp[q])
        if kind == "span":
            span[q] = s
        elif kind == "path":
            path[q] = s
        if kind:
            nm[q] = (sr if s else sf)[q][1]
    # the first class as its own module states it: the two restatements agree
    assert span == W.class_reads(g, cfg, reads, o)[0]
    return Classes(span, path, o, mp, nm)


def closed_form(cfg, read, strand, mapped):
    L = len(read)
    return [{"score": W.full_score(cfg, L), "offset": 0, "clipping": 0, "end_clipping": 0, "num_matches": L,
             "nodes": list(mapped), "cigar": "%d=" % L, "sequence": rc(read) if strand else read, "orientation": strand}]


def check_closed_form(g, cfg, reads):
    """every read's oracle result, in either class, is the closed form over its strand's mapped nodes -> Classes"""
    c = classes(g, cfg, reads)
    want = c.run.results()
    for cls in (c.span, c.path):
        for q, s in cls.items():
            assert want[q] == closed_form(cfg, reads[q], s, c.nodes[q][s]), (q, reads[q], want[q])
    return c


# ---- directed worlds: a random genome with bubbles, multi-way forks, a tip, a tandem repeat, a low-complexity stretch ----
# A SNP at p with another allele in the graph: the FORK node is the k-mer that ends at p - 1 (it starts at p - k), the MERGE node
# the k-mer that starts at p + 1.  A read G[a : a + L] has the k-mers that start at a .. a + L - k.
SNP = 400                    # one bubble, nothing else within 160 characters
BUBBLES3 = (800, 830, 861)   # three bubbles one read crosses
FORK3, FORK4 = 1200, 1500    # three and four alleles
TIP = 1800                   # the other branch is a dead end: five characters, no merge
POLY = 2100                  # 26 x A: DUST masks the MEM a read begins with here
POLY_SNP = POLY + 26 + 40
TWIN = (2500, 2700)          # this segment's reverse complement is in the graph too
UNIT = 37                    # a tandem repeat of 4 units is appended behind the genome, a SNP in front of it


def dust_config(k):
    """the k-mer seeder with the complexity filter: seeds inside a homopolymer are dropped"""
    from metagraph_amd import capi
    c = capi.config_cli(k)
    c.max_seed_length = k
    c.seed_complexity_filter = 1
    return c


def _other(c, avoid=""):
    return next(x for x in "TGCA" if x != c and x not in avoid)


def directed_world(k, seed=4100):
    """-> (graph, [(group name, read, expected kind with the CLI's configuration: 'path', 'out' (in neither class) or None for
    "whatever the oracle's seeds say")])"""
    rng = random.Random(seed + k)
    G = list(rand_seq(rng, 3000))
    G[POLY:POLY + 26] = "A" * 26
    G = "".join(G)
    unit = rand_seq(rng, UNIT)
    T0 = len(G) + 60                                     # where the repeat begins
    G = G + rand_seq(rng, 60) + unit * 4 + rand_seq(rng, 200)
    TSNP = T0 - 20                                       # a bubble in front of the repeat

    def allele(p, alt):
        return G[p - k + 1:p] + alt + G[p + 1:p + k]

    seqs = [G, allele(SNP, _other(G[SNP])), allele(POLY_SNP, _other(G[POLY_SNP])), allele(TSNP, _other(G[TSNP]))]
    seqs += [allele(p, _other(G[p])) for p in BUBBLES3]
    a1 = _other(G[FORK3])
    seqs += [allele(FORK3, a1), allele(FORK3, _other(G[FORK3], a1))]
    seqs += [allele(FORK4, x) for x in "ACGT" if x != G[FORK4]]
    seqs.append(G[TIP - k + 1:TIP] + _other(G[TIP]) + rand_seq(rng, 5))
    seqs.append(rc(G[TWIN[0]:TWIN[1]]))
    g = orc.Graph.build(k, seqs, 0, False)
    rows = []

    def add(name, a, L, kind="path", both=True):
        r = G[a:a + L]
        assert len(r) == L
        rows.append((name, r, kind))
        if both:
            rows.append((name + "_rc", rc(r), kind))        # (on the other strand the fork is a merge and the merge a fork)

    p = SNP

    def at_snp(name, a, L):
        # the first seed must end at the fork node where that is a k-mer of the read other than its last: the path class
        add(name, a, L, "path" if 0 <= p - k - a < L - k else None)

    for L in (40, 97, 150):
        # the fork node: the read's first k-mer / its last k-mer (the read ends in front of the SNP) / one node past the read's end
        at_snp("fork_first_%d" % L, p - k, L)
        at_snp("fork_last_%d" % L, p - L, L)
        at_snp("fork_past_end_%d" % L, p - L - 1, L)
        # the merge node: first k-mer (the read begins behind the SNP) / last k-mer / one node past the end
        at_snp("merge_first_%d" % L, p + 1, L)
        at_snp("merge_last_%d" % L, p + 1 + k - L, L)
        at_snp("merge_past_end_%d" % L, p + k - L, L)
        at_snp("bubble_inside_%d" % L, p - L // 2, L)
    add("three_bubbles", BUBBLES3[0] - 30, 130)
    add("fork3", FORK3 - 50, 100)
    add("fork4", FORK4 - 50, 100)
    add("tip", TIP - 50, 100)
    add("tandem_with_fork", TSNP - 25, 150)                  # (20 + 25 characters, then 105 of the repeat: its nodes met again)
    # L = k and L = k + 1 at the fork and at the merge: a read of k characters is one k-mer (a seed that spans it), one of k + 1
    # whose two k-mers are the fork node and its child is split by the seeder only if the MEM ends between them
    for L in (k, k + 1):
        add("fork_L%d" % L, p - k, L, None)
        add("merge_L%d" % L, p + 1 - (L - k), L, None)
    # perfect but for the first / the last character: a zero at index 0 / L - k of the node array
    base = G[p - 50:p + 50]
    rows.append(("first_kmer_missing", _other(base[0]) + base[1:], "out"))
    rows.append(("last_kmer_missing", base[:-1] + _other(base[-1]), "out"))
    rows.append(("first_kmer_missing_rc", rc(_other(base[0]) + base[1:]), "out"))
    rows.append(("last_kmer_missing_rc", rc(base[:-1] + _other(base[-1])), "out"))
    # Reads that begin in / run across the 26 x A, then cross a bubble.  The MEM seeder does not filter (aligner_seeder_methods.cpp:
    # only the k-mer seeder :84 and the sub-k seeder :226, :300 call sdust), so with the CLI's configuration they are path-class
    # reads; with max_seed_length = k (DUST_CONFIG below) the seeds in the homopolymer are dropped: the first read's first seed
    # has clipping > 0 (out of the class), the second keeps its first seed and loses later ones (in the class, num_matching < L)
    add("dust_first_mem", POLY + 2, 110, "path", both=False)
    add("dust_middle_mem", POLY - 40, 140, "path", both=False)
    # a segment on both strands, crossed with nothing: the second-strand rule
    add("twin", TWIN[0] + 20, 100, "out")
    # and reads that are not perfect, without seeds, shorter than k
    rows.append(("substitution", base[:60] + _other(base[60]) + base[61:], "out"))
    rows.append(("random", rand_seq(rng, 100), "out"))
    rows.append(("short", G[p - 5:p + k - 6], "out"))
    return g, rows


# ---- the GPU batches: the mixed shapes of tests/lane_cases.py (its main world has bubbles, a three-way fork and a segment on both
# strands), every ninth read replaced by a random one ----
def mixed_batch(n):
    """-> (case, reads, expected hand-over codes with the exit off)"""
    c = lc.CASES["shape_%d" % n]() if "shape_%d" % n in lc.CASES else lc.shape_n(n)
    rng = random.Random(900 + n)
    reads, expected = list(c.reads), list(c.expected)
    for i in range(8, n, 9):
        reads[i], expected[i] = rand_seq(rng, 100), 0
    return c, reads, expected


def histogram(codes):
    return {k: v for k, v in collections.Counter(codes).items() if k}
