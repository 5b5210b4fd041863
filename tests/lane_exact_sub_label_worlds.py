"""Worlds, the predicate and the closed form for the SUBSTITUTION class of the lane extender's exact exit on LABEL-AWARE batches
(level 3; metagraph_amd/csrc/lane_read.hpp lane_exact_class<true>(), lane_exact_sub<true>(); DESIGN.md 3.4 "the substitution
class, label-aware"; TEST INFRASTRUCTURE).  A read of a label-aware batch is in the class when
  (1) the one-label seed filter passes (lane_exact_label_worlds.label_filter()) and leaves a label L;
  (2) the conditions of the unlabeled substitution class hold on what the filter left (lane_exact_sub_worlds.classify(): the strand
      choice, the first seed, the one run of zeros, the walk on the plain graph, the later seeds, the thresholds);
  (3) every node of the path — the mapped nodes outside the run and the walked ones — has the row exactly [L].
Its result is the closed form of the unlabeled class with the label list [L].  Everything here is evaluated from the ORACLE — the
seeds of its plain aligner, mapping(), Graph.outgoing(), Annotation.get_rows() — never from the code under test; the oracle's
LabeledAligner is the judge of the closed form."""
import collections
import random

import lane_exact_label_worlds as LW
import lane_exact_sub_worlds as SW
import orc
from test_emu_vs_oracle import mutate, rand_seq, rc

Classes = collections.namedtuple("Classes", "span path sub label run nodes filtered refused_row refused_walk refused_seed")


def classes(g, anno, cfg, reads):
    """-> Classes: span / path {read: strand} and their labels (lane_exact_label_worlds), sub {read: (strand, p, character, path)},
    label {read: L} for every class read, the LabeledAligner run, the plain mapping, filtered {read: ((seeds, nm), (seeds, nm))},
    and the reads turned away for: a row of the path alone, the walk alone (one run of zeros of the class's shape on a strand whose
    first seed is at the query's first character, the walk failing), a later seed off the path"""
    c = LW.classes(g, anno, cfg, reads)
    sf, sr, mp = c.plain.seeds(0), c.plain.seeds(1), c.nodes
    n_rows = g.n_edges
    cache = {}

    def row_of(node):
        if node not in cache:
            cache[node] = [int(x) for x in anno.get_rows([node - 1])[0]] if 0 < node <= n_rows else []
        return cache[node]

    sub, label, filtered = {}, dict(c.label), dict(c.filtered)
    refused_row, refused_walk, refused_seed = set(), set(), set()
    for q, r in enumerate(reads):
        if q in c.span or q in c.path:
            continue
        f = LW.label_filter(cfg, g.k, r, sf[q], sr[q], row_of)
        if f is None:
            continue
        lbl, f0, f1 = f
        why = []
        got = SW.classify(g, cfg, r, f0, f1, mp[q], why)
        if got is None:
            if why:
                refused_seed.add(q)
            else:
                for s, (seeds, _) in enumerate((f0, f1)):
                    if not seeds or not (seeds[0]["clipping"] == 0 and seeds[0]["offset"] == 0) or len(r) < g.k:
                        continue
                    run = SW.zero_run(mp[q][s], g.k)
                    if run and all(ch in "ACGT" for ch in r) and SW.walk(g, g.k, rc(r) if s else r, mp[q][s], run[0], run[1]) is None:
                        refused_walk.add(q)
            continue
        s, p, gch, path = got
        if any(row_of(v) != [lbl] for v in path):
            refused_row.add(q)
            continue
        sub[q] = got
        label[q] = lbl
        filtered[q] = (f0, f1)
    return Classes(c.span, c.path, sub, label, c.run, mp, filtered, refused_row, refused_walk, refused_seed)


def closed_form(cfg, read, strand, p, gch, path, label):
    out = SW.closed_form(cfg, read, strand, p, gch, path)
    out[0]["labels"] = [label]
    return out


def check_closed_form(g, anno, cfg, reads):
    """the oracle's LabeledAligner result of every read of the three classes is its closed form with the label list [L]
    -> (Classes, the oracle's results with label lists)"""
    from labeled_worlds import with_labels
    c = classes(g, anno, cfg, reads)
    want = with_labels(c.run)
    for cls in (c.span, c.path):
        for q, s in cls.items():
            assert want[q] == LW.closed_form(cfg, reads[q], s, c.nodes[q][s], c.label[q]), (q, reads[q], want[q])
    for q, (s, p, gch, path) in c.sub.items():
        cf = closed_form(cfg, reads[q], s, p, gch, path, c.label[q])
        assert want[q] == cf, (q, reads[q], p, want[q], cf)
    return c, want


# ---- the directed world ----
# A genome of 3400 characters; label 0 on its k-mers that start before BOUNDARY, label 1 on the others.  Inside label 0:
#  - three sites where the k k-mers that cover one genome position carry another label (2), two labels (0 and 2) or none, every other
#    node { 0 }: a read with a substitution there walks across them;
#  - four sites where ONE k-mer has the row { 0, 2 }: path node lo, hi, lo - 1, hi + 1 of the read with a substitution at the site;
#  - a bubble whose other allele carries label 0 as well (a SNP site, and the later-seed reads), two SNPs 6 apart with both
#    haplotypes labelled 0 (the recombinant), and, in label 1, the reverse complement of the first 80 characters of one read.
BOUNDARY = 2600
ROW_SITES = (("other", 300), ("two", 500), ("none", 700))
EDGE_SITES = (("lo", 900), ("hi", 1100), ("lo_minus_1", 1300), ("hi_plus_1", 1500))
SNP = 1750
RECOMB = 2050            # the second SNP; the first one RECOMB_D in front of it
RECOMB_D = 6
OTHER_STRAND = 2300      # the reverse complement of the 80 characters from here sits at PLANT, in label 1
PLANT = 3000
PLAIN = 2450             # nothing within 100 characters: the class reads


def _other(c, avoid=""):
    return next(x for x in "TGCA" if x != c and x not in avoid)


def _sub(r, i, avoid=""):
    return r[:i] + _other(r[i], avoid) + r[i + 1:]


def directed_world(k=21, seed=8100):
    """-> (graph, annotation, [(name, read, expected: 'sub', 'out' (not in the substitution class) or None = whatever the
    predicate says)]).  Reads of ~100 characters."""
    return _directed(k, seed)[:3]


FREE = ((1780, 1990), (2100, 2290))      # stretches of label 0 without a feature: further class reads and perfect reads


def free_read(i, L=100):
    """the i-th window of L characters from the stretches of FREE (genome coordinates)"""
    lo, hi = FREE[i % 2]
    return lo + (i * 7) % (hi - lo - L)


def genome(k=21, seed=8100):
    return _directed(k, seed)[3]


def _directed(k, seed):
    rng = random.Random(seed + k)
    G = list(rand_seq(rng, 3400))
    G[PLANT:PLANT + 80] = rc("".join(G[OTHER_STRAND:OTHER_STRAND + 80]))
    G = "".join(G)
    snp_alt = G[SNP - k + 1:SNP] + _other(G[SNP]) + G[SNP + 1:SNP + k]
    s2, s1 = RECOMB, RECOMB - RECOMB_D
    a1, b1 = _other(G[s1]), _other(G[s2])
    hap2 = G[s1 - k + 1:s1] + a1 + G[s1 + 1:s2] + b1 + G[s2 + 1:s2 + k]
    g = orc.Graph.build(k, [G, snp_alt, hap2], 0, False)
    anno = orc.Annotation(g, 3)
    # label 0 in pieces: the k-mers that cover a row site's position are left out where they are to carry another row
    at = 0
    for name, s in ROW_SITES:
        if name != "two":
            anno.annotate(G[at:s], 0)                    # (k-mers that end in front of s)
            at = s + 1
    anno.annotate(G[at:BOUNDARY + k - 1], 0)
    anno.annotate(G[BOUNDARY:], 1)
    for name, s in ROW_SITES:
        if name != "none":
            anno.annotate(G[s - k + 1:s + k], 2)
    for name, s in EDGE_SITES:
        x = {"lo": s - k + 1, "hi": s, "lo_minus_1": s - k, "hi_plus_1": s + 1}[name]
        anno.annotate(G[x:x + k], 2)
    anno.annotate(snp_alt, 0)
    anno.annotate(hap2, 0)
    rows = []

    def add(name, r, kind, kind_rc="same"):
        rows.append((name, r, kind))
        rows.append((name + "_rc", rc(r), kind if kind_rc == "same" else kind_rc))

    L = 100
    base = G[PLAIN:PLAIN + L]
    # (a) class reads: the mismatch interior, in the last k characters, at the last character; both strands
    for p in (k, 50, L - k - 1, L - k + 3, L - 2, L - 1):
        add("p_%d" % p, _sub(base, p), "sub")
    add("perfect", base, "out")
    # (b) the walked nodes carry another label, two labels, none
    for name, s in ROW_SITES:
        add("walk_row_%s" % name, _sub(G[s - 50:s + 50], 50), "out")
        add("walk_row_%s_tail" % name, _sub(G[s - 95:s + 5], 95), "out")
    # (c) one node of the path with the row { 0, 2 }: the first and last walked node, the mapped nodes on either side
    for name, s in EDGE_SITES:
        add("edge_%s" % name, _sub(G[s - 50:s + 50], 50), "out")
    # (d) across the label boundary: rows [0] then [1]
    add("boundary", _sub(G[BOUNDARY - 50:BOUNDARY + 50], 30), "out")
    add("label_1", _sub(G[BOUNDARY + 150:BOUNDARY + 250], 60), "sub")
    # (e) the OTHER strand has seeds too — 80 characters of it, enough for min_exact_match, too few for a second strand to align —
    # and their nodes carry label 1
    add("other_strand_label", _sub(G[OTHER_STRAND:OTHER_STRAND + L], 90), "out", None)
    # (f) a short read whose tail substitution leaves fewer than min_exact_match x L characters covered: no seeds, no alignment
    add("short_under_min_exact_match", _sub(G[PLAIN:PLAIN + 36], k), "out")
    # (g) what the unlabeled class turns away, labelled { 0 } all along
    add("insertion", base[:50] + _other(base[50], base[49]) + base[50:L - 1], "out")
    add("snp_site", _sub(G[SNP - 50:SNP + 50], 50, avoid=_other(G[SNP])), "out")
    add("two_k1_apart", _sub(_sub(base, 30), 31 + k), "out")
    add("two_close", _sub(_sub(base, 40), 45), "out")
    for p in (96, 98):
        r = G[s2 - p:s2 - p + L]
        add("recomb_p%d" % p, r[:p] + b1 + r[p + 1:], "out", None)
    # (h) a later sub-k seed on the other allele's node behind the bubble, and reads whose sub-k seeds lie on the path
    r = G[SNP - 70:SNP + 30]
    ra = r[:70] + _other(G[SNP]) + r[71:]
    for d in range(2, k):
        rows.append(("later_d%d_front" % d, _sub(r, 70 - d), None))
        rows.append(("later_d%d_behind" % d, _sub(r, 70 + d), None))
        rows.append(("later_alt_d%d_front" % d, _sub(ra, 70 - d), None))
        rows.append(("later_alt_d%d_behind" % d, _sub(ra, 70 + d), None))
    rows.append(("random", rand_seq(rng, 100), "out"))
    rows.append(("with_n", base[:30] + "N" + base[31:], "out"))
    return g, anno, rows, G


def later_seed_config(k):
    """the sub-k seeder reaches further down (as lane_exact_sub_worlds.later_seed_world)"""
    from metagraph_amd import capi
    cfg = capi.config_cli(k)
    cfg.min_seed_length = k - 6
    return cfg


# ---- random worlds: the benchmark's label-aware batch in small ----
def random_world(seed, k=31, genome_len=12000, n_labels=12, n_reads=360, read_len=100, snp_every=490, widen=15):
    """one label per genome segment, widened by `widen` positions into its neighbours, and unlabeled SNP alleles (as
    test_gpu_lane_exact_labels.segment_batch); reads: a third perfect, a third with one substitution behind the first k characters,
    the others in turn with the benchmark's error model, with one insertion, ending inside a widened border with a substitution in
    their last k characters (walked nodes with two labels), through a SNP's other allele with a substitution next to it (walked
    nodes without a label) -> (graph, annotation, reads)"""
    rng = random.Random(seed * 977 + k)
    G = rand_seq(rng, genome_len)
    seqs, sites = [G], []
    for p in range(k + rng.randrange(snp_every), genome_len - k, snp_every):
        alt = rng.choice([c for c in "ACGT" if c != G[p]])
        sites.append((p, alt))
        seqs.append(G[p - k + 1:p] + alt + G[p + 1:p + k])
    g = orc.Graph.build(k, seqs, 0, False)
    anno = orc.Annotation(g, n_labels)
    seg = genome_len // n_labels
    for j in range(n_labels):
        anno.annotate(G[max(0, j * seg - widen):min(genome_len, (j + 1) * seg + widen + k - 1)], j)
    L = read_len
    reads = []
    for i in range(n_reads):
        a = rng.randrange(0, genome_len - L)
        r = G[a:a + L]
        kind = i % 3
        if kind == 1:
            r = _sub(r, rng.randrange(k, L))
        elif kind == 2:
            which = (i // 3) % 4
            if which == 0:
                r = mutate(rng, r, 0.01)
            elif which == 1:
                x = rng.randrange(k, L - k)
                r = r[:x] + _other(r[x], r[x - 1]) + r[x:L - 1]
            elif which == 2:
                # the last k-mer starts e positions inside the zone where two segments overlap; the mismatch in the tail, every k-mer
                # in front of it outside the zone
                b = seg * rng.randrange(1, n_labels)
                e = rng.randrange(0, 8)
                a = b - widen + e - (L - k)
                r = _sub(G[a:a + L], rng.randrange(L - k, L - e))
            else:
                # the SNP's other allele at the read's position x, a substitution behind it in the tail: every k-mer that covers the
                # allele covers the mismatch too, the walk goes through the allele's unlabeled nodes
                p, alt = sites[rng.randrange(len(sites))]
                x = rng.randrange(L - k + 2, L - 2)
                a = p - x
                r = G[a:a + L]
                r = _sub(r[:x] + alt + r[x + 1:], rng.randrange(x + 1, L))
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return g, anno, reads


# ---- the GPU batches ----
def class_read(G, i, k=21, L=100):
    """a read of the substitution class from a feature-free stretch: the mismatch at k .. L - 1, either strand"""
    a = free_read(i, L)
    r = _sub(G[a:a + L], k + (i * 5) % (L - k))
    return r if i % 2 else rc(r)


def mixed_batch(n, k=21):
    """-> (graph, annotation, [(name, read)]) of n reads from the directed world: class reads and the other reads in turn — first a
    read without seeds, one with an N, reads of k characters (the span class), perfect reads (the path class), then every refusal
    kind, then the later-seed reads; the first read is a class read"""
    g, anno, rows, G = _directed(k, 8100)
    named = [(name, r) for name, r, _ in rows]
    first = [x for x in named if x[0].startswith("p_")]
    by_name = dict(named)
    perfect = by_name["perfect"]
    specials = [("random", by_name["random"]), ("with_n", by_name["with_n"]), ("span", perfect[:k]), ("span_rc", rc(perfect[40:40 + k])),
                ("perfect", perfect), ("perfect_rc", by_name["perfect_rc"])]
    early = specials + [x for x in named if x[0].startswith(("walk_row", "edge_", "boundary", "label_1", "other_strand", "short_",
                                                            "insertion", "snp_site", "two_", "recomb"))]
    late = [x for x in named if x[0].startswith("later_")][::-1]
    pool = []
    for i in range(max(len(first), len(early))):
        if i < len(first):
            pool.append(first[i])
        if i < len(early):
            pool.append(early[i])
    pool += late
    assert len(pool) >= n, (len(pool), n)
    return g, anno, pool[:n]
