"""Worlds, the predicate and the closed form for the lane extender's exact exit on LABEL-AWARE batches (metagraph_amd/csrc/
lane_read.hpp lane_exact_class(), DESIGN.md 3.4 "label-aware batches"; TEST INFRASTRUCTURE).  A read of a label-aware batch is in
a class when
  (b) the one-label seed filter passes: every seed's first node has a one-label row, the same label L for all; a strand whose
      covered positions fall below min_exact_match * len loses its seeds; num_matching is recounted over the seeds left;
  (c) the conditions of the unlabeled classes hold on what the filter left (tests/lane_exact_path_worlds.py classify());
  (d) every mapped node of the strand aligned has the row exactly [L].
Its result is the closed form of the unlabeled exit with the label list [L].  Everything here is evaluated from the ORACLE — the
seeds of its plain aligner (what the label filter is given), mapping(), Annotation.get_rows() — and a plain-Python restatement of
the conditions, never from the code under test; the restated filter is itself checked against the oracle's LabeledAligner (its
filtered seed lists and num_matching) for every read it passes."""
import collections
import random

import lane_exact_path_worlds as PW
import lane_exact_worlds as W
import orc
from test_emu_vs_oracle import mutate, rand_seq, rc


def label_filter(cfg, k, read, seeds_fwd, seeds_rc, row_of):
    """the one-label case of LabeledAligner::filter_seeds on both strands -> (label, (seeds, num_matching) per strand) or None
    when a seed's first node has no or several labels or two seeds differ.  row_of(node) -> the node's label list"""
    L = len(read)
    both = bool(cfg.forward_and_reverse_complement)
    label = None
    out = []
    for strand, (seeds, nm_hdr) in enumerate((seeds_fwd, seeds_rc)):
        if not seeds or (strand and not both):
            out.append((list(seeds), nm_hdr))
            continue
        covered = set()
        nm, last_end, counting = 0, 0, True
        for sd in seeds:
            row = row_of(sd["nodes"][0])
            if len(row) != 1:
                return None
            if label is None:
                label = row[0]
            elif row[0] != label:
                return None
            cl, off = sd["clipping"], sd["offset"]
            covered.update(range(cl, min(cl + k - off, L)))
            if counting:
                # get_num_char_matches_in_seeds: nothing behind the first sub-k seed counts
                q_end = cl + sd["length"]
                if q_end > last_end:
                    nm += (q_end - cl) - (last_end - cl if cl < last_end else 0)
                last_end = q_end
                if off:
                    counting = False
        keep = not (float(len(covered)) < cfg.min_exact_match * float(L))
        out.append((list(seeds), nm) if keep else ([], 0))
    if label is None:
        return None
    return label, out[0], out[1]


Classes = collections.namedtuple("Classes", "span path label run plain nodes filtered")


def classes(g, anno, cfg, reads, run=None):
    """-> Classes: span / path {read: strand}, label {read: L}, the LabeledAligner run, the plain run, its mapping,
    filtered {read: ((seeds, nm) forward, (seeds, nm) reverse)} for the reads in a class"""
    # what the label filter is given: LabeledAligner seeds with min_seed_length and max_seed_length clamped to k
    # (aligner_labeled.cpp:464-465), so every seed of k characters or more is one k-mer
    import copy
    pcfg = copy.copy(cfg)
    pcfg.min_seed_length = min(g.k, cfg.min_seed_length)
    pcfg.max_seed_length = min(g.k, cfg.max_seed_length)
    plain = orc.AlignRun(g, pcfg, reads, threads=8, validate=False)
    assert plain.error == "", plain.error
    run = run or orc.LabeledAlignRun(g, cfg, anno, reads, validate=False)
    assert run.error == "", run.error
    sf, sr, mp = plain.seeds(0), plain.seeds(1), plain.mapping()
    lf, lr = run.seeds(0), run.seeds(1)
    n_rows = g.n_edges                                   # (row = node - 1; a node is an edge index of the BOSS table)
    cache = {}

    def row_of(node):
        if node not in cache:
            cache[node] = [int(x) for x in anno.get_rows([node - 1])[0]] if 0 < node <= n_rows else []
        return cache[node]

    span, path, label, filtered = {}, {}, {}, {}
    for q, r in enumerate(reads):
        f = label_filter(cfg, g.k, r, sf[q], sr[q], row_of)
        if f is None:
            continue
        lbl, f0, f1 = f
        # the restated filter against the oracle's own
        assert [emu_tuple(s) for s in f0[0]] == [emu_tuple(s) for s in lf[q][0]] and f0[1] == lf[q][1], (q, r, f0, lf[q])
        assert [emu_tuple(s) for s in f1[0]] == [emu_tuple(s) for s in lr[q][0]] and f1[1] == lr[q][1], (q, r, f1, lr[q])
        kind, s = PW.classify(cfg, g.k, r, f0, f1, mp[q])
        if kind is None:
            continue
        if any(row_of(v) != [lbl] for v in mp[q][s]):
            continue
        (span if kind == "span" else path)[q] = s
        label[q] = lbl
        filtered[q] = (f0, f1)
    return Classes(span, path, label, run, plain, mp, filtered)


def emu_tuple(s):
    return (s["clipping"], s["length"], s["offset"], s["nodes"][0] if s["offset"] else len(s["nodes"]))


def closed_form(cfg, read, strand, mapped, label):
    out = PW.closed_form(cfg, read, strand, mapped)
    out[0]["labels"] = [label]
    return out


def check_closed_form(g, anno, cfg, reads):
    """the oracle's LabeledAligner result of every read in a class is the closed form with the label list [L] -> Classes"""
    from labeled_worlds import with_labels
    c = classes(g, anno, cfg, reads)
    want = with_labels(c.run)
    for cls in (c.span, c.path):
        for q, s in cls.items():
            assert want[q] == closed_form(cfg, reads[q], s, c.nodes[q][s], c.label[q]), (q, reads[q], want[q])
    return c, want


# ---- the directed world: a hand-built graph ----
# genome of 2600 characters; label 0 on its k-mers that start before BOUNDARY, label 1 on the others (so a read across BOUNDARY
# has one-label rows all along, of two labels); four bubbles inside label 0 whose alternative paths carry: the same label, another
# label (2), two labels (0 and 2), none
BOUNDARY = 1700
BUBBLES = (("same", 300), ("other", 600), ("two", 900), ("none", 1200))


def _other(c):
    return next(x for x in "TGCA" if x != c)


def directed_world(k, seed=7300):
    """-> (graph, annotation, [(name, read, expected: 'in' (one of the classes), 'out' or None = whatever the seeds say)])"""
    rng = random.Random(seed + k)
    G = rand_seq(rng, 2600)
    alts = {name: G[p - k + 1:p] + _other(G[p]) + G[p + 1:p + k] for name, p in BUBBLES}
    g = orc.Graph.build(k, [G] + [alts[name] for name, _ in BUBBLES], 0, False)
    anno = orc.Annotation(g, 3)
    anno.annotate(G[:BOUNDARY + k - 1], 0)
    anno.annotate(G[BOUNDARY:], 1)
    anno.annotate(alts["same"], 0)
    anno.annotate(alts["other"], 2)
    anno.annotate(alts["two"], 0)
    anno.annotate(alts["two"], 2)
    rows = []

    def add(name, r, kind):
        rows.append((name, r, kind))
        rows.append((name + "_rc", rc(r), kind))

    for name, p in BUBBLES:
        for L in (60, 100, 139):
            a = p - L // 2
            main = G[a:a + L]
            # along the genome: the other allele is a side branch, whatever its labels
            add("main_%s_%d" % (name, L), main, "in")
            # through the alternative allele: its k nodes carry the allele's row
            alt = main[:p - a] + _other(G[p]) + main[p - a + 1:]
            add("alt_%s_%d" % (name, L), alt, "in" if name == "same" else "out")
        # the allele's nodes at the read's first / last k-mer only
        add("alt_first_kmer_%s" % name, G[p - k + 1:p] + _other(G[p]) + G[p + 1:p + 80], "in" if name == "same" else "out")
        add("alt_last_kmer_%s" % name, G[p - 80:p] + _other(G[p]) + G[p + 1:p + k], "in" if name == "same" else "out")
    # across the segment boundary: rows [0] then [1]
    for L in (k + 5, 100):
        a = BOUNDARY - (L - k + 1) // 2                  # (its k-mers start on both sides of the boundary)
        add("boundary_%d" % L, G[a:a + L], "out")
    add("label_1", G[BOUNDARY + 200:BOUNDARY + 300], "in")
    # reads of k and k + 1 characters, reads between two bubbles (one MEM)
    for L in (k, k + 1, 40, 120):
        add("plain_L%d" % L, G[400:400 + L], "in")
    base = G[700:800]
    add("substitution", base[:50] + _other(base[50]) + base[51:], "out")
    add("first_kmer_missing", _other(base[0]) + base[1:], "out")
    add("last_kmer_missing", base[:-1] + _other(base[-1]), "out")
    rows.append(("random", rand_seq(rng, 100), "out"))
    rows.append(("short", G[500:500 + k - 1], "out"))
    rows.append(("with_n", base[:30] + "N" + base[31:], "out"))
    return g, anno, rows


def segment_directed(seed, k=21):
    """test_lane_labels.segment_world with perfect reads added: along the genome inside a segment, across a segment boundary,
    through the SNP alleles (unlabeled, or carrying their segment's label) -> (graph, annotation, reads)"""
    from test_lane_labels import segment_world
    g, anno, reads = segment_world(seed, k=k, label_alt=seed % 2 == 0)
    rng = random.Random(seed * 7 + 1)
    # (the same genome again: segment_world draws it first from its seed)
    G = rand_seq(random.Random(seed), 6000)
    seg = 6000 // 6
    for j in range(1, 6):
        for L in (k + 5, 80):
            r = G[j * seg - L // 2:j * seg - L // 2 + L]
            reads += [r, rc(r)]
    for i in range(60):
        L = rng.randrange(k, 140) if i % 6 else k           # (a read of k characters is one seed: the span class)
        p = rng.randrange(0, 6000 - L)
        r = G[p:p + L]
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return g, anno, reads


# ---- random worlds: the benchmark's annotation in small ----
def random_world(seed, k, genome_len=6000, n_labels=6, n_bubbles=60, n_reads=260, widen=15):
    """genome segments as labels, each widened by `widen` positions into its neighbours (bench.py --labels); bubbles whose
    alternative paths carry the same label, another label, both or none; perfect reads of k .. 139 characters on both strands, a
    third of them through an alternative allele; a tenth of the reads with substitutions or random"""
    rng = random.Random(seed * 1000 + k)
    G = rand_seq(rng, genome_len)
    seg = genome_len // n_labels
    sites = sorted(rng.sample(range(k + 5, genome_len - k - 5, 2 * k + 3), n_bubbles))
    alts = [(p, _other(G[p]) if rng.random() < 0.5 else rng.choice([c for c in "ACGT" if c != G[p]])) for p in sites]
    seqs = [G] + [G[p - k + 1:p] + a + G[p + 1:p + k] for p, a in alts]
    g = orc.Graph.build(k, seqs, 0, False)
    anno = orc.Annotation(g, n_labels)
    for j in range(n_labels):
        anno.annotate(G[max(0, j * seg - widen):min(genome_len, (j + 1) * seg + widen + k - 1)], j)
    for i, (p, a) in enumerate(alts):
        own = min(n_labels - 1, p // seg)
        sq = seqs[1 + i]
        kind = i % 4
        if kind in (0, 2):
            anno.annotate(sq, own)
        if kind in (1, 2):
            anno.annotate(sq, (own + 1) % n_labels)
    reads = []
    for i in range(n_reads):
        L = rng.randrange(k, 140) if i % 8 else k
        if i % 3 == 0:
            p, a = alts[rng.randrange(len(alts))]
            s = max(0, min(genome_len - L, p - rng.randrange(L)))
            r = G[s:s + L]
            r = r[:p - s] + a + r[p - s + 1:]
        else:
            s = rng.randrange(0, genome_len - L)
            r = G[s:s + L]
        if i % 10 == 9:
            r = mutate(rng, r, 0.03) if i % 20 == 9 else rand_seq(rng, L)
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return g, anno, reads


# ---- the GPU batches: the directed world's reads, the four bubbles in turn, the other reads spread among them ----
def mixed_batch(n, k=21):
    """-> (graph, annotation, [(name, read)]) of n reads: reads of both classes, reads refused for each row reason, reads with
    substitutions, without seeds, across the boundary, on both strands; beyond the directed world's own reads their tails (perfect
    reads still) and copies with a substitution"""
    g, anno, rows = directed_world(k)
    per_bubble = [[r for r in rows if r[0].split("_")[:2] in (["main", b], ["alt", b]) or r[0].startswith(("alt_first_kmer_" + b, "alt_last_kmer_" + b))]
                  for b, _ in BUBBLES]
    assert len({len(x) for x in per_bubble}) == 1
    bubbles = [per_bubble[b][i] for i in range(len(per_bubble[0])) for b in range(4)]
    others = [r for r in rows if r not in bubbles]
    # (the read without seeds, the short one, the one with an N and those with a substitution: early)
    early = [r for r in others if r[0].startswith(("random", "short", "with_n", "substitution"))]
    others = early + [r for r in others if r not in early]
    pool, oi = [], 0
    for i, r in enumerate(bubbles):
        pool.append(r)
        if i % 3 == 2 and oi < len(others):
            pool.append(others[oi])
            oi += 1
    pool += others[oi:]
    extra = []
    for i, (name, r, _) in enumerate(pool):
        if len(r) > k + 8:
            extra.append((name + "_tail", r[3:], None))
            if i % 4 == 0:
                m = len(r) // 2
                extra.append((name + "_sub", r[:m] + _other(r[m]) + r[m + 1:], None))
    pool += extra
    assert len(pool) >= n, (len(pool), n)
    return g, anno, [(name, r) for name, r, _ in pool[:n]]
