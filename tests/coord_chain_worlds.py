"""Worlds and the judge for the chain stage of LabeledAligner's coordinate mode (mgx_chain_tables_batch).  TEST INFRASTRUCTURE ONLY.

The judge is built only from what the oracle hands out:
  * orc.LabeledAlignRun(g, cfg, anno, reads).seeds(strand): the seeds filter_seeds kept and its num_matching, in coordinate mode too;
  * orc_annotation_row_tuples: the labels and coordinates on the row of a seed's first node;
  * orc_chain_seeds: the sort and the DP of chain_seeds.
The labels a list keeps follow exactly from the first two: a label is kept iff the positions covered by the KEPT seeds that carry it
reach min_exact_match x |query| — every seed that carries a kept label is itself kept, so for a kept label the count is complete,
and for a dropped one it can only be smaller.  The anchors (aligner_chainer.cpp:341-381) are then a dozen lines."""
import ctypes as C
import random

import numpy as np

import orc
from metagraph_amd import capi

K = 11
MATRIX = ("dna", 2, -1, -1)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CONFIGS = {"recipe": {"min_seed_length": 7}, "full_seeds": {"min_seed_length": K}, "exact_match": {"min_seed_length": 7, "min_exact_match": 0.7},
           "one_per_locus": {"min_seed_length": 7, "max_num_seeds_per_locus": 1}}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):
    return "".join(rng.choice([x for x in "ACGT" if x != c]) if rng.random() < rate else c for c in s)


def make_config(name_or_overrides):
    over = CONFIGS[name_or_overrides] if isinstance(name_or_overrides, str) else name_or_overrides
    return orc.make_config(dict(over), MATRIX)


def annotated(k, sequences, label_of, coord_starts):
    g = orc.Graph.build(k, sequences, 0, True)
    anno = orc.Annotation(g, max(label_of) + 1)
    for seq, lab, start in zip(sequences, label_of, coord_starts):
        anno.annotate_coords(seq, lab, start)
    return g, anno


def make_world(seed, n_reads=24, read_len=100, with_sequences=False):
    """k = 11: a genome a + u + b + u + c (three 300-bp blocks, a 60-bp unit twice) under label 0, a 2 % mutated strain under
    label 1, b + u + a under label 2 and a fourth sequence (a piece of the genome and new sequence) under label 0 again;
    coordinates run on per label, so the coordinate ranges within a label are disjoint.  Reads of 100 bp at 0 / 2 / 6 / 15 % errors,
    a third of them reverse-complemented, every twelfth random."""
    rng = random.Random(seed)
    a, b, c, u = rand_seq(rng, 300), rand_seq(rng, 300), rand_seq(rng, 300), rand_seq(rng, 60)
    genome = a + u + b + u + c
    strain = mutate(rng, genome, 0.02)
    third = b + u + a
    fourth = genome[150:330] + rand_seq(rng, 150)
    sequences, label_of = [genome, strain, third, fourth], [0, 1, 2, 0]
    coord_starts = [0, 0, 0, len(genome) + 500]
    g, anno = annotated(K, sequences, label_of, coord_starts)
    reads = []
    for i in range(n_reads):
        if i % 12 == 11:
            reads.append(rand_seq(rng, read_len))
            continue
        src = rng.choice(sequences)
        at = rng.randrange(0, len(src) - read_len + 1)
        r = mutate(rng, src[at:at + read_len], [0.0, 0.02, 0.06, 0.15][i % 4])
        reads.append(revcomp(r) if i % 3 == 2 else r)
    return (g, anno, reads, sequences) if with_sequences else (g, anno, reads)


def row_tuples(anno, row, cache):
    """[(label, [coordinates])] of a row, labels ascending (orc_annotation_row_tuples)"""
    if row not in cache:
        ol = orc.L()
        ol.orc_annotation_row_tuples.restype = C.c_uint64
        ol.orc_annotation_row_tuples.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_uint64]
        cap = 64
        while True:
            labels, cb, co = (C.c_uint64 * max(1, anno.n_labels))(), (C.c_uint64 * (anno.n_labels + 1))(), (C.c_int64 * cap)()
            nl = ol.orc_annotation_row_tuples(anno.h, row, labels, cb, co, cap)
            if nl == 0 or cb[nl] <= cap:
                break
            cap = int(cb[nl])
        cache[row] = [(int(labels[t]), [int(co[x]) for x in range(cb[t], cb[t + 1])]) for t in range(nl)]
    return cache[row]


def clamped_min_seed_length(cfg, k):
    """min_seed_length as DBGAligner's and LabeledAligner's constructors leave it (dbg_aligner.cpp:33-61, aligner_labeled.cpp:463-465)"""
    lo = cfg.min_seed_length or k
    hi = cfg.max_seed_length or k
    return min(k, min(lo, hi))


def chain_on_oracle(cfg, k, lists, query_sizes):
    """orc_chain_seeds over anchor lists of (label, coordinate, clipping, end, score, seed_index) -> (sorted lists, backtraces)"""
    n = sum(len(l) for l in lists)
    begin = np.zeros(len(lists) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum([len(l) for l in lists])
    flat = (capi.ChainAnchor * max(1, n))()
    x = 0
    for l in lists:
        for a in l:
            flat[x] = capi.ChainAnchor(*a)
            x += 1
    back = (C.c_uint32 * max(1, n))()
    qs = np.array(query_sizes, dtype=np.uint32)
    c = capi.Config.from_buffer_copy(cfg)
    c.min_seed_length = clamped_min_seed_length(cfg, k)
    ol = orc.L()
    ol.orc_chain_seeds.restype = None
    ol.orc_chain_seeds.argtypes = [C.POINTER(capi.Config), C.POINTER(capi.ChainAnchor), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint64,
                                   C.POINTER(C.c_uint32)]
    ol.orc_chain_seeds(C.byref(c), flat, begin.ctypes.data_as(C.POINTER(C.c_uint64)), qs.ctypes.data_as(C.POINTER(C.c_uint32)), len(lists), back)
    tup = lambda a: (a.label, a.coordinate, a.seed_clipping, a.seed_end, a.chain_score, a.seed_index)
    out_lists, out_back = [], []
    for l in range(len(lists)):
        b, e = int(begin[l]), int(begin[l + 1])
        out_lists.append([tup(flat[i]) for i in range(b, e)])
        out_back.append([int(back[i]) for i in range(b, e)])
    return out_lists, out_back


def judge(g, cfg, anno, reads, stats=None):
    """-> one dict per list (list 2q = read q, 2q + 1 = its reverse complement), in the layout of aligner.chain_lists: seeds
    [(clipping, length, offset, [nodes])] in chain_seeds' reversed order, num_matching, the sorted anchors with their final scores,
    backtrace.  stats (a dict): counters of what the lists exercise, summed over calls."""
    k = g.k
    run = orc.LabeledAlignRun(g, cfg, anno, reads)
    assert run.error == "", run.error
    per_strand = [run.seeds(0), run.seeds(1)]
    max_locus = int(cfg.max_num_seeds_per_locus)
    cache, out, raw_lists, sizes = {}, [], [], []
    st = stats if stats is not None else {}
    for q, read in enumerate(reads):
        L = len(read)
        for strand in (0, 1):
            seeds, nm = per_strand[strand][q]
            rows = [row_tuples(anno, s["nodes"][0] - 1, cache) for s in seeds]
            covered = {}
            for s, tuples in zip(seeds, rows):
                for lab, _ in tuples:
                    covered.setdefault(lab, set()).update(range(s["clipping"], s["clipping"] + k - s["offset"]))
            kept = {lab for lab, pos in covered.items() if not len(pos) < cfg.min_exact_match * L}
            rev = list(zip(seeds, rows))[::-1]
            anchors = []
            for i, (s, tuples) in enumerate(rev):
                mine = [(lab, coords) for lab, coords in tuples if lab in kept]
                assert mine, "the oracle kept a seed none of whose labels reaches the cut-off"
                for lab, coords in mine:
                    shifted = [c + s["offset"] for c in coords]
                    take = min(len(shifted), max_locus)
                    st["multi_coordinate_pairs"] = st.get("multi_coordinate_pairs", 0) + (len(shifted) > 1)
                    st["tuples_cut"] = st.get("tuples_cut", 0) + (take < len(shifted))
                    for t in range(take):                                    # from the largest coordinate down
                        anchors.append((lab, shifted[len(shifted) - 1 - t], s["clipping"], s["clipping"] + s["length"], s["length"], i))
            keys = [a[:4] for a in anchors]
            st["duplicate_sort_keys"] = st.get("duplicate_sort_keys", 0) + (len(keys) - len(set(keys)))
            st["sub_k_seeds"] = st.get("sub_k_seeds", 0) + sum(1 for s in seeds if s["offset"] > 0)
            st["labels_dropped_with_one_kept"] = st.get("labels_dropped_with_one_kept", 0) + (bool(kept) and len(kept) < len(covered))
            out.append({"seeds": [(s["clipping"], s["length"], s["offset"], list(s["nodes"])) for s, _ in rev], "num_matching": int(nm)})
            raw_lists.append(anchors)
            sizes.append(L)
    sorted_lists, backs = chain_on_oracle(cfg, k, raw_lists, sizes)
    for d, anchors, back in zip(out, sorted_lists, backs):
        d["anchors"], d["backtrace"] = anchors, back
        st["lists"] = st.get("lists", 0) + 1
        st["lists_with_a_back_pointer"] = st.get("lists_with_a_back_pointer", 0) + any(b != 0xFFFFFFFF for b in back)
        st["lists_without_seeds"] = st.get("lists_without_seeds", 0) + (not d["seeds"])
    return out


def kat_worlds():
    """the nine worlds of tests/golden/aligner_coordinate_kats.json as (name, g, anno, cfg, [query])"""
    import json
    import os
    kats = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner_coordinate_kats.json")))
    out = []
    for case in kats["tangle"]:
        g, anno = annotated(case["k"], case["sequences"], list(range(len(case["labels"]))), [0] * len(case["sequences"]))
        out.append((case["name"], g, anno, orc.make_config({}, MATRIX), [case["query"]]))
    for case in kats["coord"]:
        g, anno = annotated(5, case["sequences"], [0] * len(case["sequences"]), case["coord_starts"])
        over = {"max_seed_length": 2 ** 64 - 1}
        if "min_exact_match" in case:
            over["min_exact_match"] = case["min_exact_match"]
        out.append((case["name"], g, anno, orc.make_config(over, MATRIX), [case["query"]]))
    return out


def device_annotation(g, anno, extra=()):
    """the oracle's annotation with its coordinates as an aligner.Annotation on the GPU (from_sparse + set_coordinates).
    extra: further (row, label, [coordinates]) entries the oracle's annotation does not have (labels on rows of dummy nodes, which
    AnnotationBuffer never hands out)"""
    from metagraph_amd import aligner
    cache = {}
    cols = [[] for _ in range(anno.n_labels)]
    for r in range(g.n_edges):
        for lab, coords in row_tuples(anno, r, cache):
            cols[lab].append((r, coords))
    for r, lab, coords in extra:
        cols[lab].append((r, list(coords)))
    col_begin, rows, coord_begin, coords = [0], [], [0], []
    for col in cols:
        for r, cs in col:
            rows.append(r)
            coords += cs
            coord_begin.append(len(coords))
        col_begin.append(len(rows))
    A = aligner.Annotation.from_sparse(g.n_edges, np.array(col_begin, dtype=np.uint64), np.array(rows, dtype=np.uint64))
    A.set_coordinates(col_begin, rows, coord_begin, coords)
    return A
