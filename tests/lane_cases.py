"""Directed worlds for the lane-per-read extender (metagraph_amd/csrc/lane_read.hpp, lane_column.hpp; TEST INFRASTRUCTURE): one
builder per case, each a small graph and a few reads whose fate in lane_read() follows from the arithmetic of one guard.  The host
model pins the fate per read (tests/test_lane_edges.py), the GPU tests compare the kernel's histogram with it
(tests/test_gpu_lane_edges.py).

A builder returns Case(graph, config, limits or None, annotation or None, reads, expected):
  expected[i]    the LANE_BAIL code read i goes to the group kernel with, 0 = a lane finishes it.
Everything is deterministic: the genomes come from seeded generators, the reads are cut from them by rule.  Every case holds a read
that a lane finishes and a plain read cut from the genome.  The derivation of each expected code stands next to its builder; the
constants are the CLI's unless the case says otherwise: match 2, mismatch -3, gap open -6, gap extension -2, xdrop 27, both end
bonuses 5, rel_score_cutoff 0.95, min_seed_length 19, and LFW = 32 window cells, K = 21.

The codes (LANE_BAIL(code) in lane_read.hpp) and where they are reached:
  1  L > Lmax or L > 256: NOT REACHABLE.  derive_limits() sets Lmax to the batch's longest read rounded up to 8, and
     lane_enabled() keeps the kernel off a batch whose Lmax exceeds LANE_MAX_L_HOST = 256 = LANE_MAX_L.  Nothing asserted.
  2  seed header not ST_OK          seed_limit (mgx_limits.max_seeds lowered)
  3  a second strand to align       second_strand (boundary pair on num_matching), second_strand_rel0, the shapes
  4  more than LANE_MAX_SEEDS = 512 seeds on the strand       many_seeds (513 seeds against 510; 576, where max_seeds is full)
  5  a character outside ACGT       invalid_character.  The second site (the other strand, loaded for the backward pass) is NOT
     REACHABLE: the reverse complement's invalid-character words are the forward strand's mirrored, so pass 0 has left already.
  6  the first seed's first node is 0: NOT REACHABLE.  A seed is written for a matched k-mer (its node is the mapping's, non-zero)
     or for a sub-k range (its node is an edge of the graph, >= 1).  Nothing asserted.
  7  a replay column of the first seed's first node without its S row: NOT REACHABLE.  It is tested for a later seed whose last
     node is node0; then the filter of pass 0 holds node0's bit (or is all ones), and keep_row of every column of node0 was set.
  8  the root's record does not fit the cell arena       cell_arena_root_204 (against _208)
  9  the root does not fit the window                    root_window_57 (against root_window_56; L = 29 against 28)
 10  more than two children        three_way_fork (the fork at column K against K - 1), the shapes
 11  a child that is node 0: NOT REACHABLE.  lane_children() / lane_parents() return edges i >= 2 that are in the graph, a
     replayed node is a node of the seed or of the forward path.  Nothing asserted.
 12  the column table is full      max_columns (L = 61 against 60 at max_columns = 64)
 13  the cell arena's test         cell_arena_2332 (against _2336; L = 104 against 100), cell_arena_root_*
 14  a column that does not fit the window (LC_FALLBACK): NOT REACHED, not proven unreachable.  The band half cannot happen: the
     head passed `(trim & 3) + size + 3 <= LFW` (codes 9 and 16) and the child's band lies inside the head's cells, so
     (begin - org) + max(n_loop, size0) <= (trim & 3) + size + 3.  The other half — an insertion run of three or more cells behind
     a column of 30 — needs gap extensions far below the match score and a cut-off that stood still; wide x-drops with the
     CLI's gaps and with -58 / -32 (root_window_*, wide_rows_*) and random reads with insertions at xdrop 45 ended in 16.
 15  a node seen before            tandem_repeat
 16  a head that does not fit the window                 root_window_56
 17  a kept S row with a cell more than 127 below the column's maximum     wide_rows_126_32 (against _126_33 and _125_32)
 18  no start cell after the forward extension: NOT REACHED, not proven unreachable.  Random reads with substitutions, insertions,
     deletions and junk ends under nine configurations (no end bonuses, sub-k seeds, min_cell_score, min_path_score among
     them: tools/lane_code_harvest.py, seeds and configurations there) always had one: the seed's own columns score above every
     min_start_score the forward pass runs with.
 19  a later seed that lives       later_seed, bubbles (a sub-k seed behind a bubble), many_seeds, the shapes; the staying sides:
     merged_vector (a later seed that ends in the first seed's first node), later_seeds_16_17, every read with a substitution
 20  more than LANE_MAX_RUNS = 16 CIGAR runs             cigar_runs (17 runs against 16 and 15)
 21  DEAD CODE: `bad` is set only inside an iteration of the trace whose last statement is `if (bad || ...) LANE_BAIL(20)`.
 22, 23, 24, 26, 29: NOT REACHED, not proven unreachable.  Tried: tools/lane_code_harvest.py (22 410 reads with its default seed, none of these); allow_left_trim = 0 with a
     substitution at positions 0 .. 15 (left_trim_off: the forward trace still ends in the root, the backward pass finishes
     the read); reads with junk at either end.  24 and 22 need a trace that leaves the band or ends short of k - offset
     columns, 23 a cell below the trace's start by more than the extension's minimum, 26 a forward alignment without nodes,
     29 a trace that ends inside a column whose row was not kept.
 27  an equal-score batch          ties (inside the query: leaves; beyond its end: LANE_TIE_MODE, stays), tie_size_cap_1.07
     (against _1.075: stop_all / the size caps under tie mode), the shapes.  Two sites are NOT REACHED, not proven unreachable:
     tie mode followed by a new best score, and by a competing start cell.  Tie mode begins beyond the query's end, where a
     column gains nothing on its parent, and the best start cell is the last query column's (its score and the end bonus); a
     column that stayed behind inside the query and is revived after the tie carries the head's remaining characters less
     its own mismatch.  Tried: tools/lane_code_harvest.py (reads that end 0 .. K before and behind every fork, five configurations).
 28  no frontier slot left         bubbles (the fourth fork against the third; the third against the second), the shapes
 30  label-aware: not "one label all along"              labels (five ways in, and the fork that stays)
 31  the backward pass has no start cell and the forward alignment was not added     min_path_score_206 (against _205)
"""
import collections
import functools
import random

import orc
from metagraph_amd import capi
from test_emu_vs_oracle import rand_seq, rc

Case = collections.namedtuple("Case", "graph config limits annotation reads expected")

K = 21
REACHED = {2, 3, 4, 5, 8, 9, 10, 12, 13, 15, 16, 17, 19, 20, 27, 28, 30, 31}      # (the table above)
UNREACHABLE = {1, 6, 7, 11, 21}
NOT_REACHED = {14, 18, 22, 23, 24, 26, 29}
CAPACITY = {2, 8, 12, 13}            # the group kernel meets the same limit: the read's status is MGX_ERR_CAPACITY until the retry


def _other(c, avoid=""):
    return next(x for x in "TGCA" if x != c and x not in avoid)


def _sub(read, *positions):
    """the read with the characters at `positions` substituted"""
    r = list(read)
    for p in positions:
        r[p] = _other(r[p])
    return "".join(r)


def _rows(graph, cfg, rows, limits=None, annotation=None):
    return Case(graph, cfg, limits, annotation, [r[0] for r in rows], [r[1] for r in rows])


# ---- the main world: K = 21, a random genome (forward strand only), bubbles, a three-way fork, a segment on both strands --------

SNPS_ALT_FIRST = [600, 625, 650, 690]        # genome T, other allele A: the child that mismatches the read comes first in edge order
SNPS_ALT_LAST = [900, 925, 960]              # genome A, other allele T: the child that matches comes first
SNP_TIE = 1200
FORK3 = 1500                                 # three alleles
TWIN = (2000, 2300)                          # this segment's reverse complement is in the graph too
CLEAN = (100, 560)                           # no feature in G[100:560] and from 2400 on


@functools.lru_cache(maxsize=None)
def main_world():
    rng = random.Random(7001)
    G = list(rand_seq(rng, 4000))
    for p in SNPS_ALT_FIRST:
        G[p] = "T"
    for p in SNPS_ALT_LAST:
        G[p] = "A"
    G = "".join(G)
    alleles = [(p, "A") for p in SNPS_ALT_FIRST] + [(p, "T") for p in SNPS_ALT_LAST] + [(SNP_TIE, _other(G[SNP_TIE]))]
    a1 = _other(G[FORK3])
    alleles += [(FORK3, a1), (FORK3, _other(G[FORK3], a1))]
    seqs = [G] + [G[p - K + 1:p] + a + G[p + 1:p + K] for p, a in alleles]
    seqs.append(rc(G[TWIN[0]:TWIN[1]]))
    return orc.Graph.build(K, seqs, 0, False), G


def plain(p, L=100):
    return main_world()[1][p:p + L]


def cli(**kw):
    cfg = capi.config_cli(K)
    for a, v in kw.items():
        setattr(cfg, a, v)
    return cfg


def limits(**kw):
    lim = capi.Limits()
    for a, v in kw.items():
        setattr(lim, a, v)
    return lim


# ---- read set-up ------------------------------------------------------------------------------------------------------------------

def no_seeds():
    """reads without seeds finish in the lane (n == 0: no extension, an empty result): the empty read, L < K, a random read, a
    read of N"""
    g, G = main_world()
    rng = random.Random(7002)
    return _rows(g, cli(), [("", 0), ("ACGT", 0), (G[100:120], 0), (rand_seq(rng, 100), 0), ("N" * 50, 0), (plain(100), 0), (rc(plain(300)), 0)])


def second_strand():
    """code 3: `m_second >= m_first * rel_score_cutoff && n_second > 0`.  G[2000:2300] is in the graph on both strands.  A read of
    100 characters inside it matches 100 characters on either strand: 3.  A read that ends 5 characters behind the segment
    matches 100 on its own strand and 95 on the other: 95 >= 100 * 0.95, 3; 6 characters behind: 94 < 95, the lane aligns the
    one strand.  The same from the other strand."""
    g, G = main_world()
    a, b = TWIN
    return _rows(g, cli(), [(G[a + 50:a + 150], 3), (G[b - 95:b + 5], 3), (G[b - 94:b + 6], 0), (rc(G[b - 95:b + 5]), 3), (rc(G[b - 94:b + 6]), 0),
                            (plain(100), 0)])


def second_strand_rel0():
    """code 3 with rel_score_cutoff = 0 (and min_exact_match = 0, so that a strand with few matches keeps its seeds): 0 >= 0 holds
    for a strand without matches, and `n_second > 0` alone keeps the plain reads in the lane; 30 matching characters on the
    other strand (the read starts 30 before the twin segment's end), or 25 (a chimera), have seeds: 3"""
    g, G = main_world()
    b = TWIN[1]
    cfg = cli(rel_score_cutoff=0.0, min_exact_match=0.0)
    return _rows(g, cfg, [(plain(100), 0), (G[b - 30:b + 70], 3), (plain(3000, 75) + rc(plain(3300, 25)), 3), (rc(plain(200)), 0)])


def invalid_character():
    """code 5: an N behind 90 and behind 5 matching characters (the rest still reaches min_exact_match: the read has seeds)"""
    r = plain(100)
    return _rows(main_world()[0], cli(), [(r[:90] + "N" + r[91:], 5), (r[:5] + "N" + r[6:], 5), (r, 0), (rc(r)[:40] + "n" + rc(r)[41:], 5)])


def seed_limit():
    """code 2: one seed per k-mer (max_seed_length = K): L - 20 seeds on the read's strand.  max_seeds = 85: L = 105 fills it,
    L = 106 gets the seeder's capacity status, which the lane passes on"""
    cfg = cli(max_seed_length=K)
    return _rows(main_world()[0], cfg, [(plain(100, 105), 0), (plain(100, 106), 2), (plain(400, 60), 0), (rc(plain(200, 106)), 2)], limits(max_seeds=85))


@functools.lru_cache(maxsize=None)
def _triples_world():
    """k = 16: a read of 256 random characters and, per position i, three contigs of one k-mer each that end with read[i:i + 12]
    behind a character that is not read[i - 1]: every position matches exactly 12 characters, in three nodes"""
    rng = random.Random(7020)
    read = rand_seq(rng, 256)
    seqs = []
    for i in range(256 - 11):
        for pre in ("ACG", "CGT", "GTA"):                 # (three different k-mers)
            seqs.append(pre + _other(read[i - 1] if i else "A") + read[i:i + 12])
    G = rand_seq(rng, 1500)
    return orc.Graph.build(16, seqs + [G], 0, False), read, G


def many_seeds():
    """code 4: `n > LANE_MAX_SEEDS` = 512.  k = 16, min_seed_length = 12, min_exact_match = 0: a read of L characters of the
    triples world has L - 11 positions with a sub-k seed of three nodes each: 3 (L - 11) seeds on its strand, none on the other.
    The batch's longest read has 256 characters: max_seeds = 2 x 256 + 64 = 576.  L = 182: 513 seeds: 4.  L = 181: 510 seeds pass;
    the first seed's extension ends with its contig, every later seed's node is another contig's: 19.  L = 203: 576 seeds fill
    max_seeds, the seeder still reports ST_OK: 4."""
    g, read, G = _triples_world()
    cfg = capi.config_cli(16)
    cfg.min_seed_length = 12
    cfg.min_exact_match = 0.0
    return _rows(g, cfg, [(read[:182], 4), (read[:181], 19), (read[:203], 4), (G[100:356], 0), (G[500:600], 0)])


MANY_SEEDS = [513, 510, 576]                 # the oracle's seeds on the strand of the first three reads of many_seeds()


# ---- the root column ------------------------------------------------------------------------------------------------------------------

def root_window(xdrop):
    """codes 9 and 16.  A seed at query position 0: the root's cell 0 scores the left end bonus 5, its insertion run 5 - 6 = -1,
    -3, ... down to -xdrop, at most L cells of it (the window has L + 1): root_size = 1 + min(L, 1 + (xdrop - 1) // 2).
      xdrop = 57, L >= 29: root_size = 30, 30 + 3 > 32: 9.  L = 28: 29 fits, and so does every column: none has more than
      L + 1 = 29 cells, and its trim grows as its size shrinks (`(trim & 3) + size + 3 <= LFW`): the lane finishes the read.
      xdrop = 56, L >= 29: root_size = 29 fits (29 + 3 <= 32); the first column holds the root's 29 cells and one more (L = 29:
      its 30 cells are the whole window; longer: the 29 of the band, the tail cell, an insertion cell): more than 29, 16.
      L = 28 as before."""
    cfg = cli(xdrop=xdrop)
    big = 9 if xdrop >= 57 else 16
    return _rows(main_world()[0], cfg, [(plain(100, 28), 0), (plain(100, 29), big), (plain(100, 30), big), (plain(100, 100), big), (rc(plain(400, 28)), 0), ("ACGT", 0)])


def cell_arena_root(nbytes):
    """codes 8 and 13.  xdrop 27: the root of a seed at position 0 has 1 + 14 cells (5, -1, -3 ... -27), one that starts later
    (sroot = 0: -6 ... -26) 1 + 11.  rec_words(w) = (2 w + w / 4 + 3) & ~3: the root's test asks for rec_words(15 + 8) = 52
    words, rec_words(12 + 8) = 48.  51 words (204 bytes): 8 for the first kind, the second passes and fails the first column's
    test (13: it asks for 4 x 72 words more); 52 words (208 bytes): 13 for both.  The group kernel has the same root test: the
    reads get a capacity status and the batch's retry aligns them.  A read without seeds needs no arena."""
    rng = random.Random(7003)
    first = 8 if nbytes < 208 else 13
    return _rows(main_world()[0], cli(), [(plain(100), first), (_sub(plain(100), 0), 13), (rand_seq(rng, 100), 0), (plain(500, 40), first)],
                 limits(cell_arena_bytes=nbytes))


def cell_arena(nbytes):
    """code 13: cell_top + (LANE_MAX_DEFER + 1) rec_words(32) + rec_words(window_size + 1 - begin + 8) > cell_words.  A read
    without forks keeps cell_top at the root's rec_words((15 + 8) & ~3) = 48; rec_words(32) = 72; the last term is largest at
    the first column (begin = 0): L = 100: rec_words(109) = 248, L = 104: rec_words(113) = 256, L = 40: rec_words(49) = 112.
    48 + 288 + 248 = 584 words = 2336 bytes: L = 100 stays, L = 104 (592) leaves; 2332 bytes = 583 words: L = 100 leaves."""
    at = 0 if nbytes >= 2336 else 13
    return _rows(main_world()[0], cli(), [(plain(100), at), (plain(100, 104), 13), (plain(100, 40), 0), (rc(plain(300)), at)], limits(cell_arena_bytes=nbytes))


# ---- the column loop ------------------------------------------------------------------------------------------------------------------

def max_columns():
    """code 12: `tsize >= max_columns - 1` before a column is computed, tsize = 1 + the columns committed.  A read that matches
    all along asks for L columns on the query, then for the deletion columns behind its end: with s = 5 + 2 L in [120, 160) the
    first (s - 6 >= int(0.95 s)) is committed, the second (s - 8) is computed and popped.  L + 2 requests, the last with
    tsize = L + 2.  max_columns = 64 (the floor of derive_limits): L = 60 asks with tsize up to 62, L = 61 with 63: 12.
    L = 40 (s = 85: the first deletion column is popped): 41 requests."""
    return _rows(main_world()[0], cli(), [(plain(100, 60), 0), (plain(100, 61), 12), (plain(100, 64), 12), (rc(plain(300, 60)), 0), (plain(100, 40), 0)],
                 limits(max_columns=64))


def three_way_fork():
    """code 10.  Three alleles at G[1500].  The columns 0 .. K - 1 of a seed replay its first node (`no < k`); from column K on the
    head's children are enumerated.  A read that starts at 1500 - K has the fork at column K: 10; one that starts a character
    later has all three alleles' position inside its first node: no fork is ever seen."""
    p = FORK3
    return _rows(main_world()[0], cli(), [(plain(p - 50), 10), (plain(p - K), 10), (plain(p - K + 1), 0), (plain(p - 10), 0), (plain(100), 0)])


def tandem_repeat():
    """code 15: a unit of 25 >= k = 15 characters eight times over: the k-mers of one copy are the next copy's, the extension of a
    read inside the repeat meets its first node again after 25 columns.  (The model of tests/test_lane_read.py.)  Reads of the
    flanks finish."""
    rng = random.Random(7005)
    unit = rand_seq(rng, 25)
    genome = rand_seq(rng, 300) + unit * 8 + rand_seq(rng, 300)
    g = orc.Graph.build(15, [genome], 0, False)
    rows = [(genome[p:p + 120], 15) for p in (250, 300, 320)] + [(genome[20:140], 0), (genome[560:680], 0)]
    return _rows(g, capi.config_cli(15), rows)


def wide_rows(xdrop, ge):
    """code 17 and the cell-by-cell packing of an S row (m + xdrop > 127), gap open -58, min_seed_length = K (no sub-k seeds: a
    plain read has one seed, an empty filter and keeps no row).  A kept row's column c has, three cells below its diagonal, the
    cell of a deletion over columns c - 2 .. c: (base - 6) - 58 + 2 ge.  The cut-off the column ran with is the best score before
    it minus xdrop = base - 2 - xdrop.
      xdrop 126, ge -32: that cell is base - 128 = the cut-off: real, and more than 127 below base: 17 — for the read with a
      substitution at 50 (two seeds: the column of the later seed's last node keeps its row) and the one with a substitution at 5
      (a backward pass, whose replay columns keep theirs).
      xdrop 126, ge -33: base - 130 lies below the cut-off; the lowest real cells are at base - 126: the rows are packed cell by
      cell and the reads finish.   xdrop 125, ge -32: m + xdrop = 127, the clamping form packs them."""
    cfg = cli(xdrop=xdrop, gap_opening_penalty=-58, gap_extension_penalty=ge, min_seed_length=K)
    at = 17 if (xdrop, ge) == (126, -32) else 0
    return _rows(main_world()[0], cfg, [(plain(100), 0), (_sub(plain(300), 50), at), (_sub(plain(400), 5), at), (rc(plain(100)), 0)])


def bubbles():
    """code 28 at its two sites.  The first child of a fork is parked in a free frontier slot while the second is computed; the
    child that mismatches the read stays behind (it is popped when the extension ends).  The children come in edge order,
    A < C < G < T.
      genome T, allele A (SNPs at 600, 625, 650, 690): the mismatching child comes first and keeps its slot.  Three forks fill
      the three slots (G[560:673]: the lane finishes it); at the fourth no slot is free for the first child (G[560:715]): 28.
      genome A, allele T (900, 925, 960): the matching child is parked, the mismatching one takes another slot.  Two forks:
      slots 1 and 2 (G[860:948] finishes); at the third, slot 0 holds the parked child and nothing is free (G[860:983]): 28.
    (The staying reads end K characters or more behind their last SNP: the sub-k seed of a read's last 19 characters would
    otherwise have the other allele's node too, which is not on the path: 19.  The next SNP lies more than the four deletion
    columns behind the read's end away: a fork there would want a slot as well.)"""
    return _rows(main_world()[0], cli(), [(plain(560, 113), 0), (plain(560, 155), 28), (plain(860, 88), 0), (plain(860, 123), 28), (plain(100), 0), (plain(560, 110), 19)])


def ties():
    """code 27 and LANE_TIE_MODE.  Two alleles at G[1200].  A read with the third character there: both children score the same
    mismatch, an equal-score batch inside the query: 27.  A read that ends at 1199: the fork is the first column beyond the
    query's end, its children tie on deletions alone: the lane takes its own order (tie mode), both branches run into the
    x-drop, the read finishes.  A read that ends with 1200 itself: an ordinary fork."""
    g, G = main_world()
    p = SNP_TIE
    third = _other(G[p], _other(G[p]))
    r = plain(p - 50)
    return _rows(g, cli(), [(r[:50] + third + r[51:], 27), (plain(p - 100, 100), 0), (plain(p - 99, 100), 0), (plain(100), 0)])


def tie_size_cap(cap):
    """code 27, the size caps under LANE_TIE_MODE (`stop_all && LANE_TIE_MODE()` for a head or a popped column below the best
    score, and the same comparison once more when the extension ends): tsize / window_size >= max_nodes_per_seq_char.  The read
    of ties() that ends at 1199 (L = window_size = 100, score s = 205): 100 columns on the query, then the fork; each branch
    commits the deletion columns s - 6, s - 8, s - 10 >= int(0.95 s) = 194 and has the next popped.  With the root
    tsize = 1 + 100 + 3 + 3 = 107.  cap = 1.07: 107 / 100 >= 1.07, in tie mode: 27.  cap = 1.075: never reached, the read
    finishes.  A plain read commits 1 + 100 + 3 = 104 < 107 columns and is in no tie mode: it finishes under either."""
    p = SNP_TIE
    return _rows(main_world()[0], cli(max_nodes_per_seq_char=cap), [(plain(p - 100, 100), 27 if cap <= 1.07 else 0), (plain(100), 0), (rc(plain(300)), 0)])


# ---- after the extension ---------------------------------------------------------------------------------------------------------------

def later_seed():
    """code 19: a chimera of two places of the genome: the second seed's last node is not on the first seed's extension.  A read
    with a substitution has a second seed too — on the path: it dies on the kept row of its last node's column."""
    return _rows(main_world()[0], cli(), [(plain(100, 50) + plain(3000, 50), 19), (_sub(plain(100), 50), 0), (plain(100), 0)])


def later_seeds_16_17():
    """the S-row filter: one seed per k-mer, L = K + 16 and K + 17: 16 later seeds (one filter bit each) and 17
    (> LANE_S8_FILTER_SEEDS: every column keeps its row); all of them die on the path"""
    cfg = cli(max_seed_length=K)
    return _rows(main_world()[0], cfg, [(plain(100, K + 16), 0), (plain(100, K + 17), 0), (plain(100, K), 0), (plain(100, 100), 0)])


def merged_vector():
    """the later seed that ends in the first seed's first node (`ln == node0`: the merged vector of the replay columns,
    lane_merge_column).  K characters of the genome and a character that is not the next one: one matched k-mer, seed 0 = its
    node; the last k-mer matches nothing, so the read's tail is looked up: read[2:21], 19 characters, is a sub-k seed (clipping 2,
    offset 2) that reports the same node.  Its last position 20 lies in the vector (the K replay columns cover positions
    0 .. 20), where the diagonal scored 5 + 2 x 21 = 47 >= 19 x 2, the seed's score: it dies, the read finishes.  K + 1
    characters of the genome: the sub-k seed's node is the second k-mer's (the ordinary look-up)."""
    g, G = main_world()
    rows = [(plain(p, K) + _other(G[p + K]), 0) for p in (100, 237, 3100, 3500)] + [(plain(100, K + 1), 0)]
    return _rows(g, cli(), rows)


def cigar_runs():
    """code 20: `n_runs >= LANE_MAX_RUNS` when a run begins.  250 characters with substitutions 28 apart (27, 55, ...): n of them
    inside the read give 2 n + 1 runs.  7: 15 runs.  7 and the last character (a mismatch there scores -3 + 5, the end bonus: it is
    aligned): 16 runs, the array is full and the read finishes.  8: the 17th run: 20."""
    base = plain(2400, 250)
    subs = [27 + 28 * i for i in range(8)]
    return _rows(main_world()[0], cli(), [(_sub(base, *subs[:7]), 0), (_sub(base, *(subs[:7] + [249])), 0), (_sub(base, *subs), 20), (base, 0)])


CIGAR_RUNS = [15, 16, 17, 1]                 # the oracle's CIGAR runs for the reads of cigar_runs()


def backward(**kw):
    """reads with a substitution in the first 16 characters (too few in front of it for a sub-k seed): the seed starts behind
    it and the forward alignment inside the query, so the lane keeps the read for the backward pass (LR_AGAIN) and finishes it"""
    return _rows(main_world()[0], cli(**kw), [(_sub(plain(100 + 10 * p), p), 0) for p in (0, 1, 2, 3, 5, 8, 15)] + [(plain(100), 0)])


def min_path_score(mps):
    """code 31.  L = 100, a substitution at 5: the forward alignment (seed at 6) scores 94 x 2 + 5 = 193, the backward pass can
    reach 5 + 5 x 2 - 3 + 94 x 2 + 5 = 205.  min_path_score = 206: the forward alignment is not added (193 < 206) and no cell of
    the backward pass is a start cell: 31.  205: the backward pass's last column is one, the lane finishes the read.  A plain
    read (score 210) is aligned either way; one of 60 characters (130) finishes without an alignment."""
    return _rows(main_world()[0], cli(min_path_score=mps), [(_sub(plain(100), 5), 31 if mps > 205 else 0), (plain(300), 0), (plain(300, 60), 0), (rc(plain(200)), 0)])


# ---- label-aware ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def label_world():
    """label 0 on G[0:1000], 1 on G[1000:2000] (the k-mers across 1000 have none), 2 and 3 on G[2000:2600], none behind; a SNP at 400
    whose other allele has no label, one at 1400 whose other allele has labels 1 and 2"""
    rng = random.Random(7010)
    G = rand_seq(rng, 3000)
    alt = [G[p - K + 1:p] + _other(G[p]) + G[p + 1:p + K] for p in (400, 1400)]
    g = orc.Graph.build(K, [G] + alt, 0, False)
    anno = orc.Annotation(g, 4)
    anno.annotate(G[0:1000], 0)
    anno.annotate(G[1000:2000], 1)
    anno.annotate(G[2000:2600], 2)
    anno.annotate(G[2000:2600], 3)
    anno.annotate(alt[1], 1)
    anno.annotate(alt[1], 2)
    return g, anno, G


def labels():
    """code 30: a seed on a node without a label (G[2700:2800]); on a node with two (G[2100:2200]); seeds of two labels (a
    substitution at 1000 of G[950:1050]: no k-mer across the boundary is matched); a column whose row is not { L } (G[940:1040]
    unchanged: one seed, first node { 0 }, the columns reach the unlabeled k-mers); a fork child with two labels (G[1350:1450]).
    The staying side: the fork at 400, whose other child has no label and is no child."""
    g, anno, G = label_world()
    rows = [(G[100:200], 0), (G[2700:2800], 30), (G[2100:2200], 30), (_sub(G[950:1050], 50), 30), (G[940:1040], 30), (G[1350:1450], 30),
            (G[350:450], 0), (rc(G[1100:1200]), 0)]
    return _rows(g, cli(), rows, annotation=anno)


# ---- batch shapes (the launch code of mgx.hip / mgx_lane.hip), all in the main world with the CLI's configuration -------------------

def plain_reads(n):
    lo, hi = CLEAN
    out = []
    for i in range(n):
        p = lo + (i * 7) % (hi - lo - 100)
        out.append(plain(p) if i % 2 == 0 else rc(plain(p)))
    return [(r, 0) for r in out]


def backward_reads(n):
    lo, hi = CLEAN
    return [(_sub(plain(lo + (i * 11) % (hi - lo - 100)), 1 + i % 15), 0) for i in range(n)]


def leavers(n):
    """reads that leave, six codes in turn: 5, 10, 28, 19, 27, 3 (each as in its case above, shifted by a few characters)"""
    G = main_world()[1]
    third = _other(G[SNP_TIE], _other(G[SNP_TIE]))
    kinds = [lambda j: (plain(CLEAN[0] + j)[:60 + j] + "N" + plain(CLEAN[0] + j)[61 + j:], 5),
             lambda j: (plain(FORK3 - 70 + j), 10),
             lambda j: (plain(570 - j, 130), 28),
             lambda j: (plain(CLEAN[0] + j, 50) + plain(3000 + j, 50), 19),
             lambda j: (plain(SNP_TIE - 70 + j)[:70 - j] + third + plain(SNP_TIE - 70 + j)[71 - j:], 27),
             lambda j: (G[TWIN[0] + 20 + j:TWIN[0] + 120 + j], 3)]
    return [kinds[i % 6]((i // 6) % 10) for i in range(n)]


def _shape(rows):
    return _rows(main_world()[0], cli(), rows)


def shape_n(n):
    """n reads, mixed: of six, three plain, one with a backward pass, two that leave"""
    pl, bw, lv = plain_reads(n), backward_reads(n), leavers(n)
    return _shape([pl[i] if i % 6 in (0, 1, 3) else bw[i] if i % 6 == 4 else lv[i // 2] for i in range(n)])


def shape_all_leave(n=70):
    return _shape(leavers(n))


def shape_none_leave(n=70):
    return _shape(plain_reads(n))


def shape_backward_mixed(n=70):
    pl, bw = plain_reads(n), backward_reads(n)
    return _shape([bw[i] if i % 2 == 0 else pl[i] for i in range(n)])


def layout_batch(L, n=96):
    """reads of one length from the feature-free end of the genome, four kinds in turn: plain; from the other strand; three
    substitutions 60 (L = 100: 30) apart (7 CIGAR runs, the later seeds die on the path); a chimera whose second half comes from
    the genome's start.  The chimera's first seed is extended along the genome's one path, at most L + 11 nodes forward; the
    second seed's nodes lie 1800 characters back and cannot be in the table: the seed lives, 19.  (Behind the junction the read
    mismatches the genome at random; the places, (i * 17 + 5) % 350, are ones where no chance alignment there widens the band
    past the window first, which would be code 16 — that much was found by running the host model, not derived.)
    The batch's longest read sets max_cols, hash_slots and both strides of the lane scratch."""
    d = 60 if L > 200 else 30
    out = []
    for i in range(n):
        p = 2400 + (i * 13) % (1500 - L)
        r = plain(p, L)
        out.append([(r, 0), (rc(r), 0), (_sub(r, 25, 25 + d, 25 + 2 * d), 0), (r[:L // 2] + plain(CLEAN[0] + (i * 17 + 5) % 350, L - L // 2), 19)][i % 4])
    return _shape(out)


ONE_WAVEFRONT_READS = 64 * 5 + 37

CASES = {
    "no_seeds": no_seeds,
    "second_strand": second_strand,
    "second_strand_rel0": second_strand_rel0,
    "invalid_character": invalid_character,
    "seed_limit": seed_limit,
    "many_seeds": many_seeds,
    "root_window_57": lambda: root_window(57),
    "root_window_56": lambda: root_window(56),
    "cell_arena_root_204": lambda: cell_arena_root(204),
    "cell_arena_root_208": lambda: cell_arena_root(208),
    "cell_arena_2336": lambda: cell_arena(2336),
    "cell_arena_2332": lambda: cell_arena(2332),
    "max_columns": max_columns,
    "three_way_fork": three_way_fork,
    "tandem_repeat": tandem_repeat,
    "wide_rows_126_32": lambda: wide_rows(126, -32),
    "wide_rows_126_33": lambda: wide_rows(126, -33),
    "wide_rows_125_32": lambda: wide_rows(125, -32),
    "bubbles": bubbles,
    "ties": ties,
    "tie_size_cap_1.07": lambda: tie_size_cap(1.07),
    "tie_size_cap_1.075": lambda: tie_size_cap(1.075),
    "merged_vector": merged_vector,
    "later_seed": later_seed,
    "later_seeds_16_17": later_seeds_16_17,
    "cigar_runs": cigar_runs,
    "backward": backward,
    "left_trim_off": lambda: backward(allow_left_trim=0),
    "min_path_score_206": lambda: min_path_score(206),
    "min_path_score_205": lambda: min_path_score(205),
    "labels": labels,
    "shape_1": lambda: shape_n(1),
    "shape_63": lambda: shape_n(63),
    "shape_64": lambda: shape_n(64),
    "shape_65": lambda: shape_n(65),
    "shape_129": lambda: shape_n(129),
    "shape_357": lambda: shape_n(ONE_WAVEFRONT_READS),
    "shape_all_leave": shape_all_leave,
    "shape_none_leave": shape_none_leave,
    "shape_backward_mixed": shape_backward_mixed,
    "layout_250": lambda: layout_batch(250),
    "layout_100": lambda: layout_batch(100),
}
