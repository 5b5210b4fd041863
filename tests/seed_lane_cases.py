"""Directed worlds for the lane-per-read seeder (metagraph_amd/csrc/seed_lane.hpp; TEST INFRASTRUCTURE): one builder per case, each
a small graph and a few reads whose fate in the seeder follows from the guards of seed_lane_read() / sl_strand().  The host
model pins the fate per read (tests/test_seed_lane_edges.py), the GPU tests compare the kernel's histogram with it
(tests/test_gpu_seed_lane_edges.py).

A builder returns Case(graph, config, limits or None, reads, expected, first_pass):
  expected[i]    the SL_LEAVE code read i goes to the wave-per-read seeder with after both passes, 0 = a lane seeds it;
  first_pass     {i: code} for the reads whose fate in the FIRST pass is pinned too (0 = the first pass seeds it): the
                 boundary pairs of the small buffers, checked under MGX_EMU_SEEDLANE_ONE=1.
Everything is deterministic: the genomes come from seeded generators, the reads are cut from them by rule.

The codes (SL_LEAVE(code) in seed_lane.hpp) and where they are reached:
  1  read length          lengths_*: L < k, L > 255 (the long build's max_l)
  2  n != L - k + 1 || n > SL_MAX_KMERS: NOT REACHABLE.  Code 1 has let through k <= L <= 255 only; the mapping stage writes
     node_begin as the running sum of max(L - k + 1, 0) per read, so n == L - k + 1 <= 255 - 3 + 1 < 256.  Nothing asserted.
  3  characters outside ACGT        invalid_characters  (a lower-case character is NOT one: the packing folds case).  The
     reverse complement's invalid-character words are the forward strand's mirrored, so a read has such a character on both
     strands or on none: testing the forward strand's words alone would give the same answers — not observable from any read.
  4  DUST, first pass only (the second pass has the exact map and never leaves with 4)     dust_islands, shapes
  5  alt_total > lim.max_alt: NOT REACHABLE.  derive_limits() sets max_alt = max(4096, max_seeds); a strand has at most
     SL_PENDING_2_LONG = 256 pending records of at most 4 nodes each (the `cnt >= 4` guard), so alt_total <= 1024 < 4096.
     For the same reason `>` against `>=` in that guard cannot be observed.  Nothing asserted.
  6  more buffer entries than lim.max_seeds      seed_limit  (mgx_limits.max_seeds lowered)
  7  buffer entries / pending records   entries_32, pending_8, pending_144, many_192, many_288
  8  a strand below min_exact_match with matched k-mers, first pass only      partial_match (MGX_EMU_SEEDLANE_ONE=1)
  9  a look-up that finds no range: NOT REACHED by any case here, and not proven unreachable.  A pending record of kind 1
     carries k_map's own range for k_map's own match length, kind 2 is tested when it is listed, kind 4 is a matched k-mer's
     node, kind 3 walks the last characters of a matched last k-mer, which that k-mer's node ends with — each looks safe, but
     the argument that succ_last() of such a range always lands inside the graph is not finished.  Nothing asserted.
 12  a range without a real incoming edge     contig_start (the first characters of a contig: only the dummy path ends with them)
 13  more than four / max_num_seeds_per_locus nodes      repeat_nodes
 14  `dup && !(fl & 8)`: NOT REACHABLE.  dup needs bits 2 and 4 of the record's flags (a tail position, a seed at the last
     k-mer); sl_strand sets bit 8 exactly when both are set (expect_dup = i >= n && mem_at_last).  Nothing asserted.
"""
import collections
import functools
import random

import orc
from metagraph_amd import capi
from test_emu_vs_oracle import rand_seq, rc

Case = collections.namedtuple("Case", "graph config limits reads expected first_pass")


def _other(c, avoid=""):
    return next(x for x in "TGCA" if x != c and x not in avoid)


def _junk(rng, n, first="T"):
    """characters that match nothing planted: a random string that starts with `first`"""
    return first + rand_seq(rng, n - 1)


def _rows(graph, cfg, limits, rows):
    """rows: (read, expected) or (read, expected, first-pass code)"""
    return Case(graph, cfg, limits, [r[0] for r in rows], [r[1] for r in rows], {i: r[2] for i, r in enumerate(rows) if len(r) > 2})


# ---- the common world: k = 31, a random genome with low-complexity islands and a repeat in five contexts ----------------------

REPEAT_LEN = 24
# (no island is the reverse complement of another or of itself: a read's other strand must not match k-mers by accident)
ISLANDS = [(1000, "A", 30), (1400, "AC", 32), (1800, "C", 28), (2200, "AG", 30)]
REPEAT_AT = [3000, 3400, 3800, 4200, 4600]


@functools.lru_cache(maxsize=None)
def main_world():
    rng = random.Random(6001)
    G = list(rand_seq(rng, 6000))
    for at, unit, n in ISLANDS:
        for x in range(n):
            G[at + x] = unit[x % len(unit)]
    R = rand_seq(random.Random(6002), REPEAT_LEN)
    for j, at in enumerate(REPEAT_AT):
        # (the characters around a copy are never T: a read puts T there, so that its match is the repeat and no more)
        G[at - 1] = "ACG"[j % 3]
        G[at:at + REPEAT_LEN] = R
        G[at + REPEAT_LEN] = "GCA"[j % 3]
    G = "".join(G)
    return orc.Graph.build(31, [G], 0, False), G, R


def plain_reads(n, L=100, first=100, step=7):
    """n reads of the genome's island-free start ... a lane of the first pass seeds each"""
    G = main_world()[1]
    out = []
    for i in range(n):
        p = first + (i * step) % 700
        out.append(G[p:p + L] if i % 2 == 0 else rc(G[p:p + L]))
    return out


def island_reads(n, L=100):
    """reads across a low-complexity island: the first pass's quick scan cannot clear them (4), the second pass seeds them"""
    G = main_world()[1]
    out = []
    for i in range(n):
        at, _, ln = ISLANDS[i % len(ISLANDS)]
        p = at - 20 - (i // len(ISLANDS)) % 30
        out.append(G[p:p + L] if i % 2 == 0 else rc(G[p:p + L]))
    return out


def partial_reads(n, L=100):
    """40 characters of the genome, the rest random: matched k-mers on a strand below min_exact_match — the first pass leaves
    it (8), the second pass seeds it"""
    G = main_world()[1]
    rng = random.Random(6003)
    return [G[200 + 11 * i:240 + 11 * i] + _junk(rng, L - 40, _other(G[240 + 11 * i])) for i in range(n)]


def invalid_reads(n, L=100):
    G = main_world()[1]
    return [G[300 + 5 * i:300 + 5 * i + 50] + "N" + G[351 + 5 * i:300 + 5 * i + L] for i in range(n)]


def repeat_read(i=0):
    """genome, T, the repeat, junk: the repeat's position reports a sub-k seed whose range holds five nodes (13 in both passes)"""
    _, G, R = main_world()
    rng = random.Random(6004 + i)
    p = 500 + 13 * (i % 30)
    return G[p:p + 100] + "T" + R + _junk(rng, 12)


def island_repeat_read(i=0):
    """the same behind an island: the first pass leaves with 4 (DUST comes before the look-ups), the second with 13"""
    _, G, R = main_world()
    rng = random.Random(6104 + i)
    at = ISLANDS[i % len(ISLANDS)][0]
    return G[at - 20 - i % 7:at + 85] + "T" + R + _junk(rng, 12)


def lengths_short():
    """code 1 at k: L = k - 1, k, k + 1, the empty read; L = 160 is the longest read of the six-word build.  (L = k: the one MEM
    starts at the last k-mer, so each of the k - 1 - min_seed_length = 11 tail positions behind it is listed as expected to add
    nothing: more than SL_PENDING_1 records — the second pass seeds the read)"""
    g, G, _ = main_world()
    rows = [(G[100:130], 1), (G[100:131], 0, 7), (G[100:132], 0, 0), ("", 1), (G[700:860], 0, 0), (rc(G[100:131]), 0, 7), ("ACGT", 1)]
    return _rows(g, capi.config_cli(31), None, rows)


def lengths_long():
    """L = 160 and 161 in one batch (the nine-word build: both seeded), 255 the longest a lane takes, 256 and 300 leave"""
    g, G, _ = main_world()
    rows = [(G[700:860], 0, 0), (G[700:861], 0, 0), (G[300:555], 0, 0), (G[300:556], 1, 1), (G[300:600], 1, 1), (rc(G[300:555]), 0, 0),
            (G[100:130], 1)]
    return _rows(g, capi.config_cli(31), None, rows)


def lengths_k32():
    rng = random.Random(6010)
    G = rand_seq(rng, 1500)
    g = orc.Graph.build(32, [G], 0, False)
    rows = [(G[50:82], 0, 7), (G[50:81], 1), (G[50:83], 0, 0), (rc(G[400:500]), 0, 0)]
    return _rows(g, capi.config_cli(32), None, rows)


def invalid_characters():
    """code 3: an N in the first, a middle, the last packed word — at the word boundaries; a read of exactly one word and of one
    word and a character"""
    g, G, _ = main_world()
    base = G[300:400]
    rows = [(base[:p] + "N" + base[p + 1:], 3, 3) for p in (0, 31, 32, 63, 64, 99)]
    rows += [(base[:p] + "n" + base[p + 1:], 3, 3) for p in (50,)]
    rows += [(base[:31] + "N", 3, 3), ("N" + base[1:32], 3, 3), (base[:32] + "N", 3, 3), (base[:31] + "N" + base[32], 3, 3)]
    rows += [(base[:40] + base[40:60].lower() + base[60:], 0, 0), (base, 0, 0), (base[:32], 0, 0), (base[:33], 0, 0)]
    return _rows(g, capi.config_cli(31), None, rows)


def dust_islands(filter_on=1, min_seed_length=19):
    """code 4: sub-k seeds (min_seed_length < k) on strands with a homopolymer or dinucleotide island; without the filter the first
    pass seeds the same reads"""
    g = main_world()[0]
    cfg = capi.config_cli(31)
    cfg.min_seed_length = min_seed_length
    cfg.seed_complexity_filter = filter_on
    rows = [(r, 0, 4 if filter_on else 0) for r in island_reads(16)] + [(r, 0, 0) for r in plain_reads(4)]
    return _rows(g, cfg, None, rows)


def partial_match():
    """code 8 (first pass only)"""
    g = main_world()[0]
    rows = [(r, 0, 8) for r in partial_reads(6)] + [(r, 0, 0) for r in plain_reads(3)]
    return _rows(g, capi.config_cli(31), None, rows)


# ---- look-ups ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def repeats_world():
    """k = 21: repeats of 15 characters planted in 2, 4 and 5 contexts (each a contig of its own: 6 random characters, the
    repeat, a character that is not T)"""
    rng = random.Random(6020)
    G = rand_seq(rng, 3000)
    reps = {m: rand_seq(rng, 15) for m in (2, 4, 5)}
    seqs = [G]
    for m, R in reps.items():
        for j in range(m):
            seqs.append(rand_seq(rng, 30) + "ACG"[j % 3] + R + "GCA"[j % 3] + rand_seq(rng, 30))
    return orc.Graph.build(21, seqs, 0, False), G, reps


def repeat_nodes(per_locus=1000):
    """codes 13 and the look-ups that succeed: a sub-k position whose range holds two, four and five nodes; against
    max_num_seeds_per_locus = 1, 2 and the default"""
    g, G, reps = repeats_world()
    cfg = capi.config_cli(21)
    cfg.min_seed_length = 12
    cfg.max_num_seeds_per_locus = per_locus
    rng = random.Random(6021)
    rows = []
    for m in (2, 4, 5):
        read = G[100 * m:100 * m + 70] + "T" + reps[m] + _junk(rng, 10)
        rows.append((read, 0 if m <= min(4, per_locus) else 13))
    rows += [(G[900:1000], 0, 0)]
    return _rows(g, cfg, None, rows)


def tail_positions(many=1):
    """the ":240-244" rule: with one seed per k-mer every tail position behind the last k-mer's seed is expected to add nothing
    — the usual read; a read whose last 15 characters end another contig too has a tail position that reports after all"""
    rng = random.Random(6030)
    G = rand_seq(rng, 2500)
    other = rand_seq(rng, 40) + _other(G[684]) + G[685:700]         # ... ends with the read's last 15 characters
    g = orc.Graph.build(21, [G, other + "A"], 0, False)
    cfg = capi.config_cli(21)
    cfg.min_seed_length = 12
    if many:
        cfg.max_seed_length = 21
    rows = [(G[600:700], 0, 0), (G[1000:1100], 0, 0), (rc(G[1000:1100]), 0, 0), (G[1200:1221], 0, 0), (G[1200:1222], 0, 0)]
    return _rows(g, cfg, None, rows)


TAIL_REPORTS = [(85, 15, 6), (85, 15, 6)]          # the oracle's sub-k seeds (clipping, length, offset) of read 0 of tail_positions(1)


def contig_start():
    """code 12: the read's sub-k match is the first 15 characters of a contig — the range is the dummy path's node, without a
    real incoming edge"""
    rng = random.Random(6040)
    G = rand_seq(rng, 2500)
    C = rand_seq(rng, 80)
    g = orc.Graph.build(21, [G, C], 0, True)
    cfg = capi.config_cli(21)
    cfg.min_seed_length = 12
    read = G[100:170] + _other(G[170]) + C[:15] + _junk(rng, 10, _other(C[15]))
    return _rows(g, cfg, None, [(read, 12), (G[300:400], 0, 0)])


# ---- limits ---------------------------------------------------------------------------------------------------------------------

def seed_limit(lowered=True):
    """code 6: one seed per k-mer and sub-k seeds, k = 21, min_seed_length = 15: a read of L characters on its strand has
    L - 20 seeds and 5 tail positions listed as expected to add nothing: L - 15 buffer entries for L - 20 seeds.  max_seeds = 85:
    L = 100 fills the limit, L = 101 is one above — and the wave program, which counts seeds, still has room"""
    rng = random.Random(6050)
    G = rand_seq(rng, 2500)
    g = orc.Graph.build(21, [G], 0, False)
    cfg = capi.config_cli(21)
    cfg.min_seed_length = 15
    cfg.max_seed_length = 21
    lim = None
    if lowered:
        lim = capi.Limits()
        lim.max_seeds = 85
    rows = [(G[400:500], 0, 0), (G[400:501], 6 if lowered else 0, 6 if lowered else 0), (rc(G[800:900]), 0, 0),
            (rc(G[800:901]), 6 if lowered else 0, 6 if lowered else 0), (G[1200:1260], 0, 0)]
    return _rows(g, cfg, lim, rows)


# ---- buffer sizes ---------------------------------------------------------------------------------------------------------------

def _mem_read(G, p, n_mems, k):
    """n_mems stretches of k characters of G from p on, a substituted character between them: one MEM of one k-mer each"""
    out = []
    for j in range(n_mems):
        a = p + j * (k + 1)
        out.append(G[a:a + k])
        if j + 1 < n_mems:
            out.append(_other(G[a + k]))
    return "".join(out)


def entries_32():
    """SL_SEEDS_1 = 32: min_seed_length = k = 9, so every buffer entry is a MEM and there are no pending records; the graph
    holds both strands of the genome's first 200 characters and the forward strand only of the rest.  16 stretches from the
    first part: 16 + 16 entries; 17 stretches from the second: 17 + 0; 17 stretches that end in the first part ... see the
    oracle's seed counts, which the test asserts: 32, 33, 34"""
    rng = random.Random(6068)
    G = rand_seq(rng, 420)
    g = orc.Graph.build(9, [G, rc(G[:200])], 0, False)
    cfg = capi.config_cli(9)
    cfg.min_exact_match = 0.0
    r32 = _mem_read(G, 20, 16, 9)                  # G[20 .. 179]: both strands
    r33 = _mem_read(G, 40, 17, 9)                  # G[40 .. 209]: the last stretch (G[200 ..]) on the forward strand only
    r34 = _mem_read(G, 15, 17, 9)                  # G[15 .. 184]
    return _rows(g, cfg, None, [(r32, 0, 0), (r33, 0, 7), (r34, 0, 7), (_mem_read(G, 210, 17, 9), 0, 0)])


ENTRIES_32_SEEDS = [32, 33, 34, 17]                # the oracle's seeds per read of entries_32(), both strands


@functools.lru_cache(maxsize=None)
def _singles_world(k, m, n_pos, seed):
    """a read of n_pos + k - 1 random characters and a graph that holds, per k-mer position i of it, one contig of k characters
    that ends with read[i : i + m]: every position matches exactly m < k characters, so every position reports a sub-k seed"""
    rng = random.Random(seed)
    read = rand_seq(rng, n_pos + k - 1)
    seqs = [rand_seq(rng, k - m - 1) + _other(read[i - 1] if i else "A") + read[i:i + m] for i in range(n_pos)]
    return orc.Graph.build(k, seqs, 0, False), read


def pending_8():
    """SL_PENDING_1 = 8: reads with 8 and with 9 reporting sub-k positions (stretches of 14 characters, k = 21,
    min_seed_length = 12, no k-mer matches)"""
    rng = random.Random(6071)
    G = rand_seq(rng, 2500)
    g = orc.Graph.build(21, [G], 0, False)
    cfg = capi.config_cli(21)
    cfg.min_seed_length = 12

    def read(p, n):
        out = []
        for j in range(n):
            a = p + 15 * j
            out.append(G[a:a + 14] + _other(G[a + 14]))
        return "".join(out) + _junk(rng, 8)
    return _rows(g, cfg, None, [(read(100, 8), 0, 0), (read(400, 9), 0, 7), (read(700, 7), 0, 0)])


def pending_144():
    """SL_PENDING_2 = 144: k = 16, min_seed_length = 12, every position of the read that has 12 characters and a contig of its own
    reports (the tail positions too: the last k-mer is not matched, so they are walked): min(145, L - 11) records.  L = 155: 144
    fill the second pass's records, L = 156: one too many; L = 19 and 20: 8 and 9 for the first pass"""
    g, read = _singles_world(16, 12, 145, 6080)
    cfg = capi.config_cli(16)
    cfg.min_seed_length = 12
    return _rows(g, cfg, None, [(read[:155], 0, 7), (read[:156], 7, 7), (read, 7, 7), (read[:19], 0, 0), (read[:20], 0, 7)])


@functools.lru_cache(maxsize=None)
def _both_strands_world():
    rng = random.Random(6090)
    G = rand_seq(rng, 1200)
    return orc.Graph.build(11, [G, rc(G[:600])], 0, False), G


def many_192():
    """SL_SEEDS_1_MANY = SL_SEEDS_2 = 192: one seed per k-mer (max_seed_length = k = 11), both strands in the graph:
    2 * (L - 10) entries — L = 106: 192, the first pass seeds it; L = 107: 194, both passes leave it; a read of 107 whose last k-mer
    is on the forward strand only: 97 + 96 = 193, both leave it"""
    g, G = _both_strands_world()
    cfg = capi.config_cli(11)
    cfg.max_seed_length = 11
    rows = [(G[100:206], 0, 0), (G[100:207], 7, 7), (G[494:601], 7, 7), (rc(G[100:206]), 0, 0), (G[700:860], 0, 0)]
    return _rows(g, cfg, None, rows)


def many_288():
    """the same in a batch with a read of more than 160 characters (SL_SEEDS_1_MANY_LONG = SL_SEEDS_2_LONG = 288): L = 154: 288
    entries, seeded; L = 155: 290; L = 155 with 145 + 144 = 289"""
    g, G = _both_strands_world()
    cfg = capi.config_cli(11)
    cfg.max_seed_length = 11
    rows = [(G[100:254], 0, 0), (G[100:255], 7, 7), (G[446:601], 7, 7), (G[100:207], 0, 0), (G[700:900], 0, 0)]
    return _rows(g, cfg, None, rows)


# ---- batch shapes (the launch code of mgx.hip / mgx_seedlane.hip) -------------------------------------------------------------

def _shape(rows):
    return _rows(main_world()[0], capi.config_cli(31), None, rows)


def _leavers(n):
    """reads that leave both passes: the first with 4 and with other codes (front and back of the list), the second with 1, 3, 13"""
    inv = invalid_reads(n)
    kinds = [lambda i: ("ACGT" * (i % 7), 1, 1), lambda i: (inv[i], 3, 3), lambda i: (repeat_read(i), 13, 13),
             lambda i: (island_repeat_read(i), 13, 4)]
    return [kinds[i % 4](i) for i in range(n)]


def _second_pass_reads(n):
    """reads the first pass leaves and the second seeds: by 4 (front) and by 8 (back)"""
    isl, par = island_reads(n), partial_reads(n)
    return [(isl[i], 0, 4) if i % 2 == 0 else (par[i], 0, 8) for i in range(n)]


def shape_n(n):
    """n reads, mixed: two of three seeded by the first pass"""
    pl, lv, sp = plain_reads(n), _leavers(n), _second_pass_reads(n)
    return _shape([(pl[i], 0, 0) if i % 3 < 2 else (lv[i] if i % 2 else sp[i]) for i in range(n)])


def shape_all_leave_first(n=130):
    """every read leaves the first pass: the front and back lists meet and fill the list exactly; the second pass seeds them"""
    return _shape(_second_pass_reads(n))


def shape_all_leave_both(n=130):
    """... and every read leaves the second pass too: the wave-per-read seeder takes the whole batch"""
    return _shape(_leavers(n))


def shape_none_leave(n=130):
    return _shape([(r, 0, 0) for r in plain_reads(n)])


def shape_lanes(which):
    """64 reads of which lane 0, lane 63 or every other lane leaves (both passes)"""
    pl, lv = plain_reads(64), _leavers(64)
    leave = {"first": lambda i: i == 0, "last": lambda i: i == 63, "odd": lambda i: i % 2 == 1}[which]
    return _shape([lv[i] if leave(i) else (pl[i], 0, 0) for i in range(64)])


def shape_short_between():
    """empty reads and reads shorter than k between seeded ones"""
    pl = plain_reads(40)
    rows = []
    for i in range(40):
        rows.append((pl[i], 0, 0))
        rows.append([("", 1, 1), ("ACGTAC", 1, 1), (pl[i][:30], 1, 1)][i % 3])
    return _shape(rows)


# the cases whose first_pass is checked with the first pass alone (tests/test_seed_lane_edges.py): all but the batch shapes
def first_pass_cases():
    return [n for n in CASES if not n.startswith("shape_")]


CASES = {
    "lengths_short": lengths_short,
    "lengths_long": lengths_long,
    "lengths_k32": lengths_k32,
    "invalid_characters": invalid_characters,
    "dust_islands": dust_islands,
    "dust_islands_msl12": lambda: dust_islands(1, 12),
    "dust_islands_unfiltered": lambda: dust_islands(0),
    "partial_match": partial_match,
    "repeat_nodes": repeat_nodes,
    "repeat_nodes_per_locus_1": lambda: repeat_nodes(1),
    "repeat_nodes_per_locus_2": lambda: repeat_nodes(2),
    "tail_positions_many": tail_positions,
    "tail_positions_mems": lambda: tail_positions(0),
    "contig_start": contig_start,
    "seed_limit": seed_limit,
    "seed_limit_default": lambda: seed_limit(False),
    "entries_32": entries_32,
    "pending_8": pending_8,
    "pending_144": pending_144,
    "many_192": many_192,
    "many_288": many_288,
    "shape_1": lambda: shape_n(1),
    "shape_63": lambda: shape_n(63),
    "shape_64": lambda: shape_n(64),
    "shape_65": lambda: shape_n(65),
    "shape_129": lambda: shape_n(129),
    "shape_all_leave_first": shape_all_leave_first,
    "shape_all_leave_both": shape_all_leave_both,
    "shape_none_leave": shape_none_leave,
    "shape_lane_0": lambda: shape_lanes("first"),
    "shape_lane_63": lambda: shape_lanes("last"),
    "shape_every_other_lane": lambda: shape_lanes("odd"),
    "shape_short_between": shape_short_between,
}
