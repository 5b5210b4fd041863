"""A plain k-mer dictionary over a BOSS table (W, last, F).  TEST INFRASTRUCTURE ONLY.

The second, independent reference of the mapping tests: the oracle (oracle/) restates BOSS with rank / select, this module
does not.  It spells the k-mer of every edge with direct array operations and looks reads up in a dictionary, so a shared
misreading of the rank / select structure cannot pass both.  Pure numpy / Python: nothing of the project is imported.

The table, from its definition: edges 1 .. n (slot 0 unused) are sorted by their source node (k - 1 characters, co-lex: last
character most significant); W[i] % 5 is the edge's label in "$ACGT", W[i] >= 5 flags an edge that is not the first one into
its target; last[i] marks the last edge of its source node; F[c] is the number of edges whose node ends in a character < c.
The j-th node that ends in c is the target of the j-th unflagged edge labelled c — the one step every spelling needs.
"""
import numpy as np

BASIC, PRIMARY = 0, 2                       # graph modes (include/mgx.h: MGX_MODE_BASIC, MGX_MODE_PRIMARY)

# the DNA alphabet of the k-mer extractor: case-insensitive, U reads as T; every other byte is outside it
_CODE = np.full(256, 255, dtype=np.uint8)
for _chars, _c in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _chars:
        _CODE[ord(_ch)] = _c
_LETTERS = np.frombuffer(b"$ACGT", dtype=np.uint8)


def _node_chars(k, W, last, F):
    """-> (chars, label): chars[p][i] = character code (0 = '$', 1 .. 4 = ACGT) at position p of the source node of edge i,
    p = 0 .. k - 2; label[i] = W[i] % 5.  Index 0 of every array is the unused slot."""
    W = np.asarray(W, dtype=np.uint8)
    last = np.asarray(last, dtype=np.uint8)
    F = np.asarray([int(x) for x in F], dtype=np.int64)
    n = len(W) - 1
    idx = np.arange(n + 1, dtype=np.int64)
    # last character of the node of edge i: the largest c with F[c] < i
    node_last = (np.searchsorted(F, idx, side="left") - 1).clip(0, 4).astype(np.uint8)
    lb = last.astype(np.int64)
    lb[0] = 0
    cs = np.cumsum(lb)                                       # set `last` bits in 1 .. i
    rank = np.zeros(n + 1, dtype=np.int64)                   # the node of edge i is the rank[i]-th node
    rank[1:] = cs[:-1] + 1
    NF = cs[F]                                               # nodes that end in a character < c
    parent = idx.copy()                                      # an edge INTO the node of edge i ('$' nodes: none, see below)
    for c in range(1, 5):
        into = np.flatnonzero(W == c)
        sel = np.flatnonzero((node_last == c) & (idx >= 1))
        parent[sel] = into[rank[sel] - NF[c] - 1]
    chars = [None] * (k - 1)
    ptr = idx
    for r in range(k - 1):
        # a node that ends in '$' is all '$' before that too (a sentinel-prefixed dummy): it keeps pointing at itself
        chars[k - 2 - r] = node_last[ptr]
        if r < k - 2:
            ptr = parent[ptr]
    return chars, (W % 5).astype(np.uint8)


def spell_edges(k, W, last, F):
    """The k-mer of every BOSS edge whose spelling holds no '$'.
    k <= 32 -> (edges, keys): edge indices (ascending) and their k-mers as 2-bit packed uint64 (first character most
    significant, A C G T = 0 .. 3); k > 32 -> (edges, kmers) with `kmers` a list of bytes."""
    chars, label = _node_chars(k, W, last, F)
    n = len(label) - 1
    real = label != 0
    for c in chars:
        real &= c != 0
    real[0] = False
    edges = np.flatnonzero(real)
    if k <= 32:
        key = np.zeros(n + 1, dtype=np.uint64)
        for p, c in enumerate(chars):
            key |= (c.astype(np.uint64) - np.uint64(1)) << np.uint64(2 * (k - 1 - p))
        key |= label.astype(np.uint64) - np.uint64(1)
        return edges, key[edges]
    text = np.stack([_LETTERS[c[edges]] for c in chars] + [_LETTERS[label[edges]]], axis=1)
    return edges, [row.tobytes() for row in text]


def unpack_key(key, k):
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - p))) & 3] for p in range(k))


class KmerDict:
    """k-mer -> edge index; edges that `valid` masks out are absent."""

    def __init__(self, k, W, last, F, valid=None):
        self.k = k
        self.n = len(W) - 1
        edges, keys = spell_edges(k, W, last, F)
        if valid is not None:
            keep = np.asarray(valid)[edges] != 0
            edges = edges[keep]
            keys = keys[keep] if k <= 32 else [s for s, t in zip(keys, keep) if t]
        self.packed = k <= 32
        if self.packed:
            order = np.argsort(keys, kind="stable")
            self.keys, self.edges = keys[order], edges[order]
            assert not (self.keys[1:] == self.keys[:-1]).any(), "a k-mer spelled by two edges"
        else:
            self.table = dict(zip(keys, edges.tolist()))
            assert len(self.table) == len(keys), "a k-mer spelled by two edges"

    def __len__(self):
        return len(self.keys) if self.packed else len(self.table)

    def kmers(self):
        """-> list of (k-mer string, edge)"""
        if self.packed:
            return [(unpack_key(x, self.k), int(e)) for x, e in zip(self.keys, self.edges)]
        return [(s.decode(), e) for s, e in self.table.items()]

    def lookup(self, codes):
        """codes: uint8 array, 0 .. 3 or 255 (outside the alphabet) -> (edge, ident, ok) of every window of k codes: the edge
        or 0; the window's identity (packed key or bytes), only meant for comparing windows with one another; whether the
        window lies inside the alphabet"""
        k, L = self.k, len(codes)
        nk = L - k + 1
        if nk <= 0:
            return np.zeros(0, dtype=np.int64), [], np.zeros(0, dtype=bool)
        bad = np.concatenate(([0], np.cumsum(codes == 255)))
        ok = (bad[k:] - bad[:-k]) == 0
        out = np.zeros(nk, dtype=np.int64)
        if self.packed:
            c = np.where(codes == 255, 0, codes).astype(np.uint64)
            weights = np.uint64(1) << (np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64))
            win = np.lib.stride_tricks.sliding_window_view(c, k)
            key = (win * weights[None, :]).sum(axis=1, dtype=np.uint64)
            if len(self.keys):
                at = np.searchsorted(self.keys, key).clip(0, len(self.keys) - 1)
                hit = ok & (self.keys[at] == key)
                out[hit] = self.edges[at[hit]]
            return out, key, ok
        text = _LETTERS[np.where(codes == 255, 0, codes + 1)].tobytes()
        ident = [text[i:i + k] for i in range(nk)]
        for i in np.flatnonzero(ok):
            out[i] = self.table.get(ident[i], 0)
        return out, ident, ok


def encode(read):
    b = read if isinstance(read, bytes) else read.encode("latin-1")
    return _CODE[np.frombuffer(b, dtype=np.uint8)]


def reverse_complement_codes(codes):
    return np.where(codes == 255, 255, 3 - codes).astype(np.uint8)[::-1]


def map_reads(d, reads, mode=BASIC):
    """Per read (fwd, rev): the node of every k-mer of the read and of its reverse complement (each in its own strand's
    order), 0 where the k-mer is not in the dictionary or its window holds a byte outside the alphabet; a read shorter
    than k gives two empty lists.
    PRIMARY (the graph stores one k-mer of every reverse-complement pair and is queried as the canonical graph of 2 n ids): a
    k-mer found itself keeps its id a on its own strand; on the other strand that same id means the reverse complement, so the
    mirrored position holds a + n — unless the k-mer is its own reverse complement (even k), then a.  A k-mer found only as
    its reverse complement b is b + n on its own strand and b on the other."""
    out = []
    for read in reads:
        codes = encode(read)
        f, fid, _ = d.lookup(codes)
        r, rid, _ = d.lookup(reverse_complement_codes(codes))
        if mode == PRIMARY:
            nk = len(f)
            cf, cr = np.zeros(nk, dtype=np.int64), np.zeros(nk, dtype=np.int64)
            for i in range(nk):
                a, b = int(f[i]), int(r[nk - 1 - i])
                if a:
                    cf[i] = a
                    cr[nk - 1 - i] = a if fid[i] == rid[nk - 1 - i] else a + d.n
                elif b:
                    cf[i] = b + d.n
                    cr[nk - 1 - i] = b
            f, r = cf, cr
        out.append((f.tolist(), r.tolist()))
    return out
