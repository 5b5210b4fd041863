"""Test infrastructure: the `.dbg` files at which a piece of the on-device decode (csrc/dbg_decode.hpp) can go wrong, written with
tests/sdsl_writer.py — the smallest shapes per piece.  Shared by tests/test_dbg_decode_model.py (the kernel bodies on the host,
under sanitizers) and tests/test_gpu_dbg_decode.py (the kernels).  Every function returns [(name, file bytes)]; the properties a
case is there for are asserted where it is built."""
import numpy as np

import sdsl_writer as sw

HEADER = 8 + 5 * 8 + 8 + 8                       # F (count + 5 entries), k, state: where W begins in a DNA graph file


def table(rng, n, symbols=10):
    W = rng.integers(0, symbols, size=n).astype(np.uint8)
    W[0] = 0
    W[-1] = symbols - 1                           # (at least two symbols: a tree of three nodes or more)
    return W


def dbg(W, last, k=9, **kw):
    n = len(W)
    assert len(last) == n
    return sw.dbg_file(k, W, last, [0, 1, 1, 1, n - 1], **kw)


def rrr_cases():
    """`last` as an rrr_vector<63> of 2, 62, 63, 64, 126, 127, 4032 and 4033 bits (no valid file holds a vector of one bit: W has
    two symbols or more, hence two elements), random, all zero and all one; blocks of classes 0, 1, 31, 32, 62 and 63 — both
    sides of the complement rule — with numbers that lie across two words of btnr"""
    rng = np.random.default_rng(1)
    out = []
    for n in (2, 62, 63, 64, 126, 127, 4032, 4033):
        for fill in ("random", "zeros", "ones"):
            last = {"random": (rng.random(n) < 0.5).astype(np.uint8), "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8)}[fill]
            out.append(("rrr_%d_%s" % (n, fill), dbg(table(rng, n), last)))
    bits = []
    for k in [0, 1, 31, 32, 62, 63] * 3 + [31, 31, 32, 32, 30, 33, 1, 62]:
        blk = [1] * k + [0] * (63 - k)
        rng.shuffle(blk)
        bits += blk
    widths = [0 if k in (0, 63) else sw.comb(63, k).bit_length() for k in [sum(bits[b:b + 63]) for b in range(0, len(bits), 63)]]
    offs = np.concatenate([[0], np.cumsum(widths)])
    assert any(o // 64 != (o + w - 1) // 64 for o, w in zip(offs, widths) if w)
    out.append(("rrr_classes", dbg(table(rng, len(bits)), bits)))
    return out


def wt_cases(state):
    """two symbols (three nodes); all ten symbols of W with geometric counts (a tree nine levels deep) and a symbol that occurs
    once; sequences of 2, 63, 64 and 65 elements, and 65 and 129 level bits: one beyond a word of the rank directory"""
    rng = np.random.default_rng(2)
    out = []
    for n in (2, 63, 64, 65, 129):
        W = (rng.random(n) < 0.4).astype(np.uint8) * 3       # symbols 0 and 3 only: n level bits
        W[0], W[-1] = 0, 3
        out.append(("wt2_%d" % n, dbg(W, rng.integers(0, 2, size=n), state=state)))
    geo = np.concatenate([np.full(2 ** (9 - s) if s < 9 else 1, s, dtype=np.uint8) for s in range(10)])      # 512, 256, ..., 2, 1
    assert len(set(geo.tolist())) == 10 and (geo == 9).sum() == 1
    rng.shuffle(geo)
    paths = np.frombuffer(sw.wt_huff(geo.tolist(), True)[-2048:], dtype=np.uint64).tolist()
    assert max(p >> 56 for p in paths) == 9
    out.append(("wt_geo", dbg(geo, rng.integers(0, 2, size=len(geo)), state=state)))
    for n in (63, 64, 65, 1000):
        out.append(("wt10_%d" % n, dbg(table(rng, n), rng.integers(0, 2, size=n), state=state)))
    return out


def _sd_wl0(size, inverted):
    """bit_vector_sd with wl = 0, which the reader takes for a vector without stored positions only"""
    body = (sw.le(size) + bytes([0]) + sw.le(0) + bytes([0]) + sw.bit_vector([0, 0]) + sw.select_support_mcl([], 2) + sw.select_support_mcl([0, 1], 2))
    return sw.be(sw.CODE_SD) + body + bytes([1 if inverted else 0])


def sd_cases():
    """`last` as an sd_vector: wl > 0 (the writer's) and wl = 0; ones at positions 0 and size - 1; an empty word of `high`
    between two ones; the inverted flag"""
    rng = np.random.default_rng(3)
    out = []
    n = 32767
    last = np.zeros(n, np.uint8)
    last[:32] = 1
    last[-32:] = 1
    ones = np.flatnonzero(last).tolist()
    wl = n.bit_length() - len(ones).bit_length()
    assert wl > 0 and {((p >> wl) + i) >> 6 for i, p in enumerate(ones)} == {0, 2}       # word 1 of high is empty
    W = table(rng, n)
    out.append(("sd_gap", dbg(W, last, last_code=sw.CODE_SD)))
    out.append(("sd_gap_inverted", dbg(W, 1 - last, last_code=sw.CODE_SD)))              # the same positions, stored inverted
    for n in (2, 64, 65, 777):
        for p in (0.1, 0.9):
            last = (rng.random(n) < p).astype(np.uint8)
            last[0] = last[-1] = 1
            out.append(("sd_%d_%d" % (n, int(p * 10)), dbg(table(rng, n), last, last_code=sw.CODE_SD)))
    for inverted in (False, True):
        n = 100
        W = table(rng, n)
        data = dbg(W, [0] * n)
        head = HEADER + len(sw.wt_huff(W.tolist(), True)) + 8
        tail = data[head + len(sw.adaptive([0] * n, sw.CODE_RRR)):]
        out.append(("sd_wl0_%d" % inverted, data[:head] + _sd_wl0(n, inverted) + tail))
    return out


def fast_cases():
    """FAST state: int_vectors of 15, 16 and 17 four-bit elements (within a word, exactly one word, one element into the next)"""
    rng = np.random.default_rng(4)
    return [("fast_%d" % n, dbg(table(rng, n), rng.integers(0, 2, size=n), state=sw.STATE_FAST)) for n in (15, 16, 17, 1000)]


def boundary_cases():
    return rrr_cases() + wt_cases(sw.STATE_SMALL) + wt_cases(sw.STATE_STAT) + sd_cases() + fast_cases()
