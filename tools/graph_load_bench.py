#!/usr/bin/env python3
"""Loading a `.dbg` file: mgx_graph_load_dbg (the file decoded on one host thread) against mgx_graph_load_dbg_device (the payloads
decoded by kernels), on a valid graph from the project's synthetic builder (metagraph_amd.synth, as bench.py and
tools/map_bench.py use it) written in SMALL and in STAT state.

tests/sdsl_writer.py states the layout with Python integers and takes minutes beyond a few hundred thousand edges, so the files
are written by the numpy functions below — the same layout, checked byte for byte against sdsl_writer on a small table before
anything is measured.  In one process, after a warm-up of each, --repeats timed calls of either loader, alternating; the split
of a call comes from the pieces on their own: reading the file, the host reader (mgx_boss_file_read: read + decode), the hook
mgx_boss_file_decode_device (read + upload + kernels + W / last copied back), and mgx_graph_create as the rest of the old call.
Exit status 1 if the new call's range reaches the old call's.

  python tools/graph_load_bench.py --out profiles/graph_load_bench.json
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdsl_writer as sw  # noqa: E402

le, be = sw.le, sw.be


# ---- the layout of tests/sdsl_writer.py over numpy arrays ---------------------------------------------------------------------
def _words(bits):
    raw = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").tobytes()
    return raw + b"\0" * (-len(raw) % 8)


def bit_vector(bits):
    return le(len(bits)) + _words(bits)


def int_vector(vals, width):
    vals = np.asarray(vals, dtype=np.uint64)
    bits = ((vals[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1) if width else np.zeros(0, np.uint8)
    return le(len(vals) * width) + bytes([width]) + _words(bits)


def select_support_mcl(args, n_bits):
    args = np.asarray(args, dtype=np.int64)
    cnt = len(args)
    out = le(cnt)
    if not cnt:
        return out
    sb = (cnt + 4095) >> 12
    logn = ((n_bits + 63) // 64 * 64).bit_length()
    out += int_vector(args[::4096], logn)
    kinds = [i % 2 == 0 for i in range(sb)] if sb > 1 else []
    out += bit_vector(np.array(kinds, dtype=np.uint8))
    parts = []
    for i in range(sb):
        mine = args[i << 12:(i + 1) << 12]
        if not kinds or kinds[i]:
            rel = mine[::64] - mine[0]
            parts.append(int_vector(np.concatenate([rel, np.zeros(64 - len(rel), np.int64)]), max(1, int(rel.max()).bit_length())))
        else:
            parts.append(int_vector(np.concatenate([mine, np.zeros(4096 - len(mine), np.int64)]), logn))
    return out + b"".join(parts)


_BINOM = np.array([[comb(n, j) if j <= n else 0 for j in range(64)] for n in range(63)], dtype=np.uint64)
_WIDTH = np.array([0 if comb(63, k) == 1 else comb(63, k).bit_length() for k in range(64)], dtype=np.int64)


def rrr_vector63(bits):
    bits = np.asarray(bits, dtype=np.uint8)
    n = len(bits)
    n_blocks = n // 63 + 1
    padded = np.zeros(n_blocks * 63, np.uint8)
    padded[:n] = bits
    blk = padded.reshape(n_blocks, 63)
    bt = blk.sum(axis=1, dtype=np.int64)
    widths = _WIDTH[bt]
    nr = np.zeros(n_blocks, np.uint64)
    p_row = (62 - np.arange(63))[None, :]
    for a in range(0, n_blocks, 1 << 16):                     # in slabs: the per-bit temporaries stay small
        b, k = blk[a:a + (1 << 16)].astype(np.int64), bt[a:a + (1 << 16)]
        inv = 2 * k > 63
        b = np.where(inv[:, None], 1 - b, b)
        k = np.where(inv, 63 - k, k)
        left = k[:, None] - (np.cumsum(b, axis=1) - b)        # ones left, the bit itself included
        term = np.where(b == 1, _BINOM[p_row, np.clip(left, 0, 63)], np.uint64(0))
        nr[a:a + (1 << 16)] = term.sum(axis=1, dtype=np.uint64)
    pos = np.concatenate([[0], np.cumsum(widths)])
    total = int(pos[-1])
    parts = []
    for a in range(0, n_blocks, 1 << 16):
        m = ((nr[a:a + (1 << 16), None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
        parts.append(m[np.arange(64)[None, :] < widths[a:a + (1 << 16), None]])
    btnr = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if n_blocks == 1 and total < 64:
        btnr = np.concatenate([btnr, np.zeros(64 - total, np.uint8)])
    ones_before = np.concatenate([[0], np.cumsum(bt)])
    ones = int(ones_before[-1])
    ptrs = pos[:-1][::32]
    ranks = np.concatenate([ones_before[:-1][::32], [ones]])
    return (le(n) + int_vector(bt, 6) + bit_vector(btnr) + int_vector(ptrs, max(1, total.bit_length())) + int_vector(ranks, max(1, ones.bit_length())))


def bit_vector_stat(bits):
    ones = np.flatnonzero(bits)
    return bit_vector(bits) + be(len(ones)) + sw.rank_support_v5(len(bits)) + select_support_mcl(ones, len(bits))


def wt_huff(seq, rrr):
    seq = np.asarray(seq, dtype=np.uint8)
    counts = {int(s): int(c) for s, c in enumerate(np.bincount(seq)) if c}
    nodes, queue = [], [(sw._huffman(counts), 0xFFFF, seq)]
    while queue:
        t, parent, sub = queue.pop(0)
        idx = len(nodes)
        nodes.append({"t": t, "parent": parent, "child": [0xFFFF, 0xFFFF], "bits": None})
        if parent != 0xFFFF:
            ch = nodes[parent]["child"]
            ch[0 if ch[0] == 0xFFFF else 1] = idx
        if t[0] == "inner":
            mask = np.isin(sub, list(sw._members(t[2])))
            nodes[idx]["bits"] = mask.astype(np.uint8)
            queue.append((t[1], idx, sub[~mask]))
            queue.append((t[2], idx, sub[mask]))
    at = ones = 0
    for nd in nodes:
        nd["bv_pos"], nd["ones_before"] = at, ones
        if nd["bits"] is not None:
            at += len(nd["bits"])
            ones += int(nd["bits"].sum())
    bits = np.concatenate([nd["bits"] for nd in nodes if nd["bits"] is not None])
    out = le(len(seq)) + le(len(counts))
    if rrr:
        out += rrr_vector63(bits)
    else:
        out += (bit_vector(bits) + sw.rank_support_v(len(bits)) + select_support_mcl(np.flatnonzero(bits), len(bits))
                + select_support_mcl(np.flatnonzero(bits == 0), len(bits)))
    out += le(len(nodes))
    c_to_leaf, path = [0xFFFF] * 256, [0] * 256
    for i, nd in enumerate(nodes):
        leaf = nd["t"][0] == "leaf"
        out += le(nd["bv_pos"]) + le(nd["t"][1] if leaf else nd["ones_before"]) + struct.pack("<HHH", nd["parent"], *nd["child"])
        if leaf:
            c_to_leaf[nd["t"][1]] = i
            chain, v = [], i
            while nodes[v]["parent"] != 0xFFFF:
                chain.append(1 if nodes[nodes[v]["parent"]]["child"][1] == v else 0)
                v = nodes[v]["parent"]
            word = 0
            for ln, b in enumerate(reversed(chain)):
                word |= b << ln
            path[nd["t"][1]] = word | (len(chain) << 56)
    return out + struct.pack("<256H", *c_to_leaf) + struct.pack("<256Q", *path)


def dbg_file(k, W, last, F, mode, state):
    logsigma = (len(F) - 1).bit_length() + 1
    out = be(len(F)) + b"".join(be(int(x)) for x in F) + be(k - 1) + be(state)
    if state == sw.STATE_SMALL:
        out += wt_huff(W, True) + be(logsigma) + be(sw.CODE_RRR) + rrr_vector63(last)
    else:
        out += wt_huff(W, False) + be(logsigma) + bit_vector_stat(last)
    return out + be(mode) + be(0) + sw.sd_vector(0, [])


def check_writer():
    """the numpy writer against tests/sdsl_writer.py, byte for byte, on tables small enough for the latter"""
    rng = np.random.default_rng(9)
    for n in (1, 62, 63, 64, 126, 5000, 9000):
        W = rng.integers(0, 10, size=n).astype(np.uint8)
        last = (rng.random(n) < (0.2, 0.5, 0.97)[n % 3]).astype(np.uint8)
        assert rrr_vector63(last) == sw.rrr_vector63(last.tolist()), ("rrr", n)
        assert bit_vector_stat(last) == sw.bit_vector_stat(last.tolist()), ("stat", n)
        if n > 1:
            F = [0, 1, 1, 1, n - 1]
            for state in (sw.STATE_SMALL, sw.STATE_STAT):
                assert dbg_file(9, W, last, F, 0, state) == sw.dbg_file(9, W, last, F, mode=0, state=state), ("dbg", n, state)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=98_000_000, help="bench.py's graph by default (written in a few seconds per file)")
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-edges", type=int, default=104_000_000, help="the edge count the decode times are scaled to")
    ap.add_argument("--profile-only", action="store_true", help="write the files, call the new loader once per file and leave (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t = time.perf_counter()
    check_writer()
    print("writer equals tests/sdsl_writer.py on the small tables (%.1f s)" % (time.perf_counter() - t), file=sys.stderr)

    import torch
    from metagraph_amd import aligner, capi, synth
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    dev = torch.device("cuda:0")
    genome = synth.random_genome(args.genome, 20240501, dev)
    tensors = [genome[None, :]]
    if args.snps:
        tensors.append(synth.snp_windows(genome, args.snps, args.k, 20240502))
    boss = synth.build_boss(tensors, args.k)
    W_d, last_d = boss["W"].contiguous(), boss["last"].contiguous()
    W, last, F, n_edges = W_d.cpu().numpy(), last_d.cpu().numpy(), [int(x) for x in boss["F"]], int(boss["n_edges"])
    del genome, tensors, boss
    torch.cuda.empty_cache()
    scale = args.bench_edges / n_edges
    record = {"workload": {"graph_edges": n_edges, "k": args.k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                           "note": "synthetic graph of metagraph_amd.synth, measured at graph_edges; scaled_to_bench_edges_ms are these "
                                   "times times %.3f (linear in the edges), an extrapolation to %d edges, not a measurement" % (scale, args.bench_edges)}}
    tmp = tempfile.mkdtemp(prefix="graph_load_bench")

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def load(device_path):
        h = C.c_void_p()
        fn = lib.mgx_graph_load_dbg_device if device_path else lib.mgx_graph_load_dbg
        t_ms, rc = ms(lambda: fn(path.encode(), 0, C.byref(h)))
        assert rc == 0, lib.mgx_last_error()
        assert lib.mgx_graph_num_edges(h) == n_edges
        lib.mgx_graph_destroy(h)
        return t_ms

    def reader(on_device):
        f = capi.BossFile()
        t_ms, rc = ms(lambda: lib.mgx_boss_file_decode_device(path.encode(), 0, C.byref(f)) if on_device else lib.mgx_boss_file_read(path.encode(), C.byref(f)))
        assert rc == 0, lib.mgx_last_error()
        tables = (np.ctypeslib.as_array(f.W, shape=(n_edges + 1,)).copy(), np.ctypeslib.as_array(f.last, shape=(n_edges + 1,)).copy())
        lib.mgx_boss_file_free(C.byref(f))
        return t_ms, tables

    def create():                                                                  # mgx_graph_create over tables already in device memory
        t_ms, G = ms(lambda: aligner.Graph(args.k, (W_d.data_ptr(), n_edges + 1), (last_d.data_ptr(), n_edges + 1), F, on_device=True))
        G.close()
        return t_ms

    worse = False
    for name, state in (("small", sw.STATE_SMALL), ("stat", sw.STATE_STAT)):
        path = os.path.join(tmp, name + ".dbg")
        t_write, data = ms(lambda: dbg_file(args.k, W, last, F, 0, state))
        with open(path, "wb") as f:
            f.write(data)
        del data
        if args.profile_only:
            load(True)
            continue
        (_, host_tables), (_, dev_tables) = reader(False), reader(True)            # warm-up of both readers, and their tables
        equal = all(np.array_equal(a, b) for a, b in zip(host_tables, dev_tables)) and np.array_equal(host_tables[0], W) and np.array_equal(host_tables[1], last)
        del host_tables, dev_tables
        load(False), load(True), create()                                          # warm-up of both loaders
        old, new, read_ms, host_reader, hook, created = [], [], [], [], [], []
        for _ in range(args.repeats):
            old.append(load(False))
            new.append(load(True))
            read_ms.append(ms(lambda: open(path, "rb").read())[0])
            host_reader.append(reader(False)[0])
            hook.append(reader(True)[0])
            created.append(create())
        o, nw, rd, hr, hk, cr = spread(old), spread(new), spread(read_ms), spread(host_reader), spread(hook), spread(created)
        host_decode = hr["median"] - rd["median"]
        device_decode = nw["median"] - cr["median"] - rd["median"]
        record[name] = {
            "file_bytes": os.path.getsize(path), "write_s": t_write / 1e3, "tables_equal": bool(equal),
            "mgx_graph_load_dbg_ms": o, "mgx_graph_load_dbg_device_ms": nw, "speedup_median": o["median"] / nw["median"],
            "pieces_ms": {"file_read": rd, "mgx_boss_file_read (read + host decode)": hr,
                          "mgx_boss_file_decode_device (read + upload + kernels + W / last copied back)": hk,
                          "mgx_graph_create over device tables": cr},
            "split_of_the_medians_ms": {
                "mgx_graph_load_dbg": {"file_read": rd["median"], "decode": host_decode, "upload_of_W_and_last": o["median"] - hr["median"] - cr["median"],
                                       "mgx_graph_create": cr["median"]},
                "mgx_graph_load_dbg_device": {"file_read": rd["median"], "upload_and_decode": device_decode, "mgx_graph_create": cr["median"]}},
            "scaled_to_bench_edges_ms": {"host_decode": host_decode * scale, "device_upload_and_decode": device_decode * scale,
                                         "mgx_graph_load_dbg": o["median"] * scale, "mgx_graph_load_dbg_device": nw["median"] * scale},
        }
        worse |= not equal or nw["max"] >= o["min"]
    if args.profile_only:
        return
    print(json.dumps(record))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")
    sys.exit(1 if worse else 0)


if __name__ == "__main__":
    main()
