"""`align --map --count-kmers` on the benchmark workload: the per-read (discovered, k-mers, distinct) triples two ways.

  baseline  mgx_map_batch (both strands mapped, two node arrays copied to the host and widened to 64 bit) + counting on the
            host with numpy (count_nonzero; sort of every row, neighbour compare) — what a caller had to do before
            mgx_map_summary_batch existed;
  new       mgx_map_summary_batch in counts mode (BASIC graph: forward strand only, 12 bytes per read to the host);
  sub-k     mgx_map_summary_batch with --sub-k L (k_map_subk), no baseline.

Same synthetic workload as bench.py (metagraph_amd.synth), reads in pinned host memory, 1 warm-up + --repeats timed calls per
leg; wall clock per call, and the mapping kernels' share from the library's HIP events (mgx_stats.seed_kernel_ms).  Both legs run
on the same --reads (the baseline's host vectors are 32 bytes per k-mer: 10 M reads do not fit every host).  The triples of
the two legs are compared on every read.  Prints one JSON line; --out writes it to a file as well.

  python tools/map_bench.py --reads 2000000 --out profiles/map_summary_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/map_bench.py --reads 2000000 --repeats 2 --no-baseline   (per-kernel times)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metagraph_amd import aligner, capi, synth  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / xs[len(xs) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sub-k", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    dev = torch.device("cuda:0")
    genome = synth.random_genome(args.genome, 20240501, dev)
    tensors = [genome[None, :]]
    if args.snps:
        tensors.append(synth.snp_windows(genome, args.snps, args.k, 20240502))
    boss = synth.build_boss(tensors, args.k)
    del tensors
    n_edges = boss["n_edges"]
    W, last = boss["W"].contiguous(), boss["last"].contiguous()
    G = aligner.Graph(args.k, (W.data_ptr(), n_edges + 1), (last.data_ptr(), n_edges + 1), boss["F"], on_device=True)
    reads_h = synth.sample_reads(genome, args.reads, args.read_len, 20240503).contiguous().cpu().pin_memory()
    offsets_h = (torch.arange(args.reads + 1, dtype=torch.int64) * args.read_len).contiguous().pin_memory()
    del genome, boss, W, last
    torch.cuda.empty_cache()
    A = aligner.Aligner(G, capi.config_cli(args.k))
    n, nk = args.reads, args.read_len - args.k + 1

    def summary(map_length):
        m = capi.MapSummary()
        rc = lib.mgx_map_summary_batch(A.h, C.c_void_p(reads_h.data_ptr()), C.c_void_p(offsets_h.data_ptr()), n, 0, map_length, 0, C.byref(m))
        assert rc == 0, lib.mgx_last_error()
        return np.ctypeslib.as_array(C.cast(m.counts, C.POINTER(C.c_uint32)), shape=(n, 3)).copy()

    def baseline():
        m = capi.Mapping()
        rc = lib.mgx_map_batch(A.h, C.c_void_p(reads_h.data_ptr()), C.c_void_p(offsets_h.data_ptr()), n, 0, C.byref(m))
        assert rc == 0, lib.mgx_last_error()
        t = time.perf_counter()
        fwd = np.ctypeslib.as_array(m.nodes_fwd, shape=(n, nk))            # reads of one length: a rectangle
        out = np.empty((n, 3), dtype=np.uint32)
        for b in range(0, n, 1 << 18):                                     # in slabs: the sorted copy stays small
            s = np.sort(fwd[b:b + (1 << 18)], axis=1)
            out[b:b + len(s), 0] = np.count_nonzero(s, axis=1)
            out[b:b + len(s), 1] = nk
            out[b:b + len(s), 2] = (s[:, 0] != 0) + np.count_nonzero((s[:, 1:] != s[:, :-1]) & (s[:, 1:] != 0), axis=1)
        return out, (time.perf_counter() - t) * 1e3

    def timed(fn):
        fn()                                                               # warm-up (buffers grow on the first call)
        wall, kern, extra, res = [], [], [], None
        for _ in range(args.repeats):
            t = time.perf_counter()
            res = fn()
            wall.append((time.perf_counter() - t) * 1e3)
            kern.append(A.stats()["seed_kernel_ms"])
            if isinstance(res, tuple):
                res, host_ms = res
                extra.append(host_ms)
        return res, wall, kern, extra

    record = {"workload": {"reads": n, "read_len": args.read_len, "k": args.k, "graph_edges": int(n_edges), "repeats": args.repeats,
                           "device": torch.cuda.get_device_name(0)}}
    new, wall, kern, _ = timed(lambda: summary(0))
    record["summary_counts_mode"] = {"wall_ms": spread(wall), "mapping_kernels_ms": spread(kern),
                                     "reads_per_s": n / (spread(wall)["median"] * 1e-3)}
    if not args.no_baseline:
        base, wall, kern, host = timed(baseline)
        record["baseline_map_batch_plus_host_counting"] = {"wall_ms": spread(wall), "mapping_kernels_ms": spread(kern),
                                                           "host_counting_ms": spread(host),
                                                           "reads_per_s": n / (spread(wall)["median"] * 1e-3)}
        record["triples_equal_on_every_read"] = bool((base == new).all())
        record["speedup_wall"] = spread(wall)["median"] / record["summary_counts_mode"]["wall_ms"]["median"]
    if args.sub_k:
        sub, wall, _, _ = timed(lambda: summary(args.sub_k))
        record["sub_k"] = {"map_length": args.sub_k, "wall_ms": spread(wall), "reads_per_s": n / (spread(wall)["median"] * 1e-3),
                           "discovered_fraction": float(sub[:, 0].sum()) / float(sub[:, 1].sum())}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
