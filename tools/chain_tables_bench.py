#!/usr/bin/env python3
"""The chain stage of LabeledAligner's coordinate mode on a read batch (mgx_chain_tables_batch) on the bench graph:
bench.py's genome and SNP windows at k = 31, a --labels-label annotation with one coordinate per entry built as
tools/coord_load_bench.py builds it (label j on rows / labels + 30 random rows, 27-bit coordinates), --reads reads of --read-len bp
from pinned host memory.  One warm-up and --repeats timed calls with MGX_CHAIN_TABLES_ON_DEVICE (a host clock around the call,
which ends in a stream synchronise); next to it the handle's own times of the mapping and seeding stages of the same batch
(mgx_aligner_stats: device events), the part of the call this stage did not write, and what is left of the call.  Nothing at
the parent commit computes these tables, so there is no earlier figure to compare with and no threshold: recorded as measured.

Random labels cover a k-mer's width each, so under the command line's min_exact_match = 0.7 the filter drops nearly every label
and next to no anchor is left (2359 of them in the recorded run): the workload is run a second time with min_exact_match = 0,
where every (seed, label) pair becomes an anchor and the sort and the DP have work (lists of single-anchor label runs).  Both
are recorded, with what each exercised.

  python tools/chain_tables_bench.py --out profiles/chain_tables_bench.json
  rocprofv3 --kernel-trace --stats ... -- python tools/chain_tables_bench.py --profile-only      (one call per configuration)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true", help="one call per configuration and leave (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from metagraph_amd import aligner, capi, synth
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    genome = synth.random_genome(args.genome, 20240501, dev)
    tensors = [genome[None, :]]
    if args.snps:
        tensors.append(synth.snp_windows(genome, args.snps, args.k, 20240502))
    boss = synth.build_boss(tensors, args.k)
    del tensors
    n_edges = boss["n_edges"]
    W, last = boss["W"].contiguous(), boss["last"].contiguous()
    G = aligner.Graph(args.k, (W.data_ptr(), n_edges + 1), (last.data_ptr(), n_edges + 1), boss["F"], on_device=True)
    reads = synth.sample_reads(genome, args.reads, args.read_len, 20240503).contiguous()
    torch.cuda.synchronize()
    del genome
    # the annotation of tools/coord_load_bench.py, handed over as arrays: rows on the host, the coordinates through the device entry
    rng = np.random.default_rng(20240601)
    per = n_edges // args.labels + 30
    columns = [np.unique(rng.integers(0, n_edges, size=per)) for _ in range(args.labels)]
    col_begin = np.zeros(args.labels + 1, dtype=np.uint64)
    col_begin[1:] = np.cumsum([len(c) for c in columns])
    rows = np.concatenate(columns).astype(np.uint64)
    del columns
    n_entries = len(rows)
    coords = rng.integers(0, 1 << 27, size=n_entries).astype(np.int64)
    AN = aligner.Annotation.from_sparse(n_edges, col_begin, rows)
    rows_d = torch.from_numpy(rows.view(np.int64)).to(dev)
    coord_begin_d = torch.arange(n_entries + 1, dtype=torch.int64, device=dev)
    coords_d = torch.from_numpy(coords).to(dev)
    lib.mgx_annotation_set_coordinates_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib.mgx_annotation_set_coordinates_device(AN.h, args.labels, col_begin.ctypes.data, rows_d.data_ptr(), coord_begin_d.data_ptr(), coords_d.data_ptr())
    assert rc == 0, lib.mgx_last_error()
    del rows_d, coord_begin_d, coords_d, rows, coords
    torch.cuda.empty_cache()
    t_setup = time.perf_counter() - t0
    print("graph %d edges, annotation %d entries, %d reads: set up in %.1f s" % (n_edges, n_entries, args.reads, t_setup), file=sys.stderr)

    # the reads in pinned host memory
    n_bytes = args.reads * args.read_len
    pinned = lib.mgx_pinned_alloc(n_bytes)
    assert pinned, "mgx_pinned_alloc failed"
    host_reads = reads.cpu().numpy()
    C.memmove(pinned, host_reads.ctypes.data, n_bytes)
    del reads, host_reads
    torch.cuda.empty_cache()
    offsets = (np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.read_len))

    record = {"workload": {"reads": args.reads, "read_len": args.read_len, "k": args.k, "graph_edges": int(n_edges), "labels": args.labels,
                           "annotation_entries": int(n_entries), "coordinates_per_entry": 1, "repeats": args.repeats,
                           "device": torch.cuda.get_device_name(0), "reads_from": "pinned host memory", "setup_s": t_setup},
              "configurations": {}}
    for name, min_exact_match in (("cli (min_exact_match 0.7)", 0.7), ("min_exact_match 0", 0.0)):
        cfg = capi.config_cli(args.k)
        cfg.min_exact_match = min_exact_match
        S = aligner.SeedChainer(G, cfg, AN)
        t = capi.ChainTables()

        def call():
            t0 = time.perf_counter()
            rc = lib.mgx_chain_tables_batch(S.h, pinned, offsets.ctypes.data, args.reads, 0, capi.MGX_CHAIN_TABLES_ON_DEVICE, C.byref(t))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, lib.mgx_last_error()
            st = S.stats()
            return ms, st["seed_kernel_ms"], st["seeding_ms"]

        before = aligner.chain_tables_kernel_launch_counts()
        warm = call()
        after = aligner.chain_tables_kernel_launch_counts()
        print("%s: warm-up %.0f ms" % (name, warm[0]), file=sys.stderr)
        if args.profile_only:
            S.close()
            continue
        runs = [call() for _ in range(args.repeats)]
        for i, r in enumerate(runs):
            print("%s: repeat %d: call %.1f ms (mapping %.1f, seeding %.1f)" % (name, i, *r), file=sys.stderr)
        # what the batch exercised: the totals of the last call (the tables' begins are on the device: their last entries)
        n_lists = 2 * args.reads
        totals = {}
        hip = C.CDLL("libamdhip64.so")
        for key, ptr in (("kept_seeds", t.seed_begin), ("anchors", t.list_begin)):
            buf = (C.c_uint64 * 1)()
            assert hip.hipMemcpy(buf, C.c_void_p(C.cast(ptr, C.c_void_p).value + 8 * n_lists), C.c_size_t(8), 2) == 0      # device to host
            totals[key] = int(buf[0])
        call_ms = [r[0] for r in runs]
        map_ms, seeding_ms = [r[1] for r in runs], [r[2] for r in runs]
        rest = [r[0] - r[1] - r[2] for r in runs]
        record["configurations"][name] = {
            "mgx_chain_tables_batch_ms": spread(call_ms), "mapping_stage_ms": spread(map_ms), "seeding_stage_ms": spread(seeding_ms),
            "call_minus_mapping_and_seeding_ms": spread(rest),
            "share_of_the_call_outside_mapping_and_seeding": spread([x / c for x, c in zip(rest, call_ms)]),
            "reads_per_s": args.reads / (spread(call_ms)["median"] / 1e3), "totals": totals,
            "launch_counts_of_one_call": [a - b for a, b in zip(after, before)]}
        S.close()
    lib.mgx_pinned_free(pinned)
    if args.profile_only:
        return
    print(json.dumps(record))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
