"""mgx_fetch_results on the benchmark workload with the pipeline option decode_on_device off and on, after ONE
mgx_align_batch_device:

  (off) records and stream copied to pageable vectors, HostResults::decode on one host thread (the default);
  (on)  k_decode_size, five scans, k_decode_write, the seven arrays of mgx_results copied to pinned host memory.

Same synthetic workload as bench.py (metagraph_amd.synth), reads in pinned host memory.  The two legs alternate in one process:
one warm-up call each, then --repeats timed calls each, wall clock per call.  The seven arrays of the two views are compared
before anything is reported.  The bytes each leg moves device-to-host are recorded: the on-leg's from the library's counter, the
off-leg's from the batch (64-byte records, the stream's used words, the 8-byte cursor).  The on-leg is also reported against the
bus: its bytes over the 57 GB/s pinned device-to-host rate of DESIGN.md 3.12.  Prints one JSON line; --out writes it to a file.

  python tools/decode_bench.py --reads 2000000 --out profiles/results_decode_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_bench.py --reads 2000000 --repeats 2 --only-on   (per-kernel times)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metagraph_amd import aligner, capi, synth  # noqa: E402

BUS_GB_S = 57.0            # pinned device-to-host copies, DESIGN.md 3.12


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / xs[len(xs) // 2]}


def arrays_of(res):
    a = capi.results_arrays(res)
    alns = a["alns"]
    out = [a["aln_begin"], a["status"], alns.view(np.uint8), a["nodes"], a["cigar"].view(np.uint8), a["seqs"]]
    nl = int(alns["n_labels"].sum()) if len(alns) else 0
    out.append(np.ctypeslib.as_array(res.labels, shape=(nl,)) if res.labels else np.zeros(0, dtype=np.uint32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-on", action="store_true", help="the option-on leg alone (for a profiler run)")
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
    n = args.reads
    del genome, boss, W, last
    torch.cuda.empty_cache()
    A = aligner.Aligner(G, capi.config_cli(args.k))
    rc = lib.mgx_align_batch_device(A.h, C.c_void_p(reads_h.data_ptr()), C.c_void_p(offsets_h.data_ptr()), n, 0)
    assert rc == 0, lib.mgx_last_error()

    def fetch(on):
        A.set_pipeline("decode_on_device=%d" % on)
        t = time.perf_counter()
        res = A.fetch()
        return res, (time.perf_counter() - t) * 1e3

    record = {"workload": {"reads": n, "read_len": args.read_len, "k": args.k, "graph_edges": int(n_edges), "repeats": args.repeats,
                           "device": torch.cuda.get_device_name(0)}}
    legs = (1,) if args.only_on else (0, 1)
    wall = {0: [], 1: []}
    # warm-up (buffers grow on the first call), and the comparison of the two views
    if not args.only_on:
        off = [x.copy() for x in arrays_of(fetch(0)[0])]
    before = aligner.decode_kernel_launch_counts()
    res_on, _ = fetch(1)
    after = aligner.decode_kernel_launch_counts()
    on_bytes = after[2] - before[2]
    on_arrays = arrays_of(res_on)
    if not args.only_on:
        assert all(np.array_equal(a, b) for a, b in zip(off, on_arrays)) and bool(res_on.labels) == (len(off[6]) > 0), "the two views differ"
        record["views_equal"] = True
        del off
    n_aln = int(on_arrays[0][-1])
    record["results"] = {"alignments": n_aln, "nodes": int(len(on_arrays[3])), "cigar_runs": int(len(on_arrays[4]) // 8),
                         "path_characters": int(len(on_arrays[5])), "labels": int(len(on_arrays[6]))}
    for _ in range(args.repeats):
        for on in legs:
            wall[on].append(fetch(on)[1])
    bound_ms = on_bytes / (BUS_GB_S * 1e9) * 1e3
    s_on = spread(wall[1])
    record["decode_on_device_1"] = {"wall_ms": s_on, "reads_per_s": n / (s_on["median"] * 1e-3), "device_to_host_bytes_per_call": int(on_bytes),
                                    "bytes_per_read": on_bytes / n, "bus_bound_ms_at_57_GB_s": bound_ms,
                                    "median_over_bus_bound": s_on["median"] / bound_ms}
    if not args.only_on:
        headers, stream = C.c_void_p(), C.c_void_p()
        hb, nq, words = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert lib.mgx_device_results(A.h, C.byref(headers), C.byref(hb), C.byref(nq), C.byref(stream), C.byref(words)) == 0
        off_bytes = 64 * n + 4 * words.value + 8
        s_off = spread(wall[0])
        record["decode_on_device_0"] = {"wall_ms": s_off, "reads_per_s": n / (s_off["median"] * 1e-3), "device_to_host_bytes_per_call": int(off_bytes),
                                        "bytes_per_read": off_bytes / n}
        record["speedup_wall_median"] = s_off["median"] / s_on["median"]
        record["on_range_wholly_below_off_range"] = bool(max(wall[1]) < min(wall[0]))
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
