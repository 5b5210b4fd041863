"""The `align --json` text of an alignment batch on the benchmark workload, two ways, both after the same mgx_align_batch_device:

  (a) baseline  mgx_fetch_results (records and stream to the host, decoded into five vectors) + mgx_format_json query by query
                into one preallocated buffer (a C++ loop: tools/json_format_bench_host.cpp) — the only path before
                mgx_format_json_batch existed; neither function is touched by the change that added the batch formatter;
  (b) new       mgx_format_json_batch over the whole batch (size kernel, scan, write kernel; the text and n + 1 offsets to the host).

Same synthetic workload as bench.py (metagraph_amd.synth), reads in pinned host memory; 1 warm-up + --repeats timed calls per
leg, wall clock per call.  The default is 200 000 reads of 150 bp: JSON text is several KB per such read (the record says how
many), so the text of that batch is of the order of a gigabyte and fits comfortably where ten times the reads would not.  The two
texts are compared before anything is reported.  Prints one JSON line; --out writes it to a file as well.

  python tools/json_format_bench.py --out profiles/format_json_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/json_format_bench.py --repeats 2 --no-baseline   (per-kernel times)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metagraph_amd import aligner, capi, synth  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / xs[len(xs) // 2]}


def host_loop_lib():
    build = os.path.join(ROOT, "metagraph_amd", "_build")
    so = os.path.join(build, "json_format_bench_host.so")
    src = os.path.join(ROOT, "tools", "json_format_bench_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src, "-L" + build, "-lmgx", "-Wl,-rpath,$ORIGIN"], check=True)
    capi.lib()                                    # (libmgx.so first: the helper resolves against it)
    H = C.CDLL(so)
    H.json_format_bench_fetch_and_format.restype = C.c_int64
    H.json_format_bench_fetch_and_format.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                                C.c_void_p, C.c_uint64, C.c_void_p]
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
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
    n = args.reads
    hs = [b"read.%d" % i for i in range(n)]
    headers = b"".join(hs)
    hoff = np.zeros(n + 1, dtype=np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in hs])
    del genome, boss, W, last
    torch.cuda.empty_cache()
    cfg = capi.config_cli(args.k)
    A = aligner.Aligner(G, cfg)
    rc = lib.mgx_align_batch_device(A.h, C.c_void_p(reads_h.data_ptr()), C.c_void_p(offsets_h.data_ptr()), n, 0)
    assert rc == 0, lib.mgx_last_error()

    def on_device():
        t = capi.Text()
        rc = lib.mgx_format_json_batch(A.h, headers, hoff.ctypes.data, 0, n, C.byref(t))
        assert rc == 0, lib.mgx_last_error()
        return t

    lb_host = np.zeros(n + 1, dtype=np.uint64)

    def baseline():
        got = H.json_format_bench_fetch_and_format(A.h, headers, hoff.ctypes.data, reads_h.data_ptr(), offsets_h.data_ptr(), n, args.k,
                                              buf.ctypes.data, cap, lb_host.ctypes.data)
        assert got > 0, got
        return got

    def timed(fn):
        fn()                                                               # warm-up (buffers grow on the first call)
        wall, res = [], None
        for _ in range(args.repeats):
            t = time.perf_counter()
            res = fn()
            wall.append((time.perf_counter() - t) * 1e3)
        return res, wall

    record = {"workload": {"reads": n, "read_len": args.read_len, "k": args.k, "graph_edges": int(n_edges), "repeats": args.repeats,
                           "device": torch.cuda.get_device_name(0)}}
    before = aligner.format_json_kernel_launch_counts()
    t, wall_b = timed(on_device)
    after = aligner.format_json_kernel_launch_counts()
    text_bytes = int(t.line_begin[n])
    record["format_json_batch"] = {"wall_ms": spread(wall_b), "reads_per_s": n / (spread(wall_b)["median"] * 1e-3), "text_bytes": text_bytes,
                                   "text_bytes_per_read": text_bytes / n, "text_gb_per_s": text_bytes / (spread(wall_b)["median"] * 1e-3) / 1e9,
                                   "device_to_host_bytes_per_call": (after[3] - before[3]) // (args.repeats + 1),
                                   "host_formatted_queries_per_call": (after[2] - before[2]) // (args.repeats + 1)}
    if not args.no_baseline:
        H = host_loop_lib()
        cap = text_bytes + 4096                                            # (the buffer of the host leg: the text's size is known by now)
        buf = np.empty(cap, dtype=np.uint8)
        got, wall_a = timed(baseline)
        # the two texts, before anything is reported
        assert got == text_bytes, (got, text_bytes)
        dev_text = np.frombuffer((C.c_char * text_bytes).from_address(t.text), dtype=np.uint8)
        assert np.array_equal(dev_text, buf[:text_bytes]), "the two texts differ"
        assert np.array_equal(np.ctypeslib.as_array(t.line_begin, shape=(n + 1,)), lb_host), "line_begin differs"
        record["texts_equal"] = True
        record["baseline_fetch_results_plus_format_json_loop"] = {
            "wall_ms": spread(wall_a), "reads_per_s": n / (spread(wall_a)["median"] * 1e-3),
            "note": "mgx_fetch_results and mgx_format_json are not touched by the change that added mgx_format_json_batch"}
        record["speedup_wall_median"] = spread(wall_a)["median"] / spread(wall_b)["median"]
        record["ranges_do_not_overlap"] = bool(max(wall_b) < min(wall_a))
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
