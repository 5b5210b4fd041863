"""The text of `align --map` for a batch on the benchmark graph, two ways:

  baseline  mgx_map_summary_batch (MGX_MAP_WANT_NODES for the k-mer: node form: the node array comes to the host) + mgx_format_map
            query by query into one preallocated buffer (a C++ loop: tools/map_format_bench_host.cpp) — the only path before
            mgx_format_map_batch existed;
  new       mgx_map_summary_batch (MGX_MAP_KEEP_NODES) + mgx_format_map_batch (size kernel, scan, write kernel; the text and the
            n + 1 offsets to the host).

Legs: (a) the k-mer: node form on --nodes-reads reads (about 5 KB of text per 150-bp read), (b) --count-kmers on --reads reads,
(c) with --driver-dir DIR: `mgx_align --map` on those --nodes-reads reads as a FASTQ file against `--map --map-on-device
--parse-on-device`, whole processes (graph load and index build included), stdout to a file, the two files compared byte for
byte first, then 1 warm-up + --repeats runs each.  In (a) and (b) the new leg's range has to lie wholly below the old leg's:
the tool exits with status 1 when it does not.
Same synthetic workload as bench.py (metagraph_amd.synth), reads in pinned host memory; 1 warm-up + --repeats timed calls per
leg, wall clock per call (summary + text).  The two texts are compared before anything is reported.  Prints one JSON line; --out
writes it to a file as well.  --dump-driver-inputs DIR writes the graph as a flat BOSS dump and the --nodes-reads reads as FASTQ
for `mgx_align --map --time` (--driver-dir does that itself).

  python tools/map_format_bench.py --out profiles/map_format_bench.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/map_format_bench.py --repeats 2 --no-baseline   (per-kernel times)
"""
import argparse
import ctypes as C
import json
import os
import struct
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
    so = os.path.join(build, "map_format_bench_host.so")
    src = os.path.join(ROOT, "tools", "map_format_bench_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src, "-L" + build, "-lmgx", "-Wl,-rpath,$ORIGIN"], check=True)
    capi.lib()                                    # (libmgx.so first: the helper resolves against it)
    H = C.CDLL(so)
    H.map_format_bench_summary_and_format.restype = C.c_int64
    H.map_format_bench_summary_and_format.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                                      C.c_int, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p]
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--nodes-reads", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--dump-driver-inputs", default=None)
    ap.add_argument("--driver-dir", default=None, help="leg (c): a directory for the graph dump, the FASTQ and the two outputs")
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
    n_all = max(args.reads, args.nodes_reads)
    reads_h = synth.sample_reads(genome, n_all, args.read_len, 20240503).contiguous().cpu().pin_memory()
    offsets_h = (torch.arange(n_all + 1, dtype=torch.int64) * args.read_len).contiguous().pin_memory()
    hs = [b"read.%d" % i for i in range(n_all)]
    headers = b"".join(hs)
    hoff = np.zeros(n_all + 1, dtype=np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in hs])
    if args.driver_dir and not args.dump_driver_inputs:
        args.dump_driver_inputs = args.driver_dir
    if args.dump_driver_inputs:
        os.makedirs(args.dump_driver_inputs, exist_ok=True)
        with open(os.path.join(args.dump_driver_inputs, "bench.boss"), "wb") as f:
            f.write(struct.pack("<7Q", args.k, n_edges, *[int(x) for x in boss["F"]]))
            f.write(W.cpu().numpy().tobytes())
            f.write(last.cpu().numpy().tobytes())
        rd = reads_h.numpy().reshape(n_all, args.read_len)
        qual = b"I" * args.read_len
        with open(os.path.join(args.dump_driver_inputs, "bench_map.fq"), "wb") as f:
            for i in range(args.nodes_reads):
                f.write(b"@" + hs[i] + b"\n" + rd[i].tobytes() + b"\n+\n" + qual + b"\n")
    del genome, boss, W, last
    torch.cuda.empty_cache()
    A = aligner.Aligner(G, capi.config_cli(args.k))
    H = None if args.no_baseline else host_loop_lib()
    record = {"workload": {"read_len": args.read_len, "k": args.k, "graph_edges": int(n_edges), "repeats": args.repeats,
                           "device": torch.cuda.get_device_name(0)}}

    def timed(fn):
        fn()                                                               # warm-up (buffers grow on the first call)
        wall, res = [], None
        for _ in range(args.repeats):
            t = time.perf_counter()
            res = fn()
            wall.append((time.perf_counter() - t) * 1e3)
        return res, wall

    for name, fmt, n, per_read in (("nodes", capi.MGX_MAP_FMT_NODES, args.nodes_reads, 56 * (args.read_len - args.k + 1) + 64),
                                   ("count_kmers", capi.MGX_MAP_FMT_COUNT_KMERS, args.reads, 96)):
        flags = capi.MGX_MAP_KEEP_NODES if fmt == capi.MGX_MAP_FMT_NODES else 0

        def on_device():
            m, t = capi.MapSummary(), capi.Text()
            rc = lib.mgx_map_summary_batch(A.h, C.c_void_p(reads_h.data_ptr()), C.c_void_p(offsets_h.data_ptr()), n, 0, 0, flags, C.byref(m))
            assert rc == 0, lib.mgx_last_error()
            rc = lib.mgx_format_map_batch(A.h, headers, hoff.ctypes.data, fmt, 0.7, C.byref(t))
            assert rc == 0, lib.mgx_last_error()
            return t

        before = aligner.format_map_kernel_launch_counts()
        t, wall_b = timed(on_device)
        after = aligner.format_map_kernel_launch_counts()
        text_bytes = int(t.line_begin[n])
        leg = {"reads": n, "text_bytes": text_bytes,
               "summary_plus_format_map_batch": {"wall_ms": spread(wall_b), "reads_per_s": n / (spread(wall_b)["median"] * 1e-3),
                                                 "device_to_host_bytes_per_call": (after[2] - before[2]) // (args.repeats + 1),
                                                 "host_to_device_bytes_per_call": (after[3] - before[3]) // (args.repeats + 1)}}
        if H is not None:
            dev_text = np.frombuffer((C.c_char * text_bytes).from_address(t.text), dtype=np.uint8).copy()
            dev_lb = np.ctypeslib.as_array(t.line_begin, shape=(n + 1,)).copy()
            cap = n * per_read
            buf = np.empty(cap, dtype=np.uint8)
            lb_host = np.zeros(n + 1, dtype=np.uint64)

            def baseline():
                got = H.map_format_bench_summary_and_format(A.h, headers, hoff.ctypes.data, reads_h.data_ptr(), offsets_h.data_ptr(), n, args.k,
                                                            fmt, 0.7, buf.ctypes.data, cap, lb_host.ctypes.data)
                assert got >= 0, got
                return got

            got, wall_a = timed(baseline)
            # the two texts, before anything is reported
            assert got == text_bytes, (got, text_bytes)
            assert np.array_equal(dev_text, buf[:text_bytes]), "the two texts differ"
            assert np.array_equal(dev_lb, lb_host), "line_begin differs"
            leg["texts_equal"] = True
            leg["baseline_summary_plus_format_map_loop"] = {"wall_ms": spread(wall_a), "reads_per_s": n / (spread(wall_a)["median"] * 1e-3)}
            leg["speedup_wall_median"] = spread(wall_a)["median"] / spread(wall_b)["median"]
            leg["ranges_do_not_overlap"] = bool(max(wall_b) < min(wall_a))
            del buf, dev_text
        record[name] = leg
    if args.driver_dir and not args.no_baseline:
        del A, G
        torch.cuda.empty_cache()
        exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
        inputs = [os.path.join(args.dump_driver_inputs, "bench.boss"), os.path.join(args.dump_driver_inputs, "bench_map.fq")]
        legs = {"map": ["--map", "--time"], "map_on_device_parse_on_device": ["--map", "--map-on-device", "--parse-on-device", "--time"]}

        def process(name, out_path):
            t = time.perf_counter()
            with open(out_path, "wb") as fo:
                r = subprocess.run([exe] + inputs + legs[name], stdout=fo, stderr=subprocess.PIPE, timeout=600)
            assert r.returncode == 0, r.stderr
            return (time.perf_counter() - t) * 1e3

        outs = {name: os.path.join(args.driver_dir, name + ".txt") for name in legs}
        for name in legs:
            process(name, outs[name])                                      # warm-up, and the outputs to compare
        a, b = (open(outs[name], "rb").read() for name in legs)
        assert a == b and len(a) > 0, "the two processes print different bytes"
        driver = {"reads": args.nodes_reads, "stdout_bytes": len(a), "stdout_equal": True}
        del a, b
        wall = {name: [] for name in legs}
        for _ in range(args.repeats):                                      # interleaved: both legs see the same machine
            for name in legs:
                wall[name].append(process(name, outs[name]))
        for name in legs:
            driver[name] = {"wall_ms": spread(wall[name])}
            os.remove(outs[name])
        driver["speedup_wall_median"] = driver["map"]["wall_ms"]["median"] / driver["map_on_device_parse_on_device"]["wall_ms"]["median"]
        driver["ranges_do_not_overlap"] = bool(max(wall["map_on_device_parse_on_device"]) < min(wall["map"]))
        record["mgx_align_whole_process"] = driver
    print(json.dumps(record))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")
    bad = [name for name in ("nodes", "count_kmers") if record[name].get("ranges_do_not_overlap") is False]
    if bad:
        print("FAILED: the new leg's range does not lie below the old leg's in: " + ", ".join(bad), file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
