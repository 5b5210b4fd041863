"""FASTA / FASTQ text to the seqs / offsets arrays of mgx_align_batch, on the benchmark workload's reads (2 M x 150 bp sampled from the
bench genome) written once as a FASTQ file and once as a 60-column FASTA file:

  (a) new       mgx_parse_reads per call, from pinned host text (the text crosses the bus once; kernels do the rest).  Beside it:
                the same call on text that already lies in device memory — the difference is the host-to-device copy, stated as
                its share of a call — and the call preceded by read(2) of the file into the pinned buffer, which is what leg (b)
                starts from;
  (b) baseline  the parent's way: read_records (std::getline from the file, two strings per record) + the concatenation of
                HipDBGAligner::align_batch_device — tools/parse_bench_host.cpp, a host program;
  (c) driver    whole-process wall time of `mgx_align GRAPH FASTQ --format-on-device` with and without --parse-on-device on the
                bench graph (built here and written as a flat BOSS dump), the two outputs compared byte for byte first.

1 warm-up + --repeats timed runs per leg; median and range.  The arrays of (a) are compared with the reads before anything is
reported.  --kernel-stats CSV (a rocprofv3 --kernel-trace --stats file of a --profile-run) adds every parser kernel's time per call
and its bytes moved / time beside the 8 TB/s peak.  Prints one JSON line; --out writes it to a file as well.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o parse -- python tools/parse_bench.py --profile-run     (FASTQ, leg (a) only)
  python tools/parse_bench.py --kernel-stats DIR/.../parse_kernel_stats.csv --out profiles/parse_reads_bench.json
"""
import argparse
import csv
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metagraph_amd import aligner, capi, synth  # noqa: E402

HBM_PEAK_GB_S = 8000.0


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / xs[len(xs) // 2]}


def timed(fn, repeats):
    fn()                                                                       # warm-up (buffers grow on the first call)
    wall = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
    return wall


def kernel_record(path, text_bytes, n_lines, n_records, seq_bytes, name_bytes):
    """Per parser kernel: time per launch from a rocprofv3 stats file, and the bytes it has to move (the arrays it reads and writes
    once each — what its searches and the text's first / last bytes per line add is not counted) over that time."""
    spans = (text_bytes + 63) // 64
    must_move = {"k_parse_count": text_bytes + 12 * spans,                    # the text in; a mask and a count per 64-byte span out
                 "k_parse_table": 12 * spans + 4 * n_lines,                    # masks and scanned counts in; line_begin out
                 "k_parse_classify": 4 * n_lines + 16 * n_lines + name_bytes,  # line_begin in, one 16-byte item per line out, the header lines' names read
                 "k_parse_records": 20 * n_lines + 16 * n_records,             # scanned items + line_begin in; two offsets per record out
                 "k_parse_copy<0>": 2 * seq_bytes, "k_parse_copy<1>": 2 * name_bytes}
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            key = next((k for k in must_move if name.startswith("void " + k) or name.startswith(k)), None)
            if key is None and "scan" in name and "rocprim" in name:
                key = "hipcub scans (" + ("RpSum" if "RpSum" in name else "uint32") + "): " + name.split("detail::")[1].split("<")[0]
            if key is None:
                continue
            ms = float(row["AverageNs"]) * 1e-6
            e = {"calls": int(row["Calls"]), "ms_per_launch": ms, "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
            if key in must_move:
                e["bytes_moved"] = must_move[key]
                e["gb_per_s"] = must_move[key] / (ms * 1e-3) / 1e9
                e["share_of_hbm_peak_pct"] = 100.0 * e["gb_per_s"] / HBM_PEAK_GB_S
            out[key] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=98_000_000)
    ap.add_argument("--snps", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-run", action="store_true", help="FASTQ and leg (a) from pinned text only: the run to put under rocprofv3")
    ap.add_argument("--kernel-stats", default=None, help="the kernel stats CSV of a --profile-run with the same --reads / --read-len")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    dev = torch.device("cuda:0")
    genome = synth.random_genome(args.genome, 20240501, dev)
    n, L = args.reads, args.read_len
    rd = synth.sample_reads(genome, n, L, 20240503).contiguous().cpu().numpy().reshape(n, L)
    tmp = tempfile.mkdtemp()
    if not args.profile_run:
        tensors = [genome[None, :]]
        if args.snps:
            tensors.append(synth.snp_windows(genome, args.snps, args.k, 20240502))
        boss = synth.build_boss(tensors, args.k)
        del tensors
        n_edges = boss["n_edges"]
        with open(os.path.join(tmp, "bench.boss"), "wb") as f:
            f.write(struct.pack("<7Q", args.k, n_edges, *[int(x) for x in boss["F"]]))
            f.write(boss["W"].contiguous().cpu().numpy().tobytes())
            f.write(boss["last"].contiguous().cpu().numpy().tobytes())
        del boss
    del genome
    torch.cuda.empty_cache()
    names = [b"read.%d" % i for i in range(n)]
    qual = b"I" * L
    texts = {"fastq": b"".join(b"@" + names[i] + b"\n" + rd[i].tobytes() + b"\n+\n" + qual + b"\n" for i in range(n))}
    if not args.profile_run:
        texts["fasta60"] = b"".join(b">" + names[i] + b"\n" + b"\n".join(rd[i, c:c + 60].tobytes() for c in range(0, L, 60)) + b"\n" for i in range(n))
    record = {"workload": {"reads": n, "read_len": L, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}}
    P = aligner.ReadParser()
    for kind, text in texts.items():
        nb = len(text)
        path = os.path.join(tmp, "bench." + ("fq" if kind == "fastq" else "fa"))
        with open(path, "wb") as f:
            f.write(text)
        pinned = lib.mgx_pinned_alloc(nb)
        C.memmove(pinned, text, nb)
        out = capi.Reads()

        def call(ptr=pinned, on_device=0):
            rc = lib.mgx_parse_reads(P.h, ptr, nb, on_device, 1, 0, C.byref(out))
            assert rc == 0, lib.mgx_last_error()
        before = aligner.parse_kernel_launch_counts()
        wall = timed(call, args.repeats)
        after = aligner.parse_kernel_launch_counts()
        r = aligner.ParsedReads(P, out)
        seqs, offs = r.to_host()
        assert r.n_records == n and seqs == rd.tobytes() and r.names == b"".join(names), "the parsed arrays differ from the reads"
        med = spread(wall)["median"]
        rec = {"text_bytes": nb, "lines": text.count(b"\n"), "seq_bytes": n * L, "name_bytes": len(r.names),
               "parse_reads": {"wall_ms": spread(wall), "reads_per_s": n / (med * 1e-3), "text_gb_per_s": nb / (med * 1e-3) / 1e9,
                               "host_to_device_bytes_per_call": (after[2] - before[2]) // (args.repeats + 1),
                               "device_to_host_bytes_per_call": (after[3] - before[3]) // (args.repeats + 1)}}
        record[kind] = rec
        if args.profile_run:
            lib.mgx_pinned_free(pinned)
            continue
        # the same call on text that lies in device memory: what is left of a call without the copy over the bus
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        wall_d = timed(lambda: call(C.c_void_p(d_text.data_ptr()), 1), args.repeats)
        med_d = spread(wall_d)["median"]
        del d_text
        rec["parse_reads_text_on_device"] = {"wall_ms": spread(wall_d)}
        rec["host_to_device_copy"] = {"ms_per_call": med - med_d, "share_of_call_pct": 100.0 * (med - med_d) / med, "gb_per_s": nb / ((med - med_d) * 1e-3) / 1e9,
                                      "note": "median of the call from pinned host text minus median of the call on device text"}
        # read(2) of the file (page cache) into the pinned buffer, then the call: the same start as leg (b)
        view = memoryview((C.c_char * nb).from_address(pinned)).cast("B")

        def read_and_call():
            at = 0
            with open(path, "rb", buffering=0) as f:
                while at < nb:
                    got = f.readinto(view[at:])
                    assert got > 0
                    at += got
            call()
        wall_r = timed(read_and_call, args.repeats)
        med_r = spread(wall_r)["median"]
        rec["file_read_plus_parse_reads"] = {"wall_ms": spread(wall_r), "reads_per_s": n / (med_r * 1e-3)}
        del view
        lib.mgx_pinned_free(pinned)
        exe = os.path.join(ROOT, "metagraph_amd", "_build", "parse_bench_host")
        src = os.path.join(ROOT, "tools", "parse_bench_host.cpp")
        if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
            subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
        rows = [ln.split() for ln in subprocess.run([exe, path, str(args.repeats + 1)], capture_output=True, text=True, check=True).stdout.splitlines()]
        assert all(int(x[1]) == n and int(x[2]) == n * L for x in rows)
        wall_b = [float(x[0]) * 1e3 for x in rows[1:]]
        med_b = spread(wall_b)["median"]
        rec["baseline_read_records_plus_concatenation"] = {"wall_ms": spread(wall_b), "reads_per_s": n / (med_b * 1e-3),
                                                           "note": "reads the file itself; the file is in the page cache for every run, the warm-up included"}
        rec["speedup_wall_median"] = {"parse_reads_from_pinned_text": med_b / med, "file_read_plus_parse_reads": med_b / med_r,
                                      "note": "the baseline includes reading the file from the page cache; the second figure gives the new path the same start"}
        rec["ranges_do_not_overlap"] = bool(max(wall_r) < min(wall_b))
    if args.kernel_stats:
        f = record["fastq"]
        record["fastq"]["kernels"] = kernel_record(args.kernel_stats, f["text_bytes"], f["lines"], n, f["seq_bytes"], f["name_bytes"])
        record["fastq"]["kernels_note"] = ("rocprofv3 --kernel-trace --stats of a --profile-run; bytes_moved: the arrays a kernel reads and writes, once each; "
                                           "HBM peak taken as %.0f GB/s" % HBM_PEAK_GB_S)
    if not args.profile_run:
        exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
        base = [exe, os.path.join(tmp, "bench.boss"), os.path.join(tmp, "bench.fq"), "--format-on-device"]
        outs, legs = {}, {}
        for leg, extra in (("read_records", []), ("parse_on_device", ["--parse-on-device"])):
            wall = []
            for run in range(args.repeats + 1):
                t = time.perf_counter()
                res = subprocess.run(base + extra, capture_output=True, check=True)
                if run:
                    wall.append(time.perf_counter() - t)
                outs[leg] = res.stdout
            legs[leg] = {"wall_s": spread(wall)}
        assert outs["read_records"] == outs["parse_on_device"] and outs["read_records"], "the two outputs differ"
        legs["outputs_equal"] = True
        legs["output_bytes"] = len(outs["read_records"])
        legs["speedup_wall_median"] = legs["read_records"]["wall_s"]["median"] / legs["parse_on_device"]["wall_s"]["median"]
        legs["ranges_do_not_overlap"] = bool(legs["parse_on_device"]["wall_s"]["max"] < legs["read_records"]["wall_s"]["min"])
        legs["note"] = "whole process: loading the graph dump, the index build, reading and parsing the file, aligning, printing to a pipe"
        record["mgx_align_whole_process"] = legs
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
