#!/usr/bin/env python3
"""Loading a column annotation with k-mer coordinates (`X.column.annodbg` + `X.column.annodbg.coords`): the host path,
mgx_column_coord_file_read + mgx_annotation_create_from_file (every column and tuple section decoded on one host thread, the
row-major coordinates built by a host sort of one record per matrix entry), against mgx_annotation_load_coord_columns_device
(DESIGN 3.18), on the shape of bench.py --labels 1000: --labels labels over --rows rows, label j on rows / labels + 30 random rows
(tools/annotation_load_bench.py's shape), one coordinate per entry.

tests/coord_writer.py states the layout with Python integers; the files are written by the numpy functions of
tools/annotation_load_bench.py / tools/graph_load_bench.py — the same layout, checked byte for byte against the Python writer at a
small size before anything is measured.  First the two paths' annotations answer mgx_annotation_get_row_tuples on a sample of
rows alike; then, in one process, one warm-up and --repeats timed calls of either path, alternating.  No ratio is a condition
here: the figures are recorded as measured, with whether the device path's range lies wholly below the host path's.

  python tools/coord_load_bench.py --out profiles/coord_load_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import annotation_load_bench as alb  # noqa: E402
import coord_writer as cw  # noqa: E402
import graph_load_bench as glb  # noqa: E402
import sdsl_writer as sw  # noqa: E402


def tuple_column(n_set, values, width):
    """one coordinate per set row: delimiters 1 (0 1)^n as bit_vector_sd stores them (the complement: the sparser side), values"""
    bits = 2 * n_set + 1
    zeros = np.arange(1, bits, 2, dtype=np.int64)
    delims = sw.be(sw.CODE_SD) + (alb.sd_vector(bits, zeros) + b"\1" if n_set else alb.sd_vector(bits, np.zeros(1, np.int64)) + b"\0")
    return delims + glb.int_vector(np.asarray(values, dtype=np.int64), width)


def write_pair(path, n_rows, labels, columns, coords, width):
    alb.write_file(path, n_rows, labels, columns, sw.CODE_SD)
    with open(path + ".coords", "wb") as f:
        for rows, co in zip(columns, coords):
            f.write(tuple_column(len(rows), co, width))


def check_writer(tmp):
    rng = np.random.default_rng(5)
    for n in (1, 64, 700):
        cols = [np.flatnonzero(rng.random(n) < d) for d in (0.0, 0.1, 0.4)]
        coords = [rng.integers(0, 1 << 20, size=len(c)) for c in cols]
        labels = ["c%d" % j for j in range(len(cols))]
        path = os.path.join(tmp, "check.column.annodbg")
        write_pair(path, n, labels, cols, coords, 20)
        want = cw.coord_pair(n, labels, [c.tolist() for c in cols], [[[int(v)] for v in co] for co in coords],
                             kinds=["sd_inv" if len(c) else "sd" for c in cols], widths=[20] * len(cols), v2=True)
        assert open(path, "rb").read() == want[0] and open(path + ".coords", "rb").read() == want[1], n


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=104_000_000, help="the bench graph's edges")
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100_000, help="rows whose tuples are compared")
    ap.add_argument("--profile-only", action="store_true", help="write the files, call the device loader once and leave (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="coord_load_bench")
    check_writer(tmp)
    print("writer equals tests/coord_writer.py at the small sizes", file=sys.stderr)

    import torch
    from metagraph_amd import aligner, capi
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    rng = np.random.default_rng(20240601)
    n_rows, per = args.rows, args.rows // args.labels + 30
    labels = ["label%d" % j for j in range(args.labels)]
    path = os.path.join(tmp, "bench.column.annodbg")
    t0 = time.perf_counter()
    columns = [np.unique(rng.integers(0, n_rows, size=per)) for _ in labels]
    coords = [rng.integers(0, 1 << 27, size=len(c)) for c in columns]
    write_pair(path, n_rows, labels, columns, coords, 27)
    n_entries = sum(len(c) for c in columns)
    del columns, coords
    t_write = time.perf_counter() - t0
    print("%d rows, %d entries, %d + %d bytes, written in %.1f s" % (n_rows, n_entries, os.path.getsize(path), os.path.getsize(path + ".coords"), t_write),
          file=sys.stderr)
    arr = (C.c_char_p * 1)(path.encode())

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def host(keep=False):
        cf, h = C.c_void_p(), C.c_void_p()
        t_ms, rc = ms(lambda: lib.mgx_column_coord_file_read(arr, 1, C.byref(cf)) or lib.mgx_annotation_create_from_file(cf, 0, C.byref(h)))
        assert rc == 0, lib.mgx_last_error()
        lib.mgx_column_file_free(cf)
        if keep:
            return h
        lib.mgx_annotation_destroy(h)
        return t_ms

    def device(keep=False):
        h = C.c_void_p()
        t_ms, rc = ms(lambda: lib.mgx_annotation_load_coord_columns_device(arr, 1, 0, C.byref(h), None))
        assert rc == 0, lib.mgx_last_error()
        if keep:
            return h
        lib.mgx_annotation_destroy(h)
        return t_ms

    if args.profile_only:
        device()
        return
    # the same answers first (this is also the warm-up of either path)
    sample = np.random.default_rng(1).integers(0, n_rows, size=args.sample).astype(np.uint64)
    answers = []
    for make in (host, device):
        an = aligner.Annotation.__new__(aligner.Annotation)
        an.h, an._cols = make(keep=True), []
        answers.append(an.get_row_tuples(sample))
        an.close()
        print("warm-up and sample of one path done", file=sys.stderr)
    equal = answers[0] == answers[1]
    n_tuples = sum(len(t) for t in answers[0])
    del answers
    t_host, t_dev = [], []
    for i in range(args.repeats):
        t_host.append(host())
        t_dev.append(device())
        print("repeat %d: host %.0f ms, device %.0f ms" % (i, t_host[-1], t_dev[-1]), file=sys.stderr)
    h, d = spread(t_host), spread(t_dev)
    record = {"workload": {"rows": n_rows, "labels": args.labels, "entries": n_entries, "coordinates_per_entry": 1, "value_width": 27,
                           "delimiters": "sd_vector, inverted", "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                           "file_bytes": os.path.getsize(path), "side_file_bytes": os.path.getsize(path + ".coords"), "write_s": t_write},
              "row_tuples_equal_on_sample": bool(equal), "sample_rows": args.sample, "sample_tuples": n_tuples,
              "mgx_column_coord_file_read + mgx_annotation_create_from_file_ms": h,
              "mgx_annotation_load_coord_columns_device_ms": d,
              "device_range_wholly_below_host_range": bool(d["max"] < h["min"])}
    print(json.dumps(record))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")
    sys.exit(0 if equal else 1)


if __name__ == "__main__":
    main()
