#!/usr/bin/env python3
"""Loading `.column.annodbg` files: mgx_column_file_read + mgx_annotation_create_from_file (every column decoded on one host
thread, the set rows uploaded at 8 bytes each) against mgx_annotation_load_columns_device (the payloads decoded by kernels,
DESIGN 3.17), on an annotation of the shape of bench.py --labels 1000 (config 3): --labels labels over --rows rows, label j on
rows / labels + 30 rows (a genome segment's k-mers and 15 positions into either neighbour).  The rows of a label are drawn at
random: a segment's nodes are scattered over the BOSS order, and the loaders see nothing else of the graph.  The file is written
once with sd columns and once with rrr columns; the rrr file at --rrr-rows rows (its writer and its 1000 bit maps of `rows` bits
take too long at the full row count: the figures of that file are measured at the stated size, nothing is extrapolated).

tests/sdsl_writer.py states the layout with Python integers; the files are written by numpy functions (those of
tools/graph_load_bench.py and the sd_vector below) — the same layout, checked byte for byte against sdsl_writer.column_file at a
small size before anything is measured.  In one process, after a warm-up of each, --repeats timed calls of either path,
alternating; the split of a call comes from the pieces on their own: reading the file, the host reader (mgx_column_file_read:
read + decode) and mgx_annotation_create_sparse over rows already in device memory (the sort both paths end in).
Exit status 1 if the new call's range reaches the old call's on a file.

  python tools/annotation_load_bench.py --out profiles/annotation_load_bench.json
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
import graph_load_bench as glb  # noqa: E402
import sdsl_writer as sw  # noqa: E402

le, be = sw.le, sw.be


def sd_vector(size, ones):
    """sdsl_writer.sd_vector over a numpy array of ascending positions"""
    ones = np.asarray(ones, dtype=np.int64)
    m = len(ones)
    logm = max(m, 1).bit_length() if m else 1
    logn = max(size, 1).bit_length()
    if logm == logn:
        logm -= 1
    wl = max(1, logn - logm)
    high = np.zeros(m + (1 << logm), np.uint8)
    high[(ones >> wl) + np.arange(m)] = 1
    return (le(size) + bytes([wl]) + glb.int_vector(ones & ((1 << wl) - 1), wl) + glb.bit_vector(high)
            + glb.select_support_mcl(np.flatnonzero(high), len(high)) + glb.select_support_mcl(np.flatnonzero(high == 0), len(high)))


def column(n_rows, rows, code):
    rows = np.asarray(rows, dtype=np.int64)
    if code == sw.CODE_SD:
        inverted = len(rows) > n_rows // 2
        if inverted:
            bits = np.ones(n_rows, np.uint8)
            bits[rows] = 0
            rows = np.flatnonzero(bits)
        return be(code) + sd_vector(n_rows, rows) + bytes([1 if inverted else 0])
    bits = np.zeros(n_rows, np.uint8)
    bits[rows] = 1
    return be(code) + (glb.rrr_vector63(bits) if code == sw.CODE_RRR else glb.bit_vector_stat(bits))


def write_file(path, n_rows, labels, columns, code):
    with open(path, "wb") as f:
        f.write(be(n_rows) + sw.label_encoder_v2(labels))
        for rows in columns:
            f.write(column(n_rows, rows, code))


def check_writer(tmp):
    """the numpy writer against tests/sdsl_writer.py, byte for byte, at sizes small enough for the latter"""
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 129, 5000):
        cols = [np.flatnonzero(rng.random(n) < d) for d in (0.0, 0.02, 0.3, 0.7, 1.0)]
        labels = ["c%d" % j for j in range(len(cols))]
        for code in (sw.CODE_SD, sw.CODE_STAT, sw.CODE_RRR):
            path = os.path.join(tmp, "check.column.annodbg")
            write_file(path, n, labels, cols, code)
            assert open(path, "rb").read() == sw.column_file(n, labels, [c.tolist() for c in cols], codes=[code] * len(cols), v2=True), (n, code)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=104_000_000, help="rows of the sd file: the bench graph's edges")
    ap.add_argument("--rrr-rows", type=int, default=8_000_000, help="rows of the rrr file")
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true", help="write the files, call the new loader once per file and leave (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="annotation_load_bench")
    t = time.perf_counter()
    check_writer(tmp)
    print("writer equals tests/sdsl_writer.py at the small sizes (%.1f s)" % (time.perf_counter() - t), file=sys.stderr)

    import torch
    from metagraph_amd import capi
    lib = capi.lib()
    assert lib.mgx_device_count() > 0, "no HIP device"
    record = {"workload": {"labels": args.labels, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                           "note": "label j on rows / labels + 30 random rows (the shape of bench.py --labels: a genome segment's nodes); every "
                                   "figure is measured at the rows stated with its file"}}

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    worse = False
    for name, code, n_rows in (("sd", sw.CODE_SD, args.rows), ("rrr", sw.CODE_RRR, args.rrr_rows)):
        rng = np.random.default_rng(20240601)
        per = n_rows // args.labels + 30
        labels = ["label%d" % j for j in range(args.labels)]
        path = os.path.join(tmp, name + ".column.annodbg")
        t_write, _ = ms(lambda: write_file(path, n_rows, labels, (np.unique(rng.integers(0, n_rows, size=per)) for _ in labels), code))
        print("%s: %d rows, %d bytes, written in %.1f s" % (name, n_rows, os.path.getsize(path), t_write / 1e3), file=sys.stderr)
        arr = (C.c_char_p * 1)(path.encode())

        def old():
            cf, h = C.c_void_p(), C.c_void_p()
            t_ms, rc = ms(lambda: lib.mgx_column_file_read(arr, 1, C.byref(cf)) or lib.mgx_annotation_create_from_file(cf, 0, C.byref(h)))
            assert rc == 0, lib.mgx_last_error()
            lib.mgx_column_file_free(cf)
            lib.mgx_annotation_destroy(h)
            return t_ms

        def new():
            h = C.c_void_p()
            t_ms, rc = ms(lambda: lib.mgx_annotation_load_columns_device(arr, 1, 0, C.byref(h), None))
            assert rc == 0, lib.mgx_last_error()
            lib.mgx_annotation_destroy(h)
            return t_ms

        if args.profile_only:
            new()
            continue
        # the host reader's tables: the reference of the comparison, and the input of the create-only piece
        cf = C.c_void_p()
        assert lib.mgx_column_file_read(arr, 1, C.byref(cf)) == 0, lib.mgx_last_error()
        cb = np.ctypeslib.as_array(lib.mgx_column_file_col_begin(cf), shape=(args.labels + 1,)).copy()
        rows = np.ctypeslib.as_array(lib.mgx_column_file_rows(cf), shape=(int(cb[-1]),)).copy()
        lib.mgx_column_file_free(cf)
        hk = C.c_void_p()
        assert lib.mgx_column_file_decode_device(arr, 1, 0, C.byref(hk)) == 0, lib.mgx_last_error()
        equal = (np.array_equal(cb, np.ctypeslib.as_array(lib.mgx_column_file_col_begin(hk), shape=(args.labels + 1,)))
                 and np.array_equal(rows, np.ctypeslib.as_array(lib.mgx_column_file_rows(hk), shape=(int(cb[-1]),))))
        lib.mgx_column_file_free(hk)
        rows_d = torch.from_numpy(rows.astype(np.int64)).cuda()
        torch.cuda.synchronize()

        def reader():
            cf = C.c_void_p()
            t_ms, rc = ms(lambda: lib.mgx_column_file_read(arr, 1, C.byref(cf)))
            assert rc == 0
            lib.mgx_column_file_free(cf)
            return t_ms

        def create():
            h = C.c_void_p()
            t_ms, rc = ms(lambda: lib.mgx_annotation_create_sparse(n_rows, args.labels, cb.ctypes.data, rows_d.data_ptr(), 1, 0, C.byref(h)))
            assert rc == 0, lib.mgx_last_error()
            lib.mgx_annotation_destroy(h)
            return t_ms

        old(), new(), create()                                                     # warm-up
        t_old, t_new, t_read, t_reader, t_create = [], [], [], [], []
        for _ in range(args.repeats):
            t_old.append(old())
            t_new.append(new())
            t_read.append(ms(lambda: open(path, "rb").read())[0])
            t_reader.append(reader())
            t_create.append(create())
        o, nw, rd, hr, cr = spread(t_old), spread(t_new), spread(t_read), spread(t_reader), spread(t_create)
        record[name] = {
            "rows": n_rows, "set_rows": int(cb[-1]), "file_bytes": os.path.getsize(path), "write_s": t_write / 1e3, "tables_equal": bool(equal),
            "mgx_column_file_read + mgx_annotation_create_from_file_ms": o, "mgx_annotation_load_columns_device_ms": nw,
            "speedup_median": o["median"] / nw["median"],
            "pieces_ms": {"file_read": rd, "mgx_column_file_read (read + host decode)": hr, "mgx_annotation_create_sparse over device rows": cr},
            "split_of_the_medians_ms": {
                "host path": {"file_read": rd["median"], "decode": hr["median"] - rd["median"],
                              "upload_of_rows": o["median"] - hr["median"] - cr["median"], "mgx_annotation_create_sparse": cr["median"]},
                "device path": {"file_read": rd["median"], "plan_upload_and_decode": nw["median"] - rd["median"] - cr["median"],
                                "mgx_annotation_create_sparse": cr["median"]}},
        }
        del rows_d
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
