"""Test infrastructure: the `.column.annodbg` files at which a piece of the on-device column decode (csrc/col_decode.hpp) can go
wrong, written with tests/sdsl_writer.py — the smallest shapes per piece.  Shared by tests/test_col_decode_model.py (the kernel
bodies on the host, under sanitizers; it also checks that the host reader returns the rows every case was written from) and
tests/test_gpu_col_decode.py (the kernels).  A case: {"name", "files": [bytes per file], "n_rows", "labels", "columns": [sorted rows
per label]}; built once per process (the writer is pure Python)."""
import functools

import numpy as np

import sdsl_writer as sw

CODES = (("sd", sw.CODE_SD), ("stat", sw.CODE_STAT), ("rrr", sw.CODE_RRR))
# the rrr block size (63) against the 64-bit word; a few thousand rows (high and the plain bits span several words); a column
# whose words cross a 256-lane workgroup (256 lanes x 64 rows = 16384 rows)
N_ROWS = (1, 62, 63, 64, 65, 126, 127, 128, 129, 3001, 16500)


def patterns(rng, n):
    """name -> rows: empty, full, only row 0, only the last row, alternating, random at several densities, and just below / just
    above one half (bit_vector_sd stores the complement — `inverted` — when more than n // 2 rows are set)"""
    pick = lambda m: sorted(int(r) for r in rng.choice(n, size=m, replace=False))
    return [("empty", []), ("full", list(range(n))), ("row0", [0]), ("last", [n - 1]), ("alt", list(range(0, n, 2))),
            ("alt1", list(range(1, n, 2))), ("d01", pick(max(1, n // 100))), ("d20", pick(n // 5)), ("half", pick(n // 2)),
            ("half1", pick(min(n, n // 2 + 1))), ("d90", pick(n - n // 10))]


def _case(name, n_rows, labels, columns, codes, v2=False):
    return {"name": name, "files": [sw.column_file(n_rows, labels, columns, codes=codes, v2=v2)], "n_rows": n_rows, "labels": list(labels),
            "columns": [sorted(c) for c in columns]}


def _mixed(rng, name, n_rows, n_cols, v2, label=lambda j: "L%d" % j):
    pats = patterns(rng, n_rows)
    cols, codes = [], []
    for j in range(n_cols):
        cols.append(pats[int(rng.integers(0, len(pats)))][1])
        codes.append(CODES[j % 3][1])
    return _case(name, n_rows, [label(j) for j in range(n_cols)], cols, codes, v2=v2)


@functools.lru_cache(maxsize=None)
def well_formed():
    rng = np.random.default_rng(1234)
    out = []
    for n in N_ROWS:                                           # every code x every pattern per n_rows, one file
        labels, cols, codes = [], [], []
        for pname, rows in patterns(rng, n):
            for cname, code in CODES:
                labels.append("%s_%s" % (cname, pname))
                cols.append(rows)
                codes.append(code)
        out.append(_case("rows%d" % n, n, labels, cols, codes, v2=(n % 2 == 0)))
    for code_name, code in CODES:                              # one column only, of each code
        out.append(_case("one_%s" % code_name, 129, ["only"], [patterns(rng, 129)[7][1]], [code]))
    out.append(_mixed(rng, "cols3_v1", 200, 3, False))
    out.append(_mixed(rng, "cols3_v2", 200, 3, True))
    out.append(_mixed(rng, "cols300_v1", 129, 300, False))
    out.append(_mixed(rng, "cols300_v2", 129, 300, True))
    long_label = lambda j: "label-%d-" % j + "x" * (128 + 70 * j)      # >= 128 bytes: the v1 encoder's multi-byte length prefix
    out.append(_mixed(rng, "long_labels_v1", 65, 4, False, label=long_label))
    out.append(_mixed(rng, "long_labels_v2", 65, 4, True, label=long_label))
    out.append(_case("no_labels", 77, [], [], []))
    for n_files in (2, 3):                                     # merge_load: the files' columns side by side
        parts = [_mixed(rng, "p", 700, 2 + i, i % 2 == 1, label=lambda j, i=i: "f%d_%d" % (i, j)) for i in range(n_files)]
        out.append({"name": "merge%d" % n_files, "files": [p["files"][0] for p in parts], "n_rows": 700,
                    "labels": sum((p["labels"] for p in parts), []), "columns": sum((p["columns"] for p in parts), [])})
    return tuple(out)


def count_mix(n_cols, inverted):
    """a file of n_cols columns over 129 rows whose kinds go round (sd — plain or inverted —, stat, rrr): the 3- and the 300-column
    files whose launch and allocation counts are compared"""
    n = 129
    kinds = [(sw.CODE_SD, list(range(0, n - 5)) if inverted else list(range(0, n, 7))), (sw.CODE_STAT, list(range(3, n, 2))), (sw.CODE_RRR, list(range(1, n, 3)))]
    cols = [kinds[j % 3] for j in range(n_cols)]
    return _case("mix%d" % n_cols, n, ["m%d" % j for j in range(n_cols)], [c[1] for c in cols], [c[0] for c in cols])


def bad_merges():
    """[(name, [file bytes], error code name, words in the message)]: files that do not go together"""
    a = sw.column_file(100, ["a", "b"], [[1, 2], [3]])
    rows = sw.column_file(101, ["c"], [[5]])
    dup = sw.column_file(100, ["c", "a"], [[5], [6]])
    return [("row_count_mismatch", [a, rows], "MGX_ERR_INVALID", "annotates 101 rows"), ("duplicate_label", [a, dup], "MGX_ERR_UNSUPPORTED", "occurs in two files")]


def header_refusals():
    """[(name, file bytes, error code name, words in the message)]: what the header walk refuses before any kernel runs"""
    good = sw.column_file(100, ["a", "b"], [[1, 2], [3, 50]], codes=[sw.CODE_SD, sw.CODE_STAT])
    head = len(sw.be(100) + sw.label_encoder_v1(["a", "b"]))
    unknown = bytearray(good)
    unknown[head + 7] = 9
    il = bytearray(good)
    il[head + 7] = 3
    return [("unknown_code", bytes(unknown), "MGX_ERR_INVALID", "unknown bit vector representation 9"),
            ("bit_vector_il", bytes(il), "MGX_ERR_UNSUPPORTED", "bit_vector_il<4096>"),
            ("cut_in_labels", good[:12], "MGX_ERR_INVALID", "file ends inside"),
            ("cut_in_column_header", good[:head + 12], "MGX_ERR_INVALID", "file ends inside column")]
