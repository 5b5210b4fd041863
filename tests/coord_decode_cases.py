"""Test infrastructure: the coordinate annotations at which the host reader (csrc/boss_files.hpp: read_tuples) or a piece of the
on-device decode (csrc/coord_decode.hpp) can go wrong, written with tests/coord_writer.py — the smallest shapes per piece.
Shared by tests/test_coord_files.py (host reader), tests/test_coord_decode_model.py (kernel bodies on the host) and
tests/test_gpu_coord_decode.py (the kernels).
A case: {"name", "form": "a" | "b", "files": [(column file, side file)] | [bytes], "n_rows", "labels", "columns": [sorted rows per
label], "tuples": [per label, per set row, its coordinates]}; built once per process (the writers are pure Python)."""
import functools
import random

import coord_writer as cw
import sdsl_writer as sw

N_ROWS = (1, 63, 64, 65, 4097)       # the rrr block (63) against the 64-bit word; several words and more than one 256-lane block
WIDTHS = (1, 7, 33, 63)
LENGTHS = (0, 1, 2, 65)              # empty tuple, one coordinate, two, more than a word of delimiters


def _patterns(rng, n):
    pick = lambda m: sorted(rng.sample(range(n), m))
    return [("empty", []), ("full", list(range(n))), ("row0", [0]), ("last", [n - 1]), ("d20", pick(max(1, n // 5)))]


def _tuples(rng, n_set, width, first):
    """ascending tuples of the lengths 0, 1, 2, 65 in turn for the first eight set rows (from `first` on), one coordinate after"""
    out = []
    for r in range(n_set):
        ln = LENGTHS[(first + r) % 4] if r < 8 else 1
        out.append(sorted(rng.randrange(0, 1 << width) for _ in range(ln)))
    return out


def _columns(rng, n, tag):
    """one column per (delimiter kind, value width): 16 columns whose row patterns and first tuple lengths go round"""
    labels, cols, tuples, kinds, widths = [], [], [], [], []
    pats = _patterns(rng, n)
    x = 0
    for kind in cw.KINDS:
        for width in WIDTHS:
            pname, rows = pats[x % len(pats)]
            labels.append("%s%s_w%d_%s" % (tag, kind, width, pname))
            cols.append(rows)
            tuples.append(_tuples(rng, len(rows), width, x))
            kinds.append(kind)
            widths.append(width)
            x += 1
    return labels, cols, tuples, kinds, widths


def _case(name, form, files, n_rows, labels, cols, tuples):
    return {"name": name, "form": form, "files": files, "n_rows": n_rows, "labels": list(labels), "columns": [sorted(c) for c in cols],
            "tuples": tuples}


@functools.lru_cache(maxsize=None)
def well_formed():
    rng = random.Random(4321)
    out = []
    codes3 = (sw.CODE_SD, sw.CODE_STAT, sw.CODE_RRR)
    for n in N_ROWS:
        labels, cols, tuples, kinds, widths = _columns(rng, n, "")
        v2 = n % 2 == 0
        codes = [codes3[j % 3] for j in range(len(cols))]
        out.append(_case("a_rows%d" % n, "a", [cw.coord_pair(n, labels, cols, tuples, kinds, widths, codes=codes, v2=v2)], n, labels, cols, tuples))
        out.append(_case("b_rows%d" % n, "b", [cw.column_coord_file(n, labels, cols, tuples, kinds, widths, v2=not v2)], n, labels, cols, tuples))
    # one column only; no labels at all (form (b): zero columns, zero rows)
    for kind in cw.KINDS:
        rows = [3, 64, 100]
        tp = [[5], [], [1, 2, 2 ** 40]]
        out.append(_case("one_%s" % kind, "a", [cw.coord_pair(129, ["only"], [rows], [tp], [kind])], 129, ["only"], [rows], [tp]))
    out.append(_case("a_no_labels", "a", [cw.coord_pair(77, [], [], [])], 77, [], [], []))
    out.append(_case("b_no_labels", "b", [cw.column_coord_file(0, [], [], [])], 0, [], [], []))
    # two pairs of form (a) merged: the columns side by side
    parts = []
    for i in range(2):
        labels, cols, tuples, kinds, widths = _columns(rng, 200, "f%d_" % i)
        parts.append((cw.coord_pair(200, labels, cols, tuples, kinds, widths, v2=i == 1), labels, cols, tuples))
    out.append(_case("a_merge2", "a", [p[0] for p in parts], 200, sum((p[1] for p in parts), []), sum((p[2] for p in parts), []),
                     sum((p[3] for p in parts), [])))
    return tuple(out)


def count_mix(n_cols):
    """form (a) over 129 rows, n_cols columns whose delimiter kinds go round: the files whose launch and allocation counts are
    compared"""
    rng = random.Random(n_cols)
    n = 129
    labels = ["m%d" % j for j in range(n_cols)]
    cols = [sorted(rng.sample(range(n), 1 + j % 7)) for j in range(n_cols)]
    tuples = [[sorted(rng.randrange(0, 1000) for _ in range(1 + (r + j) % 3)) for r in range(len(cols[j]))] for j in range(n_cols)]
    # (which kernels run depends on the kinds present: sd, stat and rrr delimiters are among the first three columns, the
    # inverted sd vectors of the larger file run in the launches of the plain ones)
    kinds = [("sd", "stat", "rrr", "sd_inv")[j % 4] for j in range(n_cols)]
    codes = [(sw.CODE_SD, sw.CODE_STAT, sw.CODE_RRR)[j % 3] for j in range(n_cols)]
    return _case("mix%d" % n_cols, "a", [cw.coord_pair(n, labels, cols, tuples, kinds, codes=codes)], n, labels, cols, tuples)


def damaged():
    """[(name, form, files, error code name, words in the message)]: one fault each.  Side file None: not written."""
    n, labels, cols = 100, ["a", "b"], [[1, 5, 70], [2, 99]]
    ta, tb = [[10, 20], [7], [1, 2, 3]], [[4], [8, 9]]
    colfile = sw.column_file(n, labels, cols)
    good_b = cw.tuple_column(cw.delimiters(tb), [4, 8, 9])
    da, va = cw.delimiters(ta), [10, 20, 7, 1, 2, 3]           # 1 0 0 1 0 1 0 0 0 1

    def side(bits, values, kind="stat", width=None):
        return cw.tuple_column(bits, values, kind, width) + good_b

    out = []
    add = lambda name, sidefile, code, words, form="a", files=None: out.append((name, form, files if files else [(colfile, sidefile)], code, words))
    add("delimiter_length", side(da[:-1] + [0, 1], va), "MGX_ERR_INVALID", "delimiters: 11 bits")
    add("first_bit_clear", side([0, 1] + da[2:], va), "MGX_ERR_INVALID", "delimiters: first bit clear")
    add("last_bit_clear", side(da[:-2] + [1, 0], va), "MGX_ERR_INVALID", "delimiters: last bit clear")
    add("one_delimiter_too_many", side(da[:1] + [1] + da[2:], va), "MGX_ERR_INVALID", "delimiters: 5 set bits")
    add("descending_tuple", side(da, [20, 10, 7, 1, 2, 3]), "MGX_ERR_INVALID", "coordinates: a tuple is not ascending")
    add("value_top_bit", side(da, [10, 20, 7, 1, 2, 1 << 63], width=64), "MGX_ERR_INVALID", "values: a coordinate of 2^63 or more")
    add("values_truncated", cw.tuple_column(da, va, "stat") + good_b[:-8], "MGX_ERR_INVALID", "values")
    add("bytes_left_over", side(da, va) + b"\0", "MGX_ERR_INVALID", "bytes left after the last column")
    add("side_file_missing", None, "MGX_ERR_INVALID", ".column.annodbg.coords")
    other = cw.coord_pair(n, ["c", "a"], [[5], [6]], [[[1]], [[2]]])
    add("label_in_two_files", None, "MGX_ERR_UNSUPPORTED", "occurs in two files", files=[(colfile, side(da, va)), other])
    add("column_sizes_differ", None, "MGX_ERR_INVALID", "column", form="b",
        files=[cw.column_coord_file(n, labels, cols, [ta, tb], sizes=[n, n + 1])])
    # the same faults in the other representations of the delimiters, and in form (b): the kernels' own checks
    for kind in ("sd", "sd_inv", "rrr"):
        add("first_bit_clear_" + kind, side([0, 1] + da[2:], va, kind), "MGX_ERR_INVALID", "delimiters: first bit clear")
        add("last_bit_clear_" + kind, side(da[:-2] + [1, 0], va, kind), "MGX_ERR_INVALID", "delimiters: last bit clear")
        add("one_delimiter_too_many_" + kind, side(da[:1] + [1] + da[2:], va, kind), "MGX_ERR_INVALID", "delimiters: 5 set bits")
    head_b = sw.label_encoder_v1(labels) + cw.column_major(n, cols)
    add("b_descending_tuple", None, "MGX_ERR_INVALID", "coordinates: a tuple is not ascending", form="b",
        files=[head_b + cw.tuple_column(da, va) + cw.tuple_column(cw.delimiters(tb), [4, 9, 8])])
    add("b_bytes_left_over", None, "MGX_ERR_INVALID", "bytes left after the last column", form="b",
        files=[cw.column_coord_file(n, labels, cols, [ta, tb]) + b"\0\0"])
    return out
