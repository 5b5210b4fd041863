"""Test infrastructure: writes column annotations with k-mer coordinates in the two forms csrc/boss_files.hpp reads
(read_tuples, parse_column_coord), on top of tests/sdsl_writer.py — an independent (Python) statement of
TupleCSCMatrix::serialize_tuples (tuple_csc_matrix.hpp:174-180: per column a bit_vector_smart of delimiters and an
sdsl::int_vector<> of values), ColumnMajor::serialize (column_major.cpp:110-123: serialize_number(n_columns), bare bit_vector_sd
columns) and StaticBinRelAnnotator::serialize (annotation_matrix.cpp:25-32: label encoder, matrix).
A column's tuples are given in the order of its set rows (ascending): tuples[r] = the coordinates of its r-th set row."""
import sdsl_writer as sw

KINDS = ("sd", "sd_inv", "stat", "rrr")       # how a delimiter vector is stored (sd_inv: the complement's positions + the flag)


def delimiters(tuples):
    """1, then per tuple one 0 per value and a closing 1 (annotate_column_compressed.cpp:320-337)"""
    bits = [1]
    for t in tuples:
        bits += [0] * len(t) + [1]
    return bits


def delimiter_vector(bits, kind):
    if kind == "sd":
        return sw.be(sw.CODE_SD) + sw.sd_vector(len(bits), [i for i, b in enumerate(bits) if b]) + b"\0"
    if kind == "sd_inv":
        return sw.be(sw.CODE_SD) + sw.sd_vector(len(bits), [i for i, b in enumerate(bits) if not b]) + b"\1"
    return sw.adaptive(bits, sw.CODE_STAT if kind == "stat" else sw.CODE_RRR)


def width_of(values):
    return max(1, max(values, default=0).bit_length())      # hi(max_coord) + 1


def tuple_column(bits, values, kind="sd", width=None):
    """one column of the tuple section from its raw parts (the damaged files are written through this)"""
    return delimiter_vector(bits, kind) + sw.int_vector(values, width_of(values) if width is None else width)


def tuple_section(col_tuples, kinds=None, widths=None):
    out = b""
    for j, tuples in enumerate(col_tuples):
        values = [v for t in tuples for v in t]
        out += tuple_column(delimiters(tuples), values, kinds[j] if kinds else "sd", widths[j] if widths else None)
    return out


def coord_pair(n_rows, labels, columns, col_tuples, kinds=None, widths=None, codes=None, v2=False):
    """form (a): (the bytes of X.column.annodbg, the bytes of X.column.annodbg.coords)"""
    return sw.column_file(n_rows, labels, columns, codes=codes, v2=v2), tuple_section(col_tuples, kinds, widths)


def column_major(n_rows, columns, sizes=None):
    out = sw.be(len(columns))
    for j, col in enumerate(columns):
        s = set(int(r) for r in col)
        out += sw.bit_vector_sd([1 if r in s else 0 for r in range(sizes[j] if sizes else n_rows)])      # no representation code
    return out


def column_coord_file(n_rows, labels, columns, col_tuples, kinds=None, widths=None, v2=False, sizes=None):
    """form (b): the bytes of X.column_coord.annodbg"""
    return ((sw.label_encoder_v2 if v2 else sw.label_encoder_v1)(labels) + column_major(n_rows, columns, sizes)
            + tuple_section(col_tuples, kinds, widths))


def write_case(d, case):
    """the case's files into directory d (a pathlib.Path) -> the paths to load"""
    paths = []
    for i, f in enumerate(case["files"]):
        if case["form"] == "b":
            p = d / ("%s_%d.column_coord.annodbg" % (case["name"], i))
            p.write_bytes(f)
        else:
            p = d / ("%s_%d.column.annodbg" % (case["name"], i))
            p.write_bytes(f[0])
            if f[1] is not None:
                (d / ("%s_%d.column.annodbg.coords" % (case["name"], i))).write_bytes(f[1])
        paths.append(p)
    return paths
