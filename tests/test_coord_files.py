"""mgx_column_coord_file_read, the host reader of column annotations with k-mer coordinates (csrc/boss_files.hpp: read_tuples,
parse_column_coord), against the input of the independent writer tests/coord_writer.py, entry for entry, on
the cases of tests/coord_decode_cases.py; the damaged files, one fault each, with the field every message names.  CPU only."""
import ctypes as C

import pytest

import coord_decode_cases as cases
import coord_writer as cw
from metagraph_amd import aligner as A
from metagraph_amd import capi


def expected(case):
    """(n_rows, labels, col_begin, rows, coord_begin, coords) as the reader must return them"""
    cb, rows, cob, co = [0], [], [0], []
    for col, tuples in zip(case["columns"], case["tuples"]):
        assert len(col) == len(tuples)
        rows += col
        cb.append(len(rows))
        for t in tuples:
            co += t
            cob.append(len(co))
    return case["n_rows"], case["labels"], cb, rows, cob, co


def as_lists(got):
    n_rows, names, cb, rows, cob, co = got
    return n_rows, names, cb.tolist(), rows.tolist(), cob.tolist(), co.tolist()


@pytest.mark.parametrize("case", cases.well_formed(), ids=lambda c: c["name"])
def test_host_reader_returns_what_was_written(case, tmp_path):
    paths = cw.write_case(tmp_path, case)
    assert as_lists(A.read_column_files(paths, coordinates=True)) == expected(case)
    if case["form"] == "a":            # mgx_column_file_read on the same files: what it returned before, the side files ignored
        n_rows, names, cb, rows = A.read_column_files(paths)
        assert (n_rows, names, cb.tolist(), rows.tolist()) == expected(case)[:4]


def test_the_cases_cover_what_they_claim():
    lengths, kinds = set(), set()
    for case in cases.well_formed():
        for label, tuples in zip(case["labels"], case["tuples"]):
            lengths |= {len(t) for t in tuples}
            kinds |= {k for k in cw.KINDS if label.replace("f0_", "").replace("f1_", "").startswith(k + "_w")}
    assert {0, 1, 2, 65} <= lengths and kinds == set(cw.KINDS)
    assert any(max((v for t in tp for v in t), default=0) >= 2 ** 62 for c in cases.well_formed() for tp in c["tuples"])


def test_accessors_are_null_without_coordinates(tmp_path):
    L = capi.lib()
    case = cases.well_formed()[0]
    paths = cw.write_case(tmp_path, case)
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    h = C.c_void_p()
    assert L.mgx_column_file_read(arr, len(paths), C.byref(h)) == 0
    assert not L.mgx_column_file_coord_begin(h) and not L.mgx_column_file_coords(h)
    L.mgx_column_file_free(h)
    assert not L.mgx_column_file_coord_begin(None) and not L.mgx_column_file_coords(None)
    assert L.mgx_column_coord_file_read(arr, len(paths), C.byref(h)) == 0
    assert L.mgx_column_file_coord_begin(h) and L.mgx_column_file_coords(h)
    L.mgx_column_file_free(h)


def test_a_column_coord_file_is_loaded_alone(tmp_path):
    case = next(c for c in cases.well_formed() if c["name"] == "b_rows63")
    p = cw.write_case(tmp_path, case)
    with pytest.raises(A.MgxError) as e:
        A.read_column_files(p + p, coordinates=True)
    assert e.value.code == capi.MGX_ERR_INVALID and "loaded alone" in str(e.value)


@pytest.mark.parametrize("name,form,files,code,words", cases.damaged(), ids=lambda x: x if isinstance(x, str) and "_" in x and " " not in x else None)
def test_damaged_files(name, form, files, code, words, tmp_path):
    paths = cw.write_case(tmp_path, {"name": name, "form": form, "files": files})
    with pytest.raises(A.MgxError) as e:
        A.read_column_files(paths, coordinates=True)
    assert e.value.code == getattr(capi, code), str(e.value)
    assert words in str(e.value), str(e.value)
