"""Column annotations with k-mer coordinates decoded by kernels (mgx_annotation_load_coord_columns_device, the hook
mgx_column_coord_file_decode_device; csrc/mgx_colload.hip over coord_decode.hpp) and transposed by kernels
(mgx_annotation_set_coordinates_device, csrc/mgx_annot.hip) against the host path (mgx_column_coord_file_read +
mgx_annotation_create_from_file, mgx_annotation_set_coordinates): the same tables entry for entry, the same annotation, the same
refusals word for word.  Needs a real MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import coord_decode_cases as cases
import coord_writer as cw
import orc
from metagraph_amd import aligner, capi

pytestmark = pytest.mark.gpu

counts = aligner.column_decode_kernel_launch_counts


def c_paths(paths):
    return (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])


@pytest.mark.parametrize("case", cases.well_formed(), ids=lambda c: c["name"])
def test_hook_gives_the_host_readers_tables(case, tmp_path):
    paths = cw.write_case(tmp_path, case)
    h = aligner.read_column_files(paths, coordinates=True)
    d = aligner.read_column_files(paths, coordinates=True, on_device=True)
    assert h[0] == d[0] == case["n_rows"] and h[1] == d[1] == case["labels"]
    for x, key in ((2, "col_begin"), (3, "rows"), (4, "coord_begin"), (5, "coords")):
        assert np.array_equal(h[x], d[x]), (case["name"], key, np.flatnonzero(h[x] != d[x])[:8] if len(h[x]) == len(d[x]) else (len(h[x]), len(d[x])))
    assert len(h[5]) == sum(len(t) for tp in case["tuples"] for t in tp)


def oracle_world():
    """the world of test_gpu_coordinates.py::test_row_tuples_...: per row its [(label, [coordinates])] from the oracle's Annotation"""
    rng = random.Random(5)
    k = 7
    genome = "".join(rng.choice("ACGT") for _ in range(600))
    seqs = [genome[:400], genome[200:], genome[100:300] + genome[100:300]]
    g = orc.Graph.build(k, seqs, 0, True)
    anno = orc.Annotation(g, 2)
    for s, l, st in zip(seqs, [0, 1, 0], [0, 1000, 5000]):
        anno.annotate_coords(s, l, st)
    ol = orc.L()
    ol.orc_annotation_row_tuples.restype = C.c_uint64
    ol.orc_annotation_row_tuples.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_uint64]
    per_row = []
    for r in range(g.n_edges):
        labels, cb, co = (C.c_uint64 * 8)(), (C.c_uint64 * 9)(), (C.c_int64 * 64)()
        nl = ol.orc_annotation_row_tuples(anno.h, r, labels, cb, co, 64)
        per_row.append([(int(labels[t]), [int(co[x]) for x in range(cb[t], cb[t + 1])]) for t in range(nl)])
    return k, g, per_row


@pytest.mark.parametrize("form", ["a", "b"])
def test_get_row_tuples_of_three_annotations(form, tmp_path):
    k, g, per_row = oracle_world()
    n_rows = g.n_edges
    cols, tuples = [[], []], [[], []]
    for r, tp in enumerate(per_row):
        for lab, coords in tp:
            cols[lab].append(r)
            tuples[lab].append(coords)
    assert any(len(cs) > 1 for tp in tuples for cs in tp)
    names = ["first", "second"]
    if form == "a":
        files = [cw.coord_pair(n_rows, names, cols, tuples, kinds=["rrr", "sd"])]
    else:
        files = [cw.column_coord_file(n_rows, names, cols, tuples, kinds=["stat", "sd_inv"], v2=True)]
    paths = cw.write_case(tmp_path, {"name": "world", "form": form, "files": files})
    D = aligner.Annotation.load(paths, on_device=True, coordinates=True)
    H = aligner.Annotation.load(paths, coordinates=True)
    assert D.has_coordinates() and H.has_coordinates() and D.labels == H.labels == names and D.n_rows == H.n_rows == n_rows
    if form == "a":                    # (the plain loader keeps ignoring the side file)
        assert not aligner.Annotation.load(paths, on_device=True).has_coordinates()
    rows = list(range(n_rows)) + [n_rows, n_rows + 5, 2 ** 40]
    want = per_row + [[], [], []]
    assert D.get_row_tuples(rows) == want
    assert H.get_row_tuples(rows) == want
    # LabeledAligner with such an annotation chains seeds: not on the device -> still refused
    W, last, F, valid = g.export()
    G = aligner.Graph(k, W, last, F, valid)
    out = C.c_void_p()
    cfg = capi.config_cli(k)
    for AN in (D, H):
        assert capi.lib().mgx_labeled_aligner_create(G.h, C.byref(cfg), None, AN.h, C.byref(out)) == capi.MGX_ERR_UNSUPPORTED


def sparse_input(rng, n_rows, n_labels):
    """shuffled columns: rows in any order within a column, tuples of 0 to 70 ascending coordinates"""
    col_begin, rows, coord_begin, coords = [0], [], [0], []
    for j in range(n_labels):
        mine = rng.sample(range(n_rows), rng.randrange(0, (n_rows + 1) // 2 + 1))
        for r in mine:
            rows.append(r)
            ln = rng.choice([0, 1, 1, 1, 2, 3, 70])
            coords += sorted(rng.randrange(-50, 10 ** 12) for _ in range(ln))
            coord_begin.append(len(coords))
        col_begin.append(len(rows))
    return (np.array(col_begin, dtype=np.uint64), np.array(rows, dtype=np.uint64), np.array(coord_begin, dtype=np.uint64),
            np.array(coords, dtype=np.int64))


def set_coordinates(A, cb, rows, cob, co, on_device):
    L = capi.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    if not on_device:
        L.mgx_annotation_set_coordinates.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        return L.mgx_annotation_set_coordinates(A.h, C.c_uint32(len(cb) - 1), p(cb), p(rows), p(cob), p(co))
    import torch
    dev = [torch.from_numpy(a.view(np.int64)).cuda() if len(a) else torch.zeros(1, dtype=torch.int64, device="cuda") for a in (rows, cob, co)]
    torch.cuda.synchronize()
    L.mgx_annotation_set_coordinates_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L.mgx_annotation_set_coordinates_device(A.h, len(cb) - 1, p(cb), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())


@pytest.mark.parametrize("n_rows,n_labels", [(1, 1), (65, 3), (5000, 40)])
def test_device_transposition_equals_the_host_one(n_rows, n_labels):
    rng = random.Random(n_rows)
    cb, rows, cob, co = sparse_input(rng, n_rows, n_labels)
    H = aligner.Annotation.from_sparse(n_rows, cb, rows)
    D = aligner.Annotation.from_sparse(n_rows, cb, rows)
    assert set_coordinates(H, cb, rows, cob, co, False) == 0, capi.lib().mgx_last_error()
    assert set_coordinates(D, cb, rows, cob, co, True) == 0, capi.lib().mgx_last_error()
    assert D.has_coordinates()
    ask = list(range(n_rows)) + [n_rows]
    got = D.get_row_tuples(ask)
    assert got == H.get_row_tuples(ask)
    want = [[] for _ in ask]
    for j in range(n_labels):
        for x in range(int(cb[j]), int(cb[j + 1])):
            want[int(rows[x])].append((j, co[int(cob[x]):int(cob[x + 1])].tolist()))
    assert got == [sorted(w) for w in want]
    assert D.device_bytes == H.device_bytes


def test_device_transposition_refuses_as_the_host_one():
    rng = random.Random(3)
    n_rows = 300
    cb, rows, cob, co = sparse_input(rng, n_rows, 4)
    L = capi.lib()
    outside = rows.copy()
    outside[len(rows) // 2] = n_rows
    x = next(x for x in range(len(rows)) if cob[x + 1] - cob[x] >= 2)
    descending = co.copy()
    descending[int(cob[x])], descending[int(cob[x]) + 1] = 9, 8
    both = (outside, descending)                                  # a row outside the matrix is named first, as the host finds it
    for bad_rows, bad_co, words in ((outside, co, "a row index is outside the matrix"), (rows, descending, "coordinates must be ascending"),
                                    (both[0], both[1], "a row index is outside the matrix")):
        msgs = []
        for on_device in (False, True):
            A = aligner.Annotation.from_sparse(n_rows, cb, rows)
            assert set_coordinates(A, cb, bad_rows, cob, bad_co, on_device) == capi.MGX_ERR_INVALID
            msgs.append(L.mgx_last_error().decode())
            assert not A.has_coordinates()
        assert msgs[0] == msgs[1] and words in msgs[0], msgs


def load_counted(paths):
    L = capi.lib()
    h = C.c_void_p()
    before = counts()
    assert L.mgx_annotation_load_coord_columns_device(c_paths(paths), len(paths), 0, C.byref(h), None) == 0, L.mgx_last_error()
    after = counts()
    L.mgx_annotation_destroy(h)
    return [a - b for a, b in zip(after, before)]


def test_launches_and_allocations_do_not_depend_on_the_number_of_columns(tmp_path):
    small, large = cases.count_mix(3), cases.count_mix(40)
    c3, c40 = load_counted(cw.write_case(tmp_path, small)), load_counted(cw.write_case(tmp_path, large))
    assert c3[0] == c40[0] > 0 and c3[1] == c40[1] > 0, (c3, c40)
    for case, c in ((small, c3), (large, c40)):
        # down: the per-label counts and the error record (read twice) — no row index, no coordinate
        assert c[3] <= 8 * len(case["labels"]) + 16, c


@pytest.mark.parametrize("name,form,files,code,words", cases.damaged(), ids=lambda x: x if isinstance(x, str) and "_" in x and " " not in x else None)
def test_damaged_files_fail_alike(name, form, files, code, words, tmp_path):
    paths = cw.write_case(tmp_path, {"name": name, "form": form, "files": files})
    for call in ("hook", "load"):
        errs = []
        for on_device in (False, True):
            with pytest.raises(aligner.MgxError) as e:
                if call == "load":
                    aligner.Annotation.load(paths, on_device=on_device, coordinates=True)
                else:
                    aligner.read_column_files(paths, on_device=on_device, coordinates=True)
            errs.append(e.value)
        assert errs[0].code == errs[1].code == getattr(capi, code), (str(errs[0]), str(errs[1]))
        assert str(errs[0]) == str(errs[1]) and words in str(errs[0]), (str(errs[0]), str(errs[1]))


def test_names_out_holds_no_rows_and_no_coordinates(tmp_path):
    case = next(c for c in cases.well_formed() if c["name"] == "one_rrr")
    paths = cw.write_case(tmp_path, case)
    L = capi.lib()
    h, names, h2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.mgx_annotation_load_coord_columns_device(c_paths(paths), len(paths), 0, C.byref(h), C.byref(names)) == 0, L.mgx_last_error()
    try:
        assert L.mgx_column_file_num_rows(names) == case["n_rows"] and L.mgx_column_file_num_labels(names) == 1
        assert L.mgx_column_file_label(names, 0).decode() == "only"
        assert np.ctypeslib.as_array(L.mgx_column_file_col_begin(names), shape=(2,)).tolist() == [0, 3]
        assert not L.mgx_column_file_rows(names) and not L.mgx_column_file_coord_begin(names) and not L.mgx_column_file_coords(names)
        assert L.mgx_annotation_create_from_file(names, 0, C.byref(h2)) == capi.MGX_ERR_INVALID and not h2
        L.mgx_annotation_has_coordinates.argtypes = [C.c_void_p]
        assert L.mgx_annotation_has_coordinates(h) == 1
    finally:
        L.mgx_column_file_free(names)
        L.mgx_annotation_destroy(h)
