"""`.column.annodbg` files decoded by kernels (mgx_annotation_load_columns_device, the hook mgx_column_file_decode_device;
csrc/mgx_colload.hip) against the host reader (mgx_column_file_read + mgx_annotation_create_from_file): the same tables entry for
entry, the same annotation, the same refusals.  Only well-formed files and files the HOST part refuses reach the device here; what
a damaged payload does to the kernel bodies is tested on the CPU (tests/test_col_decode_model.py).  Needs a real MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import col_decode_cases as cases
import orc
import sdsl_writer as sw
from labeled_worlds import labeled_world, with_labels
from metagraph_amd import aligner, capi
from test_boss_files import GOLD
from test_gpu_annotation import device_rows

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metagraph_amd", "_build", "mgx_align")
GOLDEN = [os.path.join(GOLD, "test_DNA_graph.column.annodbg"), os.path.join(GOLD, "test_Protein_graph.column.annodbg")]
# device-to-host bytes of a load besides the 8 bytes per label: the error record, read after the count pass and after the write pass
D2H_CONSTANT = 16

counts = aligner.column_decode_kernel_launch_counts


def write_case(d, case):
    paths = []
    for i, data in enumerate(case["files"]):
        p = d / ("%s_%d.column.annodbg" % (case["name"], i))
        p.write_bytes(data)
        paths.append(p)
    return paths


def same_tables(paths):
    h, d = aligner.read_column_files(paths), aligner.read_column_files(paths, on_device=True)
    assert h[0] == d[0] and h[1] == d[1], (paths, "n_rows / labels")
    assert np.array_equal(h[2], d[2]), (paths, "col_begin", np.flatnonzero(h[2] != d[2])[:8])
    assert np.array_equal(h[3], d[3]), (paths, "rows", np.flatnonzero(h[3] != d[3])[:8])
    return h


def test_hook_gives_the_host_readers_tables(tmp_path):
    for case in cases.well_formed():
        n_rows, names, cb, rows = same_tables(write_case(tmp_path, case))
        assert (n_rows, names, int(cb[-1])) == (case["n_rows"], case["labels"], sum(len(c) for c in case["columns"])), case["name"]
    for p in GOLDEN:
        assert len(same_tables([p])[3]) > 0


def load_both(paths):
    return aligner.Annotation.load(paths), aligner.Annotation.load(paths, on_device=True)


def test_loaded_annotation_answers_alike(tmp_path):
    for name in ("rows129", "rows3001", "cols300_v2", "merge3", "no_labels"):
        case = next(c for c in cases.well_formed() if c["name"] == name)
        H, D = load_both(write_case(tmp_path, case))
        assert (D.n_rows, D.n_labels, D.labels) == (H.n_rows, H.n_labels, H.labels) == (case["n_rows"], len(case["labels"]), case["labels"])
        rows = list(range(case["n_rows"]))
        got = device_rows(D.h, rows)
        assert got == device_rows(H.h, rows), name
        want = [[] for _ in rows]
        for j, col in enumerate(case["columns"]):
            for r in col:
                want[r].append(j)
        assert got == want, name
    H, D = load_both([GOLDEN[0]])
    assert D.labels == H.labels and device_rows(D.h, list(range(D.n_rows))) == device_rows(H.h, list(range(H.n_rows)))


def world_files(tmp_path, mask):
    k = 15
    g, anno, reads = labeled_world(11, k, n_strains=3, n_reads=24, mask=mask)
    cols = []
    for j in range(anno.n_labels):
        words = anno.column_words(j)
        cols.append([r for r in range(g.n_edges) if (int(words[r >> 6]) >> (r & 63)) & 1])
    a, b = tmp_path / "a.column.annodbg", tmp_path / "b.column.annodbg"
    names = ["lab%d" % j for j in range(anno.n_labels)]
    a.write_bytes(sw.column_file(g.n_edges, names[:3], cols[:3], codes=[sw.CODE_SD, sw.CODE_STAT, sw.CODE_RRR], v2=True))
    b.write_bytes(sw.column_file(g.n_edges, names[3:], cols[3:]))
    return k, g, anno, reads, [a, b], names


def test_label_aware_batch_through_both(tmp_path):
    k, g, anno, reads, paths, names = world_files(tmp_path, True)
    W, last, F, valid = g.export()
    G = aligner.Graph(k, W, last, F, valid)
    cfg = capi.config_cli(k)
    want = with_labels(orc.LabeledAlignRun(g, cfg, anno, reads))
    assert sum(len(w) for w in want) > 0
    for AN in load_both(paths):
        assert AN.labels == names
        got, status = aligner.Aligner(G, cfg, annotation=AN).align_batch(reads)
        assert all(s == 0 for s in status) and got == want


def both_fail(paths, call):
    """the host path's error and the device path's: the same code, the same message"""
    errs = []
    for on_device in (False, True):
        with pytest.raises(aligner.MgxError) as e:
            if call == "load":
                aligner.Annotation.load(paths, on_device=on_device)
            else:
                aligner.read_column_files(paths, on_device=on_device)
        errs.append(e.value)
    assert errs[0].code == errs[1].code and str(errs[0]) == str(errs[1]), (str(errs[0]), str(errs[1]))
    return errs[0]


@pytest.mark.parametrize("call", ["load", "hook"])
def test_refusals_of_the_header_walk(tmp_path, call):
    before = counts()
    for name, data, code, words in cases.header_refusals():
        e = both_fail(write_case(tmp_path, {"name": name, "files": [data]}), call)
        assert e.code == getattr(capi, code) and words in str(e), (name, str(e))
    for name, files, code, words in cases.bad_merges():
        e = both_fail(write_case(tmp_path, {"name": name, "files": files}), call)
        assert e.code == getattr(capi, code) and words in str(e), (name, str(e))
    e = both_fail([tmp_path / "does_not_exist.column.annodbg"], call)
    assert e.code == capi.MGX_ERR_INVALID and "cannot open" in str(e)
    assert counts()[:2] == before[:2]                          # refused on the host: no kernel ran, nothing was allocated


def load_counted(paths):
    L = capi.lib()
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    h = C.c_void_p()
    before = counts()
    assert L.mgx_annotation_load_columns_device(arr, len(paths), 0, C.byref(h), None) == 0, L.mgx_last_error()
    after = counts()
    L.mgx_annotation_destroy(h)
    return [a - b for a, b in zip(after, before)]


@pytest.mark.parametrize("inverted", [False, True])
def test_launches_and_allocations_do_not_depend_on_the_number_of_columns(tmp_path, inverted):
    small, large = cases.count_mix(3, inverted), cases.count_mix(300, inverted)
    c3, c300 = load_counted(write_case(tmp_path, small)), load_counted(write_case(tmp_path, large))
    assert c3[0] == c300[0] > 0 and c3[1] == c300[1] > 0, (c3, c300)
    for case, c in ((small, c3), (large, c300)):
        n_labels, n_set = len(case["labels"]), sum(len(col) for col in case["columns"])
        assert c[3] <= 8 * n_labels + D2H_CONSTANT, c
        if n_labels == 300:
            assert 8 * n_set > 8 * n_labels + D2H_CONSTANT                  # (the rows' bytes would not fit under the bound)
        assert 0 < c[2] <= sum(len(f) for f in case["files"]) + 64 * 1024 + 200 * n_labels      # up: the payloads (+ tables, descriptors)


def test_names_out_holds_no_rows(tmp_path):
    case = next(c for c in cases.well_formed() if c["name"] == "cols3_v1")
    paths = write_case(tmp_path, case)
    L = capi.lib()
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    h, names, h2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.mgx_annotation_load_columns_device(arr, len(paths), 0, C.byref(h), C.byref(names)) == 0, L.mgx_last_error()
    try:
        assert L.mgx_column_file_num_rows(names) == case["n_rows"] and L.mgx_column_file_num_labels(names) == 3
        assert [L.mgx_column_file_label(names, j).decode() for j in range(3)] == case["labels"]
        cb = np.ctypeslib.as_array(L.mgx_column_file_col_begin(names), shape=(4,))
        assert cb.tolist() == np.cumsum([0] + [len(c) for c in case["columns"]]).tolist()
        assert not L.mgx_column_file_rows(names)
        assert L.mgx_annotation_create_from_file(names, 0, C.byref(h2)) == capi.MGX_ERR_INVALID
        assert b"names_out" in L.mgx_last_error() and not h2
    finally:
        L.mgx_column_file_free(names)
        L.mgx_annotation_destroy(h)


def test_driver_flag_prints_the_same_bytes(tmp_path):
    k, g, anno, reads, paths, names = world_files(tmp_path, False)
    W, last, F, _ = g.export()
    dbg = tmp_path / "g.dbg"
    dbg.write_bytes(sw.dbg_file(k, W, last, [int(x) for x in F]))
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    out = []
    for flags in ([], ["--load-on-device"]):
        r = subprocess.run([EXE, str(dbg), str(fa), "-a", str(paths[0]), "-a", str(paths[1])] + flags, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out.append(r.stdout)
    assert out[0] == out[1] and out[0].count(b"\n") >= len(reads) and b"lab0" in out[0]
