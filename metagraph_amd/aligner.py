"""Thin Python plumbing over libmgx.so (ctypes).  Mirrors the reference's operator surface for the
alignment path: `Graph` ~ DBGSuccinct (BOSS view upload), `Aligner.align_batch` ~
IDBGAligner::align_batch (graph/alignment/dbg_aligner.hpp:20-39).  No compute happens in Python and
there is no CPU fallback: every call below fails loudly without the HIP library / a GPU.
"""
import ctypes as C

import numpy as np

from . import capi


class MgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mgx error %d: %s" % (code, msg))
        self.code = code


def _check(rc):
    if rc != capi.MGX_OK:
        raise MgxError(rc, capi.lib().mgx_last_error().decode())


def pack_queries(queries):
    offs = np.zeros(len(queries) + 1, dtype=np.uint64)
    bs = [q if isinstance(q, bytes) else q.encode("latin-1") for q in queries]
    for i, b in enumerate(bs):
        offs[i + 1] = offs[i] + len(b)
    return b"".join(bs), offs


def read_boss_file(path, arrays=True, on_device=False, device=0):
    """mgx_boss_file_read (host only, no GPU): k, sigma, mode, state, n_edges, F and — with arrays — W / last of a `.dbg` file.
    on_device: mgx_boss_file_decode_device, the same content decoded by the kernels of mgx_graph_load_dbg_device and copied back."""
    L = capi.lib()
    f = capi.BossFile()
    if on_device:
        _check(L.mgx_boss_file_decode_device(str(path).encode(), device, C.byref(f)))
    else:
        _check(L.mgx_boss_file_read(str(path).encode(), C.byref(f)))
    try:
        out = {"k": f.k, "sigma": f.sigma, "mode": f.mode, "state": f.state, "n_edges": f.n_edges, "F": [int(f.F[i]) for i in range(f.sigma)]}
        if arrays:
            out["W"] = np.ctypeslib.as_array(f.W, shape=(f.n_edges + 1,)).copy()
            out["last"] = np.ctypeslib.as_array(f.last, shape=(f.n_edges + 1,)).copy()
        return out
    finally:
        L.mgx_boss_file_free(C.byref(f))


def read_edgemask(path, state, n_edges):
    """mgx_edgemask_read (host only): the valid-edge bytes (mgx_boss_view.valid) of the `.edgemask` next to a `.dbg`"""
    out = np.zeros(n_edges + 1, dtype=np.uint8)
    _check(capi.lib().mgx_edgemask_read(str(path).encode(), state, n_edges, out.ctypes.data))
    return out


def read_column_files(paths, on_device=False, device=0, coordinates=False):
    """mgx_column_file_read (host only): (n_rows, label names, col_begin, rows) of one or several `.column.annodbg` files.
    on_device: mgx_column_file_decode_device, the same content decoded by the kernels of mgx_annotation_load_columns_device and
    copied back.  coordinates: mgx_column_coord_file_read / mgx_column_coord_file_decode_device over `.column.annodbg` files with
    their `.coords` side files, or one `.column_coord.annodbg`; the tuple grows by (coord_begin, coords)."""
    L = capi.lib()
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    h = C.c_void_p()
    if coordinates:
        _check((L.mgx_column_coord_file_decode_device(arr, len(paths), device, C.byref(h)) if on_device else L.mgx_column_coord_file_read(arr, len(paths), C.byref(h))))
    elif on_device:
        _check(L.mgx_column_file_decode_device(arr, len(paths), device, C.byref(h)))
    else:
        _check(L.mgx_column_file_read(arr, len(paths), C.byref(h)))
    try:
        n = L.mgx_column_file_num_labels(h)
        names = [L.mgx_column_file_label(h, j).decode() for j in range(n)]
        cb = np.ctypeslib.as_array(L.mgx_column_file_col_begin(h), shape=(n + 1,)).copy()
        rows = np.ctypeslib.as_array(L.mgx_column_file_rows(h), shape=(int(cb[-1]),)).copy() if int(cb[-1]) else np.zeros(0, dtype=np.uint64)
        if coordinates:
            cob = np.ctypeslib.as_array(L.mgx_column_file_coord_begin(h), shape=(int(cb[-1]) + 1,)).copy()
            co = np.ctypeslib.as_array(L.mgx_column_file_coords(h), shape=(int(cob[-1]),)).copy() if int(cob[-1]) else np.zeros(0, dtype=np.int64)
            return int(L.mgx_column_file_num_rows(h)), names, cb, rows, cob, co
        return int(L.mgx_column_file_num_rows(h)), names, cb, rows
    finally:
        L.mgx_column_file_free(h)


def column_decode_kernel_launch_counts():
    """mgx_column_decode_kernel_launch_counts: [kernel launches, device allocations, bytes host-to-device, bytes device-to-host]
    of mgx_annotation_load_columns_device / mgx_column_file_decode_device since the library was loaded."""
    out = (C.c_uint64 * 4)()
    capi.lib().mgx_column_decode_kernel_launch_counts(out)
    return [int(x) for x in out]


class Graph:
    """A BOSS table on the GPU.  W/last: uint8 arrays of n_edges + 1 entries (slot 0 unused)."""

    def __init__(self, k, W, last, F, valid=None, device=0, on_device=False, mode=0):
        L = capi.lib()
        v = capi.BossView()
        v.k = k
        v.sigma = 5
        if on_device:      # (ptr, n_entries) pairs for W / last / valid
            v.n_edges = W[1] - 1
            v.W, v.last = W[0], last[0]
            v.valid = valid[0] if valid is not None else None
        else:
            W = np.ascontiguousarray(W, dtype=np.uint8)
            last = np.ascontiguousarray(last, dtype=np.uint8)
            v.n_edges = len(W) - 1
            v.W, v.last = W.ctypes.data, last.ctypes.data
            if valid is not None:
                valid = np.ascontiguousarray(valid, dtype=np.uint8)
                v.valid = valid.ctypes.data
        Fc = (C.c_uint64 * 5)(*[int(x) for x in F])
        v.F = C.cast(Fc, C.POINTER(C.c_uint64))
        v.mode = mode
        v.on_device = 1 if on_device else 0
        self.h = C.c_void_p()
        _check(L.mgx_graph_create(C.byref(v), device, C.byref(self.h)))
        self.k = k
        self.n_edges = v.n_edges

    @classmethod
    def load(cls, path, device=0, on_device=False):
        """mgx_graph_load_dbg: a `.dbg` file written by the reference (DBGSuccinct::load, dbg_succinct.cpp:690-785).
        on_device: mgx_graph_load_dbg_device, the file's payloads decoded by kernels (the same graph)."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        load = capi.lib().mgx_graph_load_dbg_device if on_device else capi.lib().mgx_graph_load_dbg
        _check(load(str(path).encode(), device, C.byref(self.h)))
        self.k = capi.lib().mgx_graph_k(self.h)
        self.n_edges, self.mode = capi.lib().mgx_graph_num_edges(self.h), capi.lib().mgx_graph_mode(self.h)
        return self

    def close(self):
        if getattr(self, "h", None) and capi is not None:      # capi is None during interpreter shutdown
            capi.lib().mgx_graph_destroy(self.h)
            self.h = None

    __del__ = close

    @property
    def device_bytes(self):
        return capi.lib().mgx_graph_device_bytes(self.h)


class Annotation:
    """The label matrix of an annotated graph on the GPU (mgx_annotation_create): columns[j] = the bit vector of label j over the
    rows (row = node - 1), 64 rows per uint64 word."""

    def __init__(self, n_rows, columns, device=0):
        self._cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
        ptrs = (C.c_void_p * max(1, len(self._cols)))(*[c.ctypes.data for c in self._cols])
        self.h = C.c_void_p()
        self.n_rows, self.n_labels = n_rows, len(self._cols)
        _check(capi.lib().mgx_annotation_create(n_rows, len(self._cols), ptrs, device, C.byref(self.h)))

    @classmethod
    def from_sparse(cls, n_rows, col_begin, rows, device=0, on_device=False):
        """mgx_annotation_create_sparse: rows[col_begin[j] : col_begin[j + 1]] = the rows with label j (a ColumnCompressed
        annotation's content).  col_begin: host uint64 array of n_labels + 1 entries; rows: host uint64 array, or a device
        pointer with on_device=True."""
        self = cls.__new__(cls)
        cb = np.ascontiguousarray(col_begin, dtype=np.uint64)
        self._cols = [cb]
        rp = rows
        if not on_device:
            r = np.ascontiguousarray(rows, dtype=np.uint64)
            self._cols.append(r)
            rp = r.ctypes.data
        self.h = C.c_void_p()
        self.n_rows, self.n_labels = n_rows, len(cb) - 1
        _check(capi.lib().mgx_annotation_create_sparse(n_rows, len(cb) - 1, cb.ctypes.data, rp, 1 if on_device else 0, device, C.byref(self.h)))
        return self

    @classmethod
    def load(cls, paths, device=0, on_device=False, coordinates=False):
        """`.column.annodbg` files written by the reference (ColumnCompressed::load / merge_load); label names in .labels.
        on_device: mgx_annotation_load_columns_device, the columns decoded by kernels (the same annotation).
        coordinates: the files' k-mer coordinates too (`.coords` side files, or one `.column_coord.annodbg`):
        mgx_column_coord_file_read + mgx_annotation_create_from_file, or mgx_annotation_load_coord_columns_device on_device."""
        if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
            paths = [paths]
        L = capi.lib()
        if coordinates and not on_device:
            arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
            f = C.c_void_p()
            _check(L.mgx_column_coord_file_read(arr, len(paths), C.byref(f)))
            try:
                self = cls.__new__(cls)
                self.h = C.c_void_p()
                self._cols = []
                _check(L.mgx_annotation_create_from_file(f, device, C.byref(self.h)))
                self.n_rows, self.n_labels = int(L.mgx_column_file_num_rows(f)), int(L.mgx_column_file_num_labels(f))
                self.labels = [L.mgx_column_file_label(f, j).decode() for j in range(self.n_labels)]
            finally:
                L.mgx_column_file_free(f)
            return self
        if on_device:
            arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
            self = cls.__new__(cls)
            self.h, names = C.c_void_p(), C.c_void_p()
            self._cols = []
            load = L.mgx_annotation_load_coord_columns_device if coordinates else L.mgx_annotation_load_columns_device
            _check(load(arr, len(paths), device, C.byref(self.h), C.byref(names)))
            try:
                self.n_rows, self.n_labels = int(L.mgx_column_file_num_rows(names)), int(L.mgx_column_file_num_labels(names))
                self.labels = [L.mgx_column_file_label(names, j).decode() for j in range(self.n_labels)]
            finally:
                L.mgx_column_file_free(names)
            return self
        n_rows, names, cb, rows = read_column_files(paths)
        self = cls.from_sparse(n_rows, cb, rows, device=device)
        self.labels = names
        return self

    @property
    def device_bytes(self):
        return capi.lib().mgx_annotation_device_bytes(self.h)

    def set_coordinates(self, col_begin, rows, coord_begin, coords):
        """mgx_annotation_set_coordinates on an annotation made by from_sparse(n_rows, col_begin, rows): pair x has the ascending
        coordinates coords[coord_begin[x] : coord_begin[x + 1]] (host arrays)."""
        cb, r = np.ascontiguousarray(col_begin, dtype=np.uint64), np.ascontiguousarray(rows, dtype=np.uint64)
        cob, co = np.ascontiguousarray(coord_begin, dtype=np.uint64), np.ascontiguousarray(coords, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        _check(capi.lib().mgx_annotation_set_coordinates(C.c_void_p(self.h.value), C.c_uint32(len(cb) - 1), p(cb), p(r), p(cob),
                                                         co.ctypes.data_as(C.POINTER(C.c_int64))))

    def has_coordinates(self):
        """AnnotationBuffer::has_coordinates: the annotation carries k-mer coordinates"""
        return bool(capi.lib().mgx_annotation_has_coordinates(self.h))

    def get_row_tuples(self, rows):
        """mgx_annotation_get_row_tuples (MultiIntMatrix::get_row_tuples): per requested row its [(label, [coordinates])], labels
        ascending; a row outside the matrix has none."""
        L = capi.lib()
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(rows)
        begin = np.zeros(n + 1, dtype=np.uint64)
        u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        ptr = lambda a, t: a.ctypes.data_as(t)
        label_cap, coord_cap = max(16, 2 * n), max(16, 4 * n)
        while True:
            labels = np.zeros(label_cap, dtype=np.uint32)
            cbegin = np.zeros(label_cap + 1, dtype=np.uint64)
            coords = np.zeros(coord_cap, dtype=np.int64)
            nl, nc = C.c_uint64(), C.c_uint64()
            rc = L.mgx_annotation_get_row_tuples(C.c_void_p(self.h.value), ptr(rows, u64p), C.c_uint64(n), ptr(begin, u64p), ptr(labels, C.POINTER(C.c_uint32)),
                                                 C.c_uint64(label_cap), ptr(cbegin, u64p), ptr(coords, i64p), C.c_uint64(coord_cap), C.byref(nl), C.byref(nc))
            if rc == capi.MGX_ERR_CAPACITY and (nl.value > label_cap or nc.value > coord_cap):
                label_cap, coord_cap = max(label_cap, nl.value), max(coord_cap, nc.value)
                continue
            _check(rc)
            break
        return [[(int(labels[e]), coords[int(cbegin[e]):int(cbegin[e + 1])].tolist()) for e in range(int(begin[i]), int(begin[i + 1]))] for i in range(n)]

    def close(self):
        if getattr(self, "h", None) and capi is not None:
            capi.lib().mgx_annotation_destroy(self.h)
            self.h = None

    __del__ = close


class Aligner:
    """DBGAligner<> on the GPU (default seeder/extender); with `annotation`: LabeledAligner<> (aligner_labeled.hpp:125-127)."""

    # kernel-selection options (mgx_aligner_set_pipeline "key=value") every new aligner starts with: all of them give the
    # same alignments; the parity suite sets this to run a kernel the automatic choice would not pick for its batch sizes
    default_options = ()

    def __init__(self, graph, config, limits=None, annotation=None):
        self.graph = graph
        self.annotation = annotation
        self.h = C.c_void_p()
        if annotation is not None:
            _check(capi.lib().mgx_labeled_aligner_create(graph.h, C.byref(config), C.byref(limits) if limits is not None else None,
                                                         annotation.h, C.byref(self.h)))
        else:
            _check(capi.lib().mgx_aligner_create(graph.h, C.byref(config), C.byref(limits) if limits is not None else None,
                                                 C.byref(self.h)))
        for opt in Aligner.default_options:
            self.set_pipeline(opt)

    def close(self):
        if getattr(self, "h", None) and capi is not None:
            capi.lib().mgx_aligner_destroy(self.h)
            self.h = None

    __del__ = close

    def get_config(self):
        c = capi.Config()
        _check(capi.lib().mgx_aligner_get_config(self.h, C.byref(c)))
        return c

    def align_batch(self, queries):
        """-> (list per query of alignment dicts, list of status codes)"""
        blob, offs = pack_queries(queries)
        res = capi.Results()
        _check(capi.lib().mgx_align_batch(self.h, blob, offs.ctypes.data, len(queries), 0, C.byref(res)))
        return capi.results_to_py(res), [res.status[i] for i in range(len(queries))]

    def align_device(self, seqs_ptr, offsets_ptr, n):
        """Reads already in HBM (device pointers); results stay on the device until fetch()."""
        _check(capi.lib().mgx_align_batch_device(self.h, seqs_ptr, offsets_ptr, n, 1))

    def align_batch_device(self, reads, first=0, n=None):
        """The records first .. first + n of a ParsedReads (ReadParser.parse) from the parser's device arrays; results stay on
        the device until fetch() / format_tsv_batch(reads.names_of(first, n))."""
        seqs, offsets, n = reads.device_slice(first, n)
        _check(capi.lib().mgx_align_batch_device(self.h, seqs, offsets, n, 1))

    def fetch(self):
        res = capi.Results()
        _check(capi.lib().mgx_fetch_results(self.h, C.byref(res)))
        return res

    def decode_device(self):
        """mgx_decode_results_device: the results of the batch align_device / align_batch ran last in the mgx_results layout,
        decoded by kernels and left in device memory.  -> (capi.Results whose pointers are DEVICE memory owned by the aligner —
        not to be dereferenced on the host —, dict of the arrays' element counts: n_alignments, n_nodes, n_cigar, n_seq_bytes,
        n_labels).  Pre-retry: a capacity-status query has its status and no alignments."""
        res, sizes = capi.Results(), capi.ResultsSizes()
        _check(capi.lib().mgx_decode_results_device(self.h, C.byref(res), C.byref(sizes)))
        return res, {f[0]: int(getattr(sizes, f[0])) for f in capi.ResultsSizes._fields_}

    def map_batch(self, queries):
        blob, offs = pack_queries(queries)
        m = capi.Mapping()
        _check(capi.lib().mgx_map_batch(self.h, blob, offs.ctypes.data, len(queries), 0, C.byref(m)))
        out = []
        for q in range(len(queries)):
            b, e = m.node_begin[q], m.node_begin[q + 1]
            out.append(([m.nodes_fwd[i] for i in range(b, e)], [m.nodes_rc[i] for i in range(b, e)]))
        return out

    def map_summary(self, queries, map_length=0, want_nodes=False, keep_nodes=False):
        """`align --map` (mgx_map_summary_batch): DeBruijnGraph::map_to_nodes of every query summarised on the device.
        -> list of (n_discovered, n_kmers, n_unique); with want_nodes: (that list, list of node lists).  map_length 0 = k,
        0 < L < k = the windows of --align-length L.  The view itself is kept in self.last_map_summary for format_map.
        keep_nodes: the node array stays in device memory for format_map_batch(.., MGX_MAP_FMT_NODES); nothing more comes to
        the host.  queries: a list of str / bytes, or (seqs, offsets, n) device pointers (ParsedReads.device_slice)."""
        flags = (capi.MGX_MAP_WANT_NODES if want_nodes else 0) | (capi.MGX_MAP_KEEP_NODES if keep_nodes else 0)
        m = capi.MapSummary()
        if isinstance(queries, tuple):
            seqs, offsets, n_queries = queries
            _check(capi.lib().mgx_map_summary_batch(self.h, seqs, offsets, n_queries, 1, map_length, flags, C.byref(m)))
        else:
            blob, offs = pack_queries(queries)
            n_queries = len(queries)
            _check(capi.lib().mgx_map_summary_batch(self.h, blob, offs.ctypes.data, n_queries, 0, map_length, flags, C.byref(m)))
        self.last_map_summary = m
        counts = [(m.counts[q].n_discovered, m.counts[q].n_kmers, m.counts[q].n_unique) for q in range(n_queries)]
        if not want_nodes:
            return counts
        nb = np.ctypeslib.as_array(m.node_begin, shape=(n_queries + 1,))
        nodes = np.ctypeslib.as_array(m.nodes, shape=(max(1, int(nb[-1])),))
        return counts, [nodes[int(nb[q]):int(nb[q + 1])].tolist() for q in range(n_queries)]

    def map_present(self, counts, query_len, map_length=0, discovery_fraction=0.7):
        return map_present(counts, query_len, self.graph.k, map_length, discovery_fraction)

    def format_map(self, summary, qi, header, query, fmt, map_length=0, discovery_fraction=0.7):
        return format_map(summary, qi, header, query, self.graph.k, fmt, map_length, discovery_fraction)

    def format_map_batch(self, headers, fmt, discovery_fraction=0.7):
        """mgx_format_map_batch: the `align --map` text of the batch map_summary ran last, written by kernels (fmt =
        capi.MGX_MAP_FMT_*; MGX_MAP_FMT_NODES after map_summary(..., keep_nodes=True)).  headers: one str / bytes per query, or
        the (bytes, offsets) pair of ParsedReads.names_of.  -> (bytes of all queries' text in query order, numpy uint64 array of
        len(headers) + 1 offsets)."""
        blob, hoff, n_headers = _pack_headers(headers)
        t = capi.Text()
        _check(capi.lib().mgx_format_map_batch(self.h, blob, hoff.ctypes.data, fmt, discovery_fraction, C.byref(t)))
        return _text_of(t, n_headers, "format_map_batch: %d headers for a batch of %d queries")

    def set_pipeline(self, name):
        """Kernel selection: 'split8' (the name of the one pipeline: accepted, selects nothing), 'general' / 'chain'
        (extension chain path off / on), 'key=value' options (include/mgx.h lists them at mgx_aligner_set_pipeline);
        results never depend on it.  Anything else raises MgxError(MGX_ERR_INVALID)."""
        L = capi.lib()
        L.mgx_aligner_set_pipeline.argtypes = [C.c_void_p, C.c_char_p]
        _check(L.mgx_aligner_set_pipeline(self.h, name.encode()))

    def keep_seeds(self, keep=True):
        capi.lib().mgx_aligner_keep_seeds(self.h, int(keep))

    def seed_info(self, n):
        from . import _seedinfo
        return _seedinfo.fetch(self, n)

    def stats(self):
        s = capi.Stats()
        _check(capi.lib().mgx_aligner_stats(self.h, C.byref(s)))
        d = {f[0]: getattr(s, f[0]) for f in capi.Stats._fields_}
        d["phase_cycles"] = list(s.phase_cycles)
        d["extend_cycles"] = list(s.extend_cycles)
        d["lane_bail_reads"] = {i: int(v) for i, v in enumerate(s.lane_bail_reads) if v}
        d["seed_lane_left_reads"] = {i: int(v) for i, v in enumerate(s.seed_lane_left_reads) if v}
        return d

    def format_tsv(self, res, qi, header, query):
        q = query if isinstance(query, bytes) else query.encode("latin-1")
        cfg = self.get_config()
        n = capi.lib().mgx_format_tsv(C.byref(res), qi, header.encode(), q, len(q), cfg.min_path_score, None, 0)
        buf = C.create_string_buffer(n + 1)
        capi.lib().mgx_format_tsv(C.byref(res), qi, header.encode(), q, len(q), cfg.min_path_score, buf, n + 1)
        return buf.value.decode("latin-1")

    def format_json_batch(self, headers, first=0, n=None):
        """mgx_format_json_batch: the `align --json` text of queries first .. first + n (n = None: to the end) of the batch
        align_device / align_batch ran last, written by kernels.  headers: one str / bytes per query OF THE RANGE, or the
        (bytes, offsets) pair of ParsedReads.names_of(first, n).  JSON text is large (~60 bytes per path node): a caller bounds the
        text of one call by its range; the ranges' texts concatenated are the whole batch's.
        -> (bytes of the range's lines in query order, numpy uint64 array of n + 1 offsets: all lines of query first + i)."""
        blob, hoff, n_headers = _pack_headers(headers)
        n = n_headers if n is None else n
        if n != n_headers:
            raise ValueError("format_json_batch: %d headers for a range of %d queries" % (n_headers, n))
        t = capi.Text()
        _check(capi.lib().mgx_format_json_batch(self.h, blob, hoff.ctypes.data, first, n, C.byref(t)))
        return _text_of(t, n, "format_json_batch: %d headers for a range of %d queries")

    def format_tsv_batch(self, headers, label_names=None):
        """mgx_format_tsv_batch: the TSV text of the batch align_device / align_batch ran last, written by kernels.
        headers: one str / bytes per query; label_names: names of labels 0 .. len - 1 (label-aware aligners; others print as
        numbers).  -> (bytes of all lines in query order, numpy uint64 array of len(headers) + 1 line offsets)."""
        blob, hoff, n_headers = _pack_headers(headers)
        names = [n if isinstance(n, bytes) else n.encode() for n in (label_names or [])]
        arr = (C.c_char_p * len(names))(*names) if names else None
        t = capi.Text()
        _check(capi.lib().mgx_format_tsv_batch(self.h, blob, hoff.ctypes.data, arr, len(names), C.byref(t)))
        return _text_of(t, n_headers, "format_tsv_batch: %d headers for a batch of %d queries")


class SeedChainer(Aligner):
    """The chain stage of LabeledAligner's coordinate mode on the GPU (mgx_seed_chainer_create): reads in, per (query, strand) the
    seeds filter_seeds keeps and the finished tables of chain_seeds out.  graph: BASIC mode; annotation: with k-mer coordinates.
    Every other batch call of Aligner is refused on such a handle (MGX_ERR_UNSUPPORTED)."""

    def __init__(self, graph, config, annotation, limits=None):
        self.graph = graph
        self.annotation = annotation
        self.h = C.c_void_p()
        _check(capi.lib().mgx_seed_chainer_create(graph.h, C.byref(config), C.byref(limits) if limits is not None else None,
                                                  annotation.h, C.byref(self.h)))
        for opt in Aligner.default_options:
            self.set_pipeline(opt)

    def chain_tables(self, queries, on_device=False):
        """mgx_chain_tables_batch -> (arrays, status): arrays = the numpy copies of mgx_chain_tables (seed_begin, seeds, nodes,
        num_matching, list_begin, anchors, backtrace; chain_lists() splits them per list), status = one code per query.
        on_device: the tables stay in device memory (MGX_CHAIN_TABLES_ON_DEVICE) and -> the capi.ChainTables of device pointers,
        not to be dereferenced on the host; fetch_chain_tables() copies them."""
        blob, offs = pack_queries(queries)
        t = capi.ChainTables()
        _check(capi.lib().mgx_chain_tables_batch(self.h, blob, offs.ctypes.data, len(queries), 0,
                                                 capi.MGX_CHAIN_TABLES_ON_DEVICE if on_device else 0, C.byref(t)))
        return t if on_device else _chain_tables_of(t)

    def fetch_chain_tables(self):
        """mgx_chain_tables_fetch: the last on_device result as chain_tables() returns it"""
        t = capi.ChainTables()
        _check(capi.lib().mgx_chain_tables_fetch(self.h, C.byref(t)))
        return _chain_tables_of(t)


CHAIN_SEED_DTYPE = np.dtype([("clipping", "<u4"), ("length", "<u4"), ("offset", "<u4"), ("n_nodes", "<u4"), ("nodes_begin", "<u8")])
CHAIN_ANCHOR_DTYPE = np.dtype([("label", "<u8"), ("coordinate", "<i8"), ("seed_clipping", "<i4"), ("seed_end", "<i4"),
                               ("chain_score", "<i4"), ("seed_index", "<u4")])


def _chain_tables_of(t):
    """numpy copies of a host mgx_chain_tables -> (dict of arrays, list of status codes)"""
    n = int(t.n_queries)

    def arr(ptr, count, dtype):
        if not count:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype, count=count).copy()

    seed_begin, list_begin = arr(t.seed_begin, 2 * n + 1, np.uint64), arr(t.list_begin, 2 * n + 1, np.uint64)
    seeds = arr(t.seeds, int(seed_begin[-1]), CHAIN_SEED_DTYPE)
    n_nodes = int(seeds["n_nodes"].sum()) if len(seeds) else 0
    n_anchors = int(list_begin[-1])
    out = {"n": n, "seed_begin": seed_begin, "seeds": seeds, "nodes": arr(t.nodes, n_nodes, np.uint64),
           "num_matching": arr(t.num_matching, 2 * n, np.uint64), "list_begin": list_begin,
           "anchors": arr(t.anchors, n_anchors, CHAIN_ANCHOR_DTYPE), "backtrace": arr(t.backtrace, n_anchors, np.uint32)}
    return out, arr(t.status, n, np.int32).tolist()


def chain_lists(arrays):
    """The arrays of SeedChainer.chain_tables per list (list 2q = query q, 2q + 1 = its reverse complement): dicts of
    seeds [(clipping, length, offset, [nodes])] in chain_seeds' (reversed) order, num_matching,
    anchors [(label, coordinate, seed_clipping, seed_end, chain_score, seed_index)] and backtrace."""
    out = []
    nodes = arrays["nodes"]
    for l in range(2 * arrays["n"]):
        sb, se = int(arrays["seed_begin"][l]), int(arrays["seed_begin"][l + 1])
        lb, le = int(arrays["list_begin"][l]), int(arrays["list_begin"][l + 1])
        seeds = [(int(s["clipping"]), int(s["length"]), int(s["offset"]),
                  nodes[int(s["nodes_begin"]):int(s["nodes_begin"]) + int(s["n_nodes"])].tolist()) for s in arrays["seeds"][sb:se]]
        out.append({"seeds": seeds, "num_matching": int(arrays["num_matching"][l]),
                    "anchors": [tuple(int(x) for x in a) for a in arrays["anchors"][lb:le].tolist()],
                    "backtrace": arrays["backtrace"][lb:le].tolist()})
    return out


def chain_tables_kernel_launch_counts():
    """mgx_chain_tables_kernel_launch_counts -> (kernel launches and device-library calls of the chain stage, device buffers it took
    or grew, bytes host-to-device, bytes device-to-host) since the library was loaded"""
    return _four_counts(capi.lib().mgx_chain_tables_kernel_launch_counts)


def _text_of(t, n_headers, mismatch):
    """the shared tail of the format_*_batch methods: the header count against the mgx_text's n_queries (mismatch: the message of
    the ValueError), then -> (bytes of the text, numpy uint64 copy of its n_headers + 1 offsets)"""
    if t.n_queries != n_headers:
        raise ValueError(mismatch % (n_headers, t.n_queries))
    lb = np.ctypeslib.as_array(t.line_begin, shape=(n_headers + 1,)).copy()
    return (C.string_at(t.text, int(lb[-1])) if int(lb[-1]) else b""), lb


def _pack_headers(headers):
    """-> (bytes, uint64 offsets from 0, count) of a list of headers, or of the flat (bytes, offsets) pair of ParsedReads.names_of"""
    if isinstance(headers, tuple) and len(headers) == 2 and isinstance(headers[1], np.ndarray):
        blob, hoff = headers
        return blob, hoff, len(hoff) - 1
    hs = [h if isinstance(h, bytes) else h.encode("latin-1") for h in headers]
    hoff = np.zeros(len(hs) + 1, dtype=np.uint64)
    if hs:
        hoff[1:] = np.cumsum([len(h) for h in hs])
    return b"".join(hs), hoff, len(hs)


class ParsedReads:
    """What ReadParser.parse returns: a view of the parser's arrays, valid until its next parse.  n_records, consumed, format;
    seqs / offsets: device pointers (ints); host_offsets, name_offsets: numpy uint64 copies; names: bytes (all names, end to end)."""

    def __init__(self, parser, r):
        self.parser = parser
        self.n_records, self.consumed, self.format = int(r.n_records), int(r.consumed), int(r.format)
        self.seqs, self.offsets = r.seqs, r.offsets
        n = self.n_records
        self.host_offsets = np.ctypeslib.as_array(r.host_offsets, shape=(n + 1,)).copy()
        self.name_offsets = np.ctypeslib.as_array(r.name_offsets, shape=(n + 1,)).copy()
        self.names = C.string_at(r.names, int(self.name_offsets[n])) if int(self.name_offsets[n]) else b""

    def name_list(self):
        o = self.name_offsets
        return [self.names[int(o[r]):int(o[r + 1])] for r in range(self.n_records)]

    def names_of(self, first=0, n=None):
        """the names of records first .. first + n as (bytes, offsets from 0): the headers of Aligner.format_tsv_batch"""
        n = self.n_records - first if n is None else n
        o = self.name_offsets[first:first + n + 1]
        return self.names[int(o[0]):int(o[-1])], np.ascontiguousarray(o - o[0])

    def device_slice(self, first=0, n=None):
        """-> (seqs, offsets, n): device pointers of the sub-batch, offsets from 0 (mgx_read_parser_slice)"""
        n = self.n_records - first if n is None else n
        seqs, offsets = C.c_void_p(), C.c_void_p()
        _check(capi.lib().mgx_read_parser_slice(self.parser.h, first, n, C.byref(seqs), C.byref(offsets)))
        return seqs, offsets, n

    def to_host(self):
        """-> (seqs bytes, offsets numpy uint64): the sequences copied back (mgx_read_parser_fetch)"""
        total = int(self.host_offsets[-1])
        buf = C.create_string_buffer(max(1, total))
        offs = np.zeros(self.n_records + 1, dtype=np.uint64)
        _check(capi.lib().mgx_read_parser_fetch(self.parser.h, buf, offs.ctypes.data))
        return buf.raw[:total], offs


class ReadParser:
    """mgx_read_parser: FASTA / FASTQ text to read batches on the device, no per-record work on the host."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(capi.lib().mgx_read_parser_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and capi is not None:
            capi.lib().mgx_read_parser_destroy(self.h)
            self.h = None

    __del__ = close

    def parse(self, data, final=True, text_on_device=False, flags=0, n_bytes=None):
        """data: bytes-like host text, or with text_on_device a device pointer (int) and n_bytes.  final=False: only complete
        records are consumed (ParsedReads.consumed says where the next chunk starts; pass the first chunk's format as flags).
        Outside the grammar: MgxError(MGX_ERR_INVALID) naming the byte position."""
        r = capi.Reads()
        if text_on_device:
            ptr, n = data, n_bytes
        else:
            keep = np.frombuffer(data, dtype=np.uint8)
            ptr, n = (keep.ctypes.data if len(keep) else None), len(keep)
        _check(capi.lib().mgx_parse_reads(self.h, ptr, n, int(bool(text_on_device)), int(bool(final)), flags, C.byref(r)))
        return ParsedReads(self, r)


def _four_counts(fn):
    out = (C.c_uint64 * 4)()
    fn(out)
    return tuple(int(x) for x in out)


def parse_kernel_launch_counts():
    """mgx_parse_kernel_launch_counts -> (line-pass kernel launches, copy-pass kernel launches, bytes host-to-device, bytes
    device-to-host) since the library was loaded"""
    return _four_counts(capi.lib().mgx_parse_kernel_launch_counts)


def format_kernel_launch_counts():
    """mgx_format_kernel_launch_counts -> (size kernel launches, write kernel launches, host-formatted lines, bytes copied
    device-to-host by format_tsv_batch) since the library was loaded"""
    return _four_counts(capi.lib().mgx_format_kernel_launch_counts)


def format_json_kernel_launch_counts():
    """mgx_format_json_kernel_launch_counts -> (size kernel launches, write kernel launches, queries formatted on the host, bytes
    copied device-to-host by format_json_batch) since the library was loaded"""
    return _four_counts(capi.lib().mgx_format_json_kernel_launch_counts)


def decode_kernel_launch_counts():
    """mgx_decode_kernel_launch_counts -> (size kernel launches, write kernel launches, bytes copied device-to-host by the decode,
    mgx_fetch_results calls the option decode_on_device served) since the library was loaded"""
    return _four_counts(capi.lib().mgx_decode_kernel_launch_counts)


def format_map_kernel_launch_counts():
    """mgx_format_map_kernel_launch_counts -> (size kernel launches, write kernel launches, bytes copied device-to-host, bytes
    copied host-to-device by format_map_batch) since the library was loaded"""
    return _four_counts(capi.lib().mgx_format_map_kernel_launch_counts)


def map_present(counts, query_len, k, map_length=0, discovery_fraction=0.7):
    """mgx_map_present (host only): --query-presence of one query from its (n_discovered, n_kmers, n_unique)."""
    c = capi.MapCounts(*counts)
    return bool(capi.lib().mgx_map_present(C.byref(c), query_len, k, map_length, discovery_fraction))


def format_map(summary, qi, header, query, k, fmt, map_length=0, discovery_fraction=0.7):
    """mgx_format_map (host only): the bytes `metagraph align --map` prints for query qi of a capi.MapSummary; fmt = capi.MGX_MAP_FMT_*."""
    q = query if isinstance(query, bytes) else query.encode("latin-1")
    args = (C.byref(summary), qi, header.encode(), q, len(q), k, map_length, fmt, discovery_fraction)
    n = capi.lib().mgx_format_map(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    capi.lib().mgx_format_map(*args, buf, n + 1)
    return buf.value.decode("latin-1")
