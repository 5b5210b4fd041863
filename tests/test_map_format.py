"""mgx_format_map / mgx_map_present (host code of libmgx.so, no GPU) on hand-built mgx_map_summary views: the reference's 21
`--map --count-kmers` lines byte for byte from their count triples, the "kmer: node" form, both presence formulas against a Python
restatement, the buffer-length convention."""
import ctypes as C

import pytest

from metagraph_amd import aligner, capi
from map_goldens import (BASIC_LINES, CANONICAL_LINES, K, SUBK_LENGTH, SUBK_LINES, present_full_k, present_sub_k, read_fastq, triples)

FRACTIONS = [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0]


def view(counts, node_lists=None):
    """a capi.MapSummary over Python data (the arrays are kept alive on the returned object)"""
    m = capi.MapSummary()
    m.n_queries = len(counts)
    m._counts = (capi.MapCounts * max(1, len(counts)))(*[capi.MapCounts(*c) for c in counts])
    m.counts = C.cast(m._counts, C.POINTER(capi.MapCounts))
    if node_lists is not None:
        begin = [0]
        for nl in node_lists:
            begin.append(begin[-1] + len(nl))
        flat = [v for nl in node_lists for v in nl]
        m._nb = (C.c_uint64 * len(begin))(*begin)
        m._nodes = (C.c_uint64 * max(1, len(flat)))(*flat)
        m.node_begin = C.cast(m._nb, C.POINTER(C.c_uint64))
        m.nodes = C.cast(m._nodes, C.POINTER(C.c_uint64))
    return m


@pytest.mark.parametrize("lines,map_length", [(BASIC_LINES, 0), (BASIC_LINES, K), (SUBK_LINES, SUBK_LENGTH), (CANONICAL_LINES, 0)])
def test_count_kmers_lines_byte_for_byte(lines, map_length):
    reads = read_fastq()
    assert len(reads) == len(lines) == 7
    m = view(triples(lines))
    for i, (name, seq) in enumerate(reads):
        got = aligner.format_map(m, i, name, seq, K, capi.MGX_MAP_FMT_COUNT_KMERS, map_length)
        assert got == lines[i] + "\n"


def test_kmer_node_form():
    seq = "ACGTNACGTAC"
    nodes = [5, 0, 18446744073709551615, 7, 12, 1, 2]          # 7 windows of 5
    m = view([(6, 7, 6), (0, 0, 0)], [nodes, []])
    got = aligner.format_map(m, 0, "r", seq, 5, capi.MGX_MAP_FMT_NODES)
    assert got == "".join("%s: %d\n" % (seq[i:i + 5], nodes[i]) for i in range(7))
    # --align-length 3 on a k = 5 graph: windows of 3 characters
    m3 = view([(9, 9, 9)], [list(range(1, 10))])
    assert aligner.format_map(m3, 0, "r", seq, 5, capi.MGX_MAP_FMT_NODES, 3) == "".join("%s: %d\n" % (seq[i:i + 3], i + 1) for i in range(9))
    assert aligner.format_map(m, 1, "short", "ACG", 5, capi.MGX_MAP_FMT_NODES) == ""
    # a view without node arrays (counts mode) has nothing to print in this form
    assert aligner.format_map(view([(6, 7, 6)]), 0, "r", seq, 5, capi.MGX_MAP_FMT_NODES) == ""


def test_presence_formulas_against_the_restatement():
    k = 11
    checked = 0
    for n_kmers in range(0, 301):
        found = sorted({0, 1, n_kmers // 10, n_kmers // 3, n_kmers // 2, (7 * n_kmers) // 10, (7 * n_kmers + 9) // 10,
                        (9 * n_kmers) // 10, max(0, n_kmers - 1), n_kmers} & set(range(n_kmers + 1)))
        for n_discovered in (range(n_kmers + 1) if n_kmers <= 40 else found):
            for f in FRACTIONS:
                c = (n_discovered, n_kmers, n_discovered)
                # map_length = k (given as 0 and as k): a query of n_kmers k-mers is n_kmers + k - 1 long; without k-mers it is shorter than k
                qlen = n_kmers + k - 1 if n_kmers else k - 1
                want = present_full_k(n_discovered, n_kmers, qlen, k, f)
                assert aligner.map_present(c, qlen, k, 0, f) == want, (c, f)
                assert aligner.map_present(c, qlen, k, k, f) == want, (c, f)
                # map_length = 7 < k: n_kmers windows
                want = present_sub_k(n_discovered, n_kmers, f)
                assert aligner.map_present(c, n_kmers + 6 if n_kmers else 3, k, 7, f) == want, (c, f)
                checked += 1
    assert checked > 20000
    for f in FRACTIONS:
        assert aligner.map_present((0, 0, 0), 10, 11, 0, f) is False          # len < k: absent (DeBruijnGraph::find)
        assert aligner.map_present((0, 0, 0), 5, 11, 7, f) is True            # no window at L < k: present (0 >= 0)


def test_presence_and_filter_text():
    reads = read_fastq()
    m = view(triples(CANONICAL_LINES))                  # 140, 140, 140, 129, 140, 2, 140 of 140
    for i, (name, seq) in enumerate(reads):
        d, n, _ = triples(CANONICAL_LINES)[i]
        for f in FRACTIONS:
            want = present_full_k(d, n, len(seq), K, f)
            assert aligner.format_map(m, i, name, seq, K, capi.MGX_MAP_FMT_QUERY_PRESENCE, 0, f) == ("1\n" if want else "0\n")
            assert aligner.format_map(m, i, name, seq, K, capi.MGX_MAP_FMT_FILTER_PRESENT, 0, f) == (">%s\n%s\n" % (name, seq) if want else "")
    assert aligner.format_map(m, 5, reads[5][0], reads[5][1], K, capi.MGX_MAP_FMT_QUERY_PRESENCE, 0, 0.7) == "0\n"
    assert aligner.format_map(m, 3, reads[3][0], reads[3][1], K, capi.MGX_MAP_FMT_QUERY_PRESENCE, 0, 0.9) == "1\n"      # 11 missing <= int(140 * 0.1) = 14


def test_buffer_length_convention():
    """as mgx_format_tsv: returns the bytes needed (without the NUL), writes at most buf_len bytes, always terminated"""
    L = capi.lib()
    m = view(triples(BASIC_LINES))
    name, seq = read_fastq()[0]
    want = (BASIC_LINES[0] + "\n").encode()
    args = (C.byref(m), 0, name.encode(), seq.encode(), len(seq), K, 0, capi.MGX_MAP_FMT_COUNT_KMERS, 0.7)
    assert L.mgx_format_map(*args, None, 0) == len(want)
    for cap in (1, 5, len(want), len(want) + 1, len(want) + 10):
        buf = C.create_string_buffer(b"\xff" * (len(want) + 16))
        assert L.mgx_format_map(*args, buf, cap) == len(want)
        wrote = min(cap, len(want) + 1)
        assert buf.raw[:wrote] == want[:wrote - 1] + b"\0" and buf.raw[wrote:wrote + 1] == b"\xff"
