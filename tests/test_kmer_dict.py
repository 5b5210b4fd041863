"""The plain k-mer dictionary (tests/kmer_dict.py) against the oracle, where both are cheap: the spelling of every edge and the
mapping of reads, BASIC and PRIMARY.  This pins the dictionary itself, so that the GPU tests of the mapping kernels
(tests/test_gpu_map_index_edges.py) may use it alone on graphs where the oracle would be slow.  CPU only."""
import pytest

import kmer_dict
import orc
from metagraph_amd import capi
from test_emu_vs_oracle import make_world, noisy_reads, rc
from test_oracle_canonical_wrapper import PRIMARY

WORLDS = [(k, mask) for k in (3, 5, 12, 31, 32, 40, 63) for mask in (False, True)]


def edge_reads(reads, k):
    return reads + ["", "A", reads[0][:k - 1], reads[0][:k], reads[1][:k + 1], "N" * (k + 5), reads[2].lower(),
                    reads[3][:k] + "n" + reads[3][k + 1:], reads[4].replace("T", "U"), reads[5][:40] + "\xc3" + reads[5][41:]]


@pytest.mark.parametrize("k,mask", WORLDS)
def test_spelling_and_mapping_equal_the_oracle(k, mask):
    g, reads = make_world(40 + k, k, mask=mask, genome_len=1500, n_reads=30, read_len=120)
    W, last, F, valid = g.export()
    assert (valid is not None) == mask
    edges, kmers = kmer_dict.spell_edges(k, W, last, F)
    spelled = dict(zip(edges.tolist(), kmers))
    n_real = 0
    for v in range(1, g.n_edges + 1):
        want = g.node_sequence(v)
        if "$" in want:
            assert v not in spelled, v
            continue
        n_real += 1
        got = kmer_dict.unpack_key(spelled[v], k) if k <= 32 else spelled[v].decode()
        assert got == want, v
    assert n_real == len(edges) and n_real > 40
    d = kmer_dict.KmerDict(k, W, last, F, valid)
    if mask:
        assert 0 < len(d) <= n_real and all(valid[e] for _, e in d.kmers())
    else:
        assert len(d) == n_real
    reads = edge_reads(reads + noisy_reads(k, reads), k)
    want = orc.AlignRun(g, capi.config_cli(k), reads).mapping()
    got = kmer_dict.map_reads(d, reads)
    for q in range(len(reads)):
        assert got[q] == want[q], (q, reads[q])
    assert sum(1 for f, _ in got for v in f if v) > 500 or k >= 40


def _primary_oracle_paths(g, reads, k):
    """the wrapper's own mapping (as tests/test_emu_primary.py::test_primary_mapping_is_the_wrappers reads it)"""
    import ctypes as C
    from test_oracle_canonical_wrapper import _L as canon_lib
    lib = canon_lib()
    out = []
    for r in reads:
        nk = max(0, len(r) - k + 1)
        buf = (C.c_uint64 * max(1, nk))()
        if nk:
            lib.orc_canonical_map(g.h, r.encode(), len(r), buf)
        fwd = list(buf)[:nk]
        out.append((fwd, [int(lib.orc_canonical_reverse_complement(g.h, v)) if v else 0 for v in fwd][::-1]))
    return out


@pytest.mark.parametrize("k,mask,seed,order", [(11, False, 1, "input"), (31, False, 3, "colex"), (15, True, 4, "input"),
                                               (12, False, 5, "lex"), (8, True, 6, "input"), (40, False, 7, "lex")])
def test_primary_mapping_equals_the_oracle(k, mask, seed, order):
    from test_emu_primary import primary_world
    g, reads = primary_world(700 + seed, k, mask=mask, order=order)
    W, last, F, valid = g.export()
    d = kmer_dict.KmerDict(k, W, last, F, valid)
    if k % 2 == 0:
        # even k: k-mers that are their own reverse complement, read on both strands
        pal = [s for s, _ in d.kmers() if s == rc(s)]
        reads = reads + pal[:5] + [reads[0][:30] + p + reads[1][:30] for p in pal[:5]]
        assert pal or k > 8, "no palindromic k-mer in this world"
    got = kmer_dict.map_reads(d, reads, kmer_dict.PRIMARY)
    want = _primary_oracle_paths(g, reads, k)
    n = g.n_edges
    for q in range(len(reads)):
        assert got[q] == want[q], (q, reads[q])
    assert any(v > n for f, _ in got for v in f) and any(0 < v <= n for f, _ in got for v in f)
    # ... and the mapping the oracle's aligner itself starts from
    o = orc.AlignRun(g, capi.config_cli(k), reads).mapping()
    assert o == got
