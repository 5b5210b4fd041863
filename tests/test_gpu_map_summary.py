"""`metagraph align --map` on the GPU through the C-ABI (mgx_map_summary_batch -> k_map_summary / k_map_subk): the reference's three
CLI goldens on genome.MT end to end, random worlds against the rules of DeBruijnGraph::map_to_nodes applied in Python to the
oracle's mappings, sub-k windows against the oracle's suffix look-up, the refusals, and host/mgx_align --map."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import orc
from metagraph_amd import aligner, capi
from map_goldens import BASIC_LINES, CANONICAL_LINES, HERE, K, SUBK_LENGTH, SUBK_LINES, read_fastq, triples
from test_oracle_kats import read_fasta
from test_oracle_canonical import CANONICAL
from test_oracle_canonical_wrapper import _L as canon_lib, PRIMARY
from test_oracle_primary_goldens import primary_contigs
from test_emu_vs_oracle import make_world
from test_emu_canonical import canonical_world
from test_emu_primary import primary_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
BASIC = 0
SHORT, LONG, SUBK, NODE_BYTES = 0, 1, 2, 3          # entries of mgx_map_kernel_launch_counts


def counters():
    out = (C.c_uint64 * 4)()
    capi.lib().mgx_map_kernel_launch_counts(out)
    return list(out)


def gpu_graph(g, mode):
    W, last, F, valid = g.export()
    return aligner.Graph(g.k, W, last, F, valid, mode=mode)


def mt_fasta():
    return read_fasta(os.path.join(HERE, "golden", "genome.MT.fa"))


def count_lines(A, reads, map_length=0):
    """--count-kmers in counts mode; asserts that no node array came to the host"""
    before = counters()
    A.map_summary([r[1] for r in reads], map_length)
    after = counters()
    assert after[NODE_BYTES] == before[NODE_BYTES], "counts mode copied a node array to the host"
    assert after[SHORT] > before[SHORT], "k_map_summary (short-read form) did not run"
    assert (after[SUBK] > before[SUBK]) == (0 < map_length < A.graph.k)
    m = A.last_map_summary
    assert not m.node_begin and not m.nodes
    return [A.format_map(m, i, reads[i][0], reads[i][1], capi.MGX_MAP_FMT_COUNT_KMERS, map_length).rstrip("\n") for i in range(len(reads))]


@pytest.mark.parametrize("mask", [False, True])
def test_basic_golden(mask):
    # integration_tests/test_align.py:59-87
    g = orc.Graph.build(K, mt_fasta(), BASIC, mask)
    A = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(K))
    assert count_lines(A, read_fastq()) == BASIC_LINES
    assert count_lines(A, read_fastq(), K) == BASIC_LINES


@pytest.mark.parametrize("mask", [False, True])
def test_sub_k_golden(mask):
    # integration_tests/test_align.py:89-121: --align-length 10
    g = orc.Graph.build(K, mt_fasta(), BASIC, mask)
    A = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(K))
    assert count_lines(A, read_fastq(), SUBK_LENGTH) == SUBK_LINES


def test_canonical_golden():
    # integration_tests/test_align.py:124-151
    g = orc.Graph.build(K, mt_fasta(), CANONICAL, True)
    A = aligner.Aligner(gpu_graph(g, CANONICAL), capi.config_cli(K))
    assert count_lines(A, read_fastq()) == CANONICAL_LINES


def wrapper_base_paths(g, reads):
    """CanonicalDBG::map_to_nodes on the wrapped PRIMARY graph as base nodes (cli/align.cpp:345-348, canonical_dbg.cpp:148-154)"""
    lib = canon_lib()
    paths = []
    for r in reads:
        n = max(0, len(r) - g.k + 1)
        out = (C.c_uint64 * max(1, n))()
        if n:
            lib.orc_canonical_map(g.h, r.encode(), len(r), out)
        paths.append([v - g.n_edges if v > g.n_edges else v for v in list(out)[:n]])
    return paths


def summarise(paths):
    return [(sum(1 for v in p if v), len(p), len({v for v in p if v})) for p in paths]


def test_primary_golden():
    """the wrapped PRIMARY graph finds what the CANONICAL graph finds (discovered / k-mers of the canonical golden); the distinct
    count is over base nodes, checked against the oracle's wrapper path"""
    contigs, _ = primary_contigs(mt_fasta(), K, "lex")
    g = orc.Graph.build(K, contigs, PRIMARY, True)
    reads = read_fastq()
    A = aligner.Aligner(gpu_graph(g, PRIMARY), capi.config_cli(K))
    lines = count_lines(A, reads)
    assert [l.rsplit("/", 1)[0] for l in lines] == [l.rsplit("/", 1)[0] for l in CANONICAL_LINES]
    assert triples(lines) == summarise(wrapper_base_paths(g, [r[1] for r in reads]))


def awkward_reads(reads, k, seed):
    """the world's reads plus: runs of N, lower case, reads shorter than k (one empty), one read of more than 4096 bp"""
    rng = random.Random(seed)
    out = list(reads)
    out.append(reads[0][:20] + "NNNNN" + reads[0][25:])
    out.append(reads[1].lower())
    out.append(reads[2][:k - 1])
    out.append("")
    out.append(reads[3][:k])
    out.append("N" * (k + 3))
    long_read = ""
    while len(long_read) <= 4096 + 300:
        long_read += rng.choice(reads)                 # repeats of whole reads: many repeated nodes
    out.append(long_read)
    out.append(reads[4][:150])
    return out


def check_world(g, mode, reads, want_paths):
    A = aligner.Aligner(gpu_graph(g, mode), capi.config_cli(g.k))
    before = counters()
    counts = A.map_summary(reads)
    mid = counters()
    assert mid[SHORT] > before[SHORT] and mid[LONG] > before[LONG], "both forms of k_map_summary must have run"
    assert mid[NODE_BYTES] == before[NODE_BYTES] and mid[SUBK] == before[SUBK]
    counts2, nodes = A.map_summary(reads, want_nodes=True)
    after = counters()
    assert after[NODE_BYTES] == mid[NODE_BYTES] + 8 * sum(len(p) for p in want_paths)
    want = summarise(want_paths)
    for i in range(len(reads)):
        assert nodes[i] == want_paths[i], (i, reads[i][:60])
        assert counts[i] == want[i] and counts2[i] == want[i], (i, counts[i], want[i])
    assert any(c[0] != c[2] for c in want), "the world holds no read with a repeated node"
    assert any(0 < c[0] < c[1] for c in want)
    # the automatic choice maps these small batches with the one-step-per-lane kernel; the pipe gives the same
    A.set_pipeline("map_pipe=2")
    assert A.map_summary(reads) == want


@pytest.mark.parametrize("k,mask,seed", [(11, False, 1), (21, True, 2), (31, False, 3), (15, True, 4), (40, False, 5)])
def test_basic_worlds(k, mask, seed):
    g, reads = make_world(900 + seed, k, n_reads=60, read_len=150, mask=mask)
    reads = awkward_reads(reads, k, seed)
    # DBGSuccinct::map_to_nodes, BASIC: the forward mapping with the mask applied
    want = [list(fwd) for fwd, _ in orc.AlignRun(g, capi.config_cli(k), reads).mapping()]
    check_world(g, BASIC, reads, want)


@pytest.mark.parametrize("k,seed", [(11, 1), (21, 2), (31, 3), (12, 4)])
def test_canonical_worlds(k, seed):
    g, reads = canonical_world(920 + seed, k, n_reads=60, read_len=150)
    reads = awkward_reads(reads, k, seed)
    # dbg_succinct.cpp:436-482: the smaller of the k-mer's and its reverse complement's index, 0 if one is missing
    want = [[min(a, b) if a and b else 0 for a, b in zip(fwd, rev[::-1])] for fwd, rev in orc.AlignRun(g, capi.config_cli(k), reads).mapping()]
    check_world(g, CANONICAL, reads, want)


@pytest.mark.parametrize("k,mask,seed,order", [(11, False, 1, "input"), (31, False, 3, "colex"), (15, True, 4, "input"), (12, False, 5, "lex")])
def test_primary_worlds(k, mask, seed, order):
    g, reads = primary_world(940 + seed, k, mask=mask, order=order, n_reads=60, read_len=150)
    reads = awkward_reads(reads, k, seed)
    check_world(g, PRIMARY, reads, wrapper_base_paths(g, reads))


def prefix_table_length(n_edges, k, cap=14):
    """choose_prefix_len of csrc/graph_build.hpp, restated"""
    m = 2
    while m < cap and (1 << (2 * (m - 1))) < n_edges:
        m += 1
    return min(m, k - 1)


@pytest.mark.parametrize("k,mask,seed,mode", [(11, False, 1, BASIC), (21, True, 2, BASIC), (31, False, 3, BASIC), (15, True, 4, BASIC),
                                              (21, False, 6, CANONICAL)])
def test_sub_k_worlds(k, mask, seed, mode):
    if mode == CANONICAL:
        g, reads = canonical_world(960 + seed, k, n_reads=30, read_len=150)
    else:
        g, reads = make_world(960 + seed, k, n_reads=30, read_len=150, mask=mask)
    reads = awkward_reads(reads, k, seed)
    A = aligner.Aligner(gpu_graph(g, mode), capi.config_cli(k))
    m = prefix_table_length(g.n_edges, k)
    lengths = sorted({L for L in (k - 1, (k + 1) // 2, m - 1, m + 1) if 1 <= L < k})
    assert len(lengths) >= 3
    for L in lengths:
        want_paths = []
        for r in reads:
            path = []
            for i in range(len(r) - L + 1):
                hits, _ = g.suffix_match(r[i:i + L], L)
                path.append(hits[0] if hits else 0)
            want_paths.append(path)
        before = counters()
        counts, nodes = A.map_summary(reads, L, want_nodes=True)
        after = counters()
        assert after[SUBK] == before[SUBK] + 1 and after[SHORT] > before[SHORT] and after[LONG] > before[LONG]
        want = summarise(want_paths)
        for i in range(len(reads)):
            assert nodes[i] == want_paths[i], (L, i, reads[i][:60])
            assert counts[i] == want[i], (L, i)
        assert A.map_summary(reads, L) == want
        assert any(c[0] for c in want)


def test_refusals():
    contigs, _ = primary_contigs(mt_fasta(), K, "lex")
    g = orc.Graph.build(K, contigs, PRIMARY, True)
    A = aligner.Aligner(gpu_graph(g, PRIMARY), capi.config_cli(K))
    with pytest.raises(aligner.MgxError) as e:
        A.map_summary(["ACGTACGTACGTACGT"], K - 1)
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED
    with pytest.raises(aligner.MgxError) as e:
        A.map_summary(["ACGTACGTACGTACGT"], K + 1)
    assert e.value.code == capi.MGX_ERR_INVALID
    gb = orc.Graph.build(K, mt_fasta(), BASIC, False)
    with pytest.raises(aligner.MgxError) as e:
        aligner.Aligner(gpu_graph(gb, BASIC), capi.config_cli(K)).map_summary(["ACGTACGTACGTACGT"], K + 1)
    assert e.value.code == capi.MGX_ERR_INVALID
    assert A.map_summary(["ACGTACGTACGTACGT"], K) == A.map_summary(["ACGTACGTACGTACGT"])


def boss_dump(g, path):
    W, last, F, _ = g.export()
    with open(path, "wb") as f:
        f.write(struct.pack("<7Q", g.k, g.n_edges, *[int(x) for x in F]))
        f.write(W.tobytes())
        f.write(last.tobytes())


def test_mgx_align_map_driver(tmp_path):
    exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
    reads = os.path.join(HERE, "golden", "genome_MT1.fq")
    dump = str(tmp_path / "mt.boss")
    boss_dump(orc.Graph.build(K, mt_fasta(), BASIC, False), dump)
    cdump = str(tmp_path / "mt.canonical.boss")
    boss_dump(orc.Graph.build(K, mt_fasta(), CANONICAL, False), cdump)

    def run(*args):
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout

    assert run(dump, reads, "--map", "--count-kmers") == "".join(l + "\n" for l in BASIC_LINES)
    assert run(dump, reads, "--map", "--count-kmers", "--align-length", "10") == "".join(l + "\n" for l in SUBK_LINES)
    assert run(cdump, reads, "--canonical", "--map", "--count-kmers") == "".join(l + "\n" for l in CANONICAL_LINES)
    # --query-presence --discovery-fraction 0.5: DeBruijnGraph::find on the golden triples (140 k-mers: at most 70 may be missing)
    assert run(dump, reads, "--map", "--query-presence", "--discovery-fraction", "0.5") == "0\n1\n1\n0\n1\n0\n0\n"
    assert run(cdump, reads, "--canonical", "--map", "--query-presence", "--discovery-fraction", "0.5") == "1\n1\n1\n1\n1\n0\n1\n"
    recs = read_fastq()
    want = "".join(">%s\n%s\n" % recs[i] for i in (1, 2, 4))
    assert run(dump, reads, "--map", "--query-presence", "--filter-present", "--discovery-fraction", "0.5") == want
    # --align-length above k: a warning, then k (cli/align.cpp:351-355)
    assert run(dump, reads, "--map", "--count-kmers", "--align-length", "12") == "".join(l + "\n" for l in BASIC_LINES)
    # --fwd-and-reverse: every record is followed by its reverse complement under the same name
    out = run(cdump, reads, "--canonical", "--map", "--count-kmers", "--fwd-and-reverse").split("\n")[:-1]
    assert len(out) == 14 and out[0::2] == CANONICAL_LINES and out[1::2] == CANONICAL_LINES
    # the k-mer: node form
    out = run(dump, reads, "--map").split("\n")[:-1]
    assert len(out) == 7 * 140 and out[0].split(": ")[0] == recs[0][1][:K]
    assert sum(1 for l in out[:140] if l.split(": ")[1] != "0") == 1
