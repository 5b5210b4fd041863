"""mgx_format_json_batch (the `align --json` text of a range of a batch written by HIP kernels: csrc/json_format.hpp,
csrc/mgx_jsonfmt.hip) against the existing host formatter: every test aligns a batch, fetches it through mgx_fetch_results,
formats every query with mgx_format_json and compares those lines byte for byte with the batch text; line_begin is compared with
the running sum of the host lines' lengths.  Outside the capacity test the hook's host-formatted count must not move: no test
passes on host-formatted lines.  Needs a real MI355X."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import orc
from metagraph_amd import aligner, capi
from test_emu_vs_oracle import make_world, rand_seq, KATS
from test_oracle_canonical import CANONICAL
from test_oracle_primary_goldens import PRIMARY
from test_gpu_format_batch import gpu_graph, align_host, format_world, WORLD_SEEDS, _bytes, BASIC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def host_lines(res, headers, reads, k):
    """the yardstick: mgx_format_json, query by query, on the fetched results"""
    return [capi.format_json(res, i, _bytes(h), _bytes(q), k).encode("latin-1") for i, (h, q) in enumerate(zip(headers, reads))]


def check_batch(A, headers, reads, k):
    """after a batch on A: the batch text equals the host lines of the fetched results, formatted by kernels alone -> the lines"""
    res = A.fetch()
    lines = host_lines(res, headers, reads, k)
    before = aligner.format_json_kernel_launch_counts()
    text, lb = A.format_json_batch(headers)
    after = aligner.format_json_kernel_launch_counts()
    assert after[2] == before[2], "lines were formatted on the host"
    assert len(lb) == len(reads) + 1
    running = 0
    for i, ln in enumerate(lines):
        assert int(lb[i]) == running, "line_begin[%d]" % i
        assert text[running:running + len(ln)] == ln, "query %d: %r != %r" % (i, text[running:running + len(ln)], ln)
        running += len(ln)
    assert int(lb[-1]) == running == len(text)
    assert text == b"".join(lines)
    return lines


def roomy_limits(A):
    """four times the limits A's last batch ran with: a few reads of the random worlds outgrow the derived per-read arenas with
    four alternative paths, and their lines would come from the host formatter (the capacity test's subject, nobody else's)"""
    lim = capi.Limits()
    assert capi.lib().mgx_aligner_get_limits(A.h, C.byref(lim)) == 0
    lim.max_columns *= 4
    lim.max_seeds = min(65535, lim.max_seeds * 4)
    lim.cell_arena_bytes *= 4
    return lim


def golden_graph():
    from test_oracle_kats import read_fasta, read_fastq
    cli = KATS["cli"]
    g = orc.Graph.build(cli["k"], read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])), 0, False)
    return cli, g, read_fastq(os.path.join(HERE, "golden", cli["reads_fastq"]))


def golden_text(name):
    return b"".join(line for line in open(os.path.join(HERE, "golden", name), "rb") if line.strip())


# ---- 1. the reference's goldens ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit_distance,name", [(False, "genome_MT1.align.json"), (True, "genome_MT1.align.edit.json")])
def test_reference_goldens_batch_text(edit_distance, name, kernels):
    from test_oracle_kats import json_golden_config
    cli, g, reads = golden_graph()
    A = aligner.Aligner(gpu_graph(g), json_golden_config(cli["k"], edit_distance))
    headers = [r[0].lstrip("@").split()[0] for r in reads]
    align_host(A, [r[1] for r in reads])
    check_batch(A, headers, [r[1] for r in reads], cli["k"])
    # the golden files hold the lines of the FASTQ's first five reads (as test_oracle_kats.py reads them): that range of the batch
    want = golden_text(name)
    n_gold = want.count(b"\n")
    before = aligner.format_json_kernel_launch_counts()
    assert n_gold == 5 and A.format_json_batch(headers[:n_gold], first=0)[0] == want
    assert aligner.format_json_kernel_launch_counts()[2] == before[2], "lines were formatted on the host"


# ---- 2. random worlds ----------------------------------------------------------------------------------------------------
INSERTION = re.compile(rb'\{"sequence":"[^"]*","to_length":\d+\}')       # an edit with "sequence" and no from_length
DELETION = re.compile(rb'\{"from_length":\d+\}')                          # an edit with from_length and no to_length


def json_world(mode):
    """format_world's reads cut to ~100 (the built ones — indels, junk tails, two places, nowhere, empty — are its last eleven), and
    two reads with junk in FRONT of a stretch of the genome: a leading clip on the forward strand in every mode"""
    g, reads = format_world(mode)
    seed = WORLD_SEEDS[mode]
    genome = rand_seq(random.Random(seed), 6000)                # (the builders draw the genome first)
    rng = random.Random(seed + 2)
    return g, reads[:88] + reads[-11:] + [rand_seq(rng, 14) + genome[p:p + 130] for p in (900, 3100)]


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reads", "device_reads"])
@pytest.mark.parametrize("num_alt", [1, 4])
@pytest.mark.parametrize("mode", ["basic", "canonical", "primary"])
def test_random_worlds_batch_text(mode, num_alt, on_device, kernels):
    g, reads = json_world(mode)
    cfg = capi.config_cli(21)
    cfg.num_alternative_paths = num_alt
    G = gpu_graph(g, {"basic": BASIC, "canonical": CANONICAL, "primary": PRIMARY}[mode])
    A = aligner.Aligner(G, cfg)
    align_host(A, reads)
    A = aligner.Aligner(G, cfg, roomy_limits(A))
    headers = ["read.%d/%s" % (i, mode) for i in range(len(reads))]
    if on_device:
        import torch
        blob, offs = aligner.pack_queries(reads)
        d_seqs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        A.align_device(d_seqs.data_ptr(), d_offs.data_ptr(), len(reads))
    else:
        align_host(A, reads)
    text = b"".join(check_batch(A, headers, reads, 21))
    assert b',"sequence":""}\n' in text                                      # a no-alignment line
    assert b'"soft_clipped":true' in text
    assert INSERTION.search(text) and DELETION.search(text)
    if mode == "basic":              # (on CANONICAL and PRIMARY graphs the oracle reports every alignment of these worlds as '+')
        assert b'"read_on_reverse_strand":true' in text
    if num_alt > 1:
        assert b'"is_secondary":true' in text


# ---- 3. edge queries and headers -------------------------------------------------------------------------------------------
def test_edge_queries_and_headers(kernels):
    k = 21
    g, reads = make_world(9200, k, genome_len=4000, n_reads=30, read_len=150)
    edge = [reads[0].lower(), reads[1][:60].lower() + reads[1][60:], reads[2][:40] + "N" * 30 + reads[2][70:], "N" * 90, "n" * 25,
            _bytes(reads[3][:70]) + b"\x80\xff\xc3\xa9" + _bytes(reads[3][74:]), b"\x80" * 40, b"\xfe", "", reads[4][:k - 1], reads[5][:3],
            "acgtnACGTN" * 9, reads[6][:k], "R" + reads[7][1:], reads[8].lower()[:80] + "~{|}" + reads[8][84:],
            _bytes(reads[9][:50]) + b"\"\\\x01\t" + _bytes(reads[9][54:])]
    reads = [_bytes(r) for r in edge + reads[10:]]
    rng = random.Random(77)
    headers = []
    for i in range(len(reads)):
        if i % 5 == 0:
            headers.append(b"")
        elif i % 5 == 1:
            headers.append(bytes(33 + rng.randrange(94) for _ in range(1000)))
        elif i % 5 == 2:
            headers.append(b"q\"uote\\back\ttab\x01ctl\x7fdel\xe9high\n%d" % i)
        else:
            headers.append(b"r%d some words:%d" % (i, i * i))
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, reads)
    lines = check_batch(A, headers, reads, k)
    text = b"".join(lines)
    assert b"\\u007F" in text and b'\\"' in text and b"\\u00E9" in text and b"\\\\" in text and b"\\u0001" in text
    assert lines[8] == b'{"name":"r8 some words:64","sequence":""}\n'         # the empty query
    assert any(len(ln) > 1000 for ln in lines)


# ---- 4. one long read -----------------------------------------------------------------------------------------------------
def test_one_long_read_many_nodes_many_runs():
    k = 21
    g, _ = make_world(9600, k, genome_len=3000, n_reads=4, read_len=100)
    genome = rand_seq(random.Random(9600), 3000)                # (the builder draws the genome first)
    read = list(genome[500:1200])
    for p in range(30, 700, 40):
        read[p] = "ACGT"[("ACGT".index(read[p]) + 1) % 4]
    read = "".join(read)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, [read, read[:150]])
    res = A.fetch()
    a = res.alignments[res.aln_begin[0]]
    assert a.n_nodes > 64 and a.n_cigar > 16
    check_batch(A, ["long", "short"], [read, read[:150]], k)


# ---- 5. a circular path ----------------------------------------------------------------------------------------------------
def test_circular_path():
    """a graph of one repeated unit of p > k characters is a cycle of p nodes; a read of k + p characters walks p + 1 nodes, the
    first again at the end (checked with the oracle on the CPU: seed 9502 aligns as 51= over 31 nodes, nodes[0] == nodes[30])"""
    k, p = 21, 30
    unit = rand_seq(random.Random(9502), p)
    g = orc.Graph.build(k, [unit * 6], 0, False)
    read = (unit * 3)[:k + p]
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, [read])
    res = A.fetch()
    a = res.alignments[res.aln_begin[0]]
    assert a.n_nodes == p + 1 and res.nodes[a.nodes_begin] == res.nodes[a.nodes_begin + a.n_nodes - 1]
    lines = check_batch(A, ["circle"], [read], k)
    assert b'"path":{"is_circular":true,"length":31,' in lines[0]


# ---- 6. ranges ------------------------------------------------------------------------------------------------------------
def test_ranges_concatenate_to_the_whole_text():
    k = 21
    g, reads = make_world(9700, k, genome_len=4000, n_reads=60, read_len=150)
    reads = reads + ["", rand_seq(random.Random(1), 100)]
    n = len(reads)
    headers = ["range%d" % i for i in range(n)]
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, reads)
    lines = check_batch(A, headers, reads, k)
    whole = b"".join(lines)
    before = aligner.format_json_kernel_launch_counts()
    pieces = []
    for first, m in ((0, 0), (0, 1), (1, 17), (18, 0), (18, n - 19), (n - 1, 1), (n, 0)):
        text, lb = A.format_json_batch(headers[first:first + m], first=first)
        assert len(lb) == m + 1 and text == b"".join(lines[first:first + m])
        assert [int(x) for x in lb] == [0] + [int(x) for x in np.cumsum([len(ln) for ln in lines[first:first + m]])]
        pieces.append(text)
    assert b"".join(pieces) == whole
    assert aligner.format_json_kernel_launch_counts()[2] == before[2]
    for first, m in ((n, 1), (n - 1, 2), (n + 1, 0)):
        with pytest.raises(aligner.MgxError) as e:
            A.format_json_batch(["h"] * m, first=first)
        assert e.value.code == capi.MGX_ERR_INVALID and "beyond" in str(e.value)


# ---- 7. label-aware aligner -----------------------------------------------------------------------------------------------
def test_labeled_aligner_prints_no_labels():
    from labeled_worlds import labeled_world
    g, anno, reads = labeled_world(21, 15, n_strains=3, n_reads=40)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(15),
                        annotation=aligner.Annotation(g.n_edges, [anno.column_words(j) for j in range(anno.n_labels)]))
    align_host(A, reads)
    lines = check_batch(A, ["q%d" % i for i in range(len(reads))], reads, 15)
    assert sum(ln.count(b"\n") for ln in lines) > len(reads)                  # (some query has one alignment per label set)


# ---- 8. capacity retry ----------------------------------------------------------------------------------------------------
def test_capacity_statuses_are_retried_and_spliced():
    g, reads = make_world(4242, 21, genome_len=6000, n_reads=200, read_len=150)
    cfg = capi.config_cli(21)
    G = gpu_graph(g)
    headers = ["cap%d" % i for i in range(len(reads))]
    D = aligner.Aligner(G, cfg)                                                # the yardstick: an aligner with default limits
    align_host(D, reads)
    res = D.fetch()
    assert all(res.status[i] == 0 for i in range(len(reads)))
    want = host_lines(res, headers, reads, 21)
    assert D.format_json_batch(headers)[0] == b"".join(want)
    lim = capi.Limits()
    lim.cell_arena_bytes = 1600
    A = aligner.Aligner(G, cfg, lim)
    align_host(A, reads)
    before = aligner.format_json_kernel_launch_counts()
    text, lb = A.format_json_batch(headers)
    after = aligner.format_json_kernel_launch_counts()
    assert text == b"".join(want)
    assert [int(x) for x in lb] == [0] + [int(x) for x in np.cumsum([len(w) for w in want])]
    retried = A.stats()["n_capacity_retried"]
    assert after[2] - before[2] == retried and retried > 0
    B = aligner.Aligner(G, cfg, lim)
    B.set_pipeline("retry_capacity=0")
    align_host(B, reads)
    with pytest.raises(aligner.MgxError) as e:
        B.format_json_batch(headers)
    assert e.value.code == capi.MGX_ERR_CAPACITY and "query" in str(e.value)


# ---- 8b. TSV, JSON and map texts in turn: one host pipeline, one set of buffers per handle ----------------------------------
def test_three_forms_in_turn_on_shared_buffers():
    """the three batch formatters run the same host sequence on the handle's tf_* buffers, scan space, pinned text and line_begin:
    TSV, JSON, a JSON range and TSV again on one handle (some queries take the capacity retry), `align --map` texts on a second
    handle of the same graph before and after another TSV call on the first.  Every text and line_begin equals the per-query host
    formatters' on a default-limits aligner.  (On the CPU, emu_drv.EmuRun in its 8-lane build, the group width these batches
    run with, aligns all reads of seed 9802 with status 0 under default limits, and leaves reads 6 and 22 a capacity status
    with a 1600-byte cell arena: one inside the range 5 .. 12, one outside.)"""
    from test_gpu_format_batch import host_lines as tsv_host_lines
    from test_gpu_map_format_batch import COUNT, NODES, check_device_texts, host_texts
    k = 21
    g, reads = make_world(9802, k, genome_len=3000, n_reads=24, read_len=120)
    cfg = capi.config_cli(k)
    G = gpu_graph(g)
    headers = ["turn%d" % i for i in range(len(reads))]
    D = aligner.Aligner(G, cfg)                                                # the yardstick: an aligner with default limits
    align_host(D, reads)
    res = D.fetch()
    assert all(res.status[i] == 0 for i in range(len(reads)))
    want_tsv = tsv_host_lines(D, res, headers, reads)
    want_json = host_lines(res, headers, reads, k)

    def same(got, want):
        text, lb = got
        assert text == b"".join(want)
        assert [int(x) for x in lb] == [0] + [int(x) for x in np.cumsum([len(w) for w in want])]
        return text

    lim = capi.Limits()
    lim.cell_arena_bytes = 1600
    A = aligner.Aligner(G, cfg, lim)
    align_host(A, reads)
    tsv = same(A.format_tsv_batch(headers), want_tsv)
    assert A.stats()["n_capacity_retried"] > 0
    same(A.format_json_batch(headers), want_json)
    assert A.stats()["n_capacity_retried"] > 0
    same(A.format_json_batch(headers[5:12], first=5, n=7), want_json[5:12])
    assert same(A.format_tsv_batch(headers), want_tsv) == tsv
    M = aligner.Aligner(G, cfg)                                                # a second handle: the same pool of device blocks
    want_map = host_texts(M, headers, reads, 0, [(NODES, 0.7), (COUNT, 0.7)])
    for _ in range(2):
        M.map_summary(reads, keep_nodes=True)
        check_device_texts(M, headers, want_map)
        assert same(A.format_tsv_batch(headers), want_tsv) == tsv


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    g, reads = make_world(9300, 21, genome_len=3000, n_reads=20, read_len=120)
    G = gpu_graph(g)
    cfg = capi.config_cli(21)
    cfg.post_chain_alignments = 1
    A = aligner.Aligner(G, cfg)
    align_host(A, reads)
    with pytest.raises(aligner.MgxError) as e:
        A.format_json_batch(["h"] * len(reads))
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED and "post_chain_alignments" in str(e.value)
    B = aligner.Aligner(G, capi.config_cli(21))
    with pytest.raises(aligner.MgxError) as e:                                # never run
        B.format_json_batch(["h"])
    assert e.value.code == capi.MGX_ERR_INVALID
    for between in (lambda: B.map_batch(reads), lambda: B.map_summary(reads)):
        align_host(B, reads)
        assert len(B.format_json_batch(["h"] * len(reads))[0]) > 0
        between()
        with pytest.raises(aligner.MgxError) as e:
            B.format_json_batch(["h"] * len(reads))
        assert e.value.code == capi.MGX_ERR_INVALID and "staged" in str(e.value)


# ---- 10. the hook: kernels ran, the records did not travel -------------------------------------------------------------------
def test_kernels_run_and_only_the_text_travels():
    g, reads = make_world(9400, 21, genome_len=5000, n_reads=120, read_len=150)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, reads)
    headers = ["t%d" % i for i in range(len(reads))]
    before = aligner.format_json_kernel_launch_counts()
    text, lb = A.format_json_batch(headers)
    after = aligner.format_json_kernel_launch_counts()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[2] == before[2]
    n = len(reads)
    assert after[3] - before[3] == len(text) + 8 * (n + 1) + 16
    check_batch(A, headers, reads, 21)


# ---- 11. the driver ---------------------------------------------------------------------------------------------------------
def test_driver_json(tmp_path):
    cli, g, _ = golden_graph()
    W, last, F, _ = g.export()
    dump = tmp_path / "mt.boss"
    with open(dump, "wb") as f:
        f.write(struct.pack("<7Q", g.k, g.n_edges, *[int(x) for x in F]))
        f.write(W.tobytes())
        f.write(last.tobytes())
    exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
    reads = os.path.join(HERE, "golden", cli["reads_fastq"])
    # the golden file holds the lines of the FASTQ's first five reads: those reads as a file of their own, then the whole file
    want = golden_text("genome_MT1.align.json")
    first5 = tmp_path / "first5.fq"
    with open(reads, "rb") as f:
        first5.write_bytes(b"".join(f.readlines()[:4 * want.count(b"\n")]))
    whole = subprocess.run([exe, str(dump), reads, "--align-min-exact-match", "0.0", "--json"], capture_output=True, timeout=120)
    assert whole.returncode == 0 and whole.stdout.startswith(want) and whole.stdout.count(b"\n") > want.count(b"\n"), whole.stderr
    device_forms = (["--format-on-device"], ["--format-on-device", "--parse-on-device"], ["--format-on-device", "--json-slice-bytes", "30000"],
                    ["--format-on-device", "--parse-on-device", "--json-slice-bytes", "1"])
    for fastq, want, forms in ((str(first5), want, ([],) + device_forms), (reads, whole.stdout, device_forms)):
        base = [exe, str(dump), fastq, "--align-min-exact-match", "0.0", "--json"]
        for extra in forms:
            r = subprocess.run(base + extra, capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr
            assert r.stdout == want, extra
    r = subprocess.run(base + ["--map"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"--json" in r.stderr and r.stdout == b""
