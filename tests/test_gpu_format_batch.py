"""mgx_format_tsv_batch (the TSV text of a whole batch written by HIP kernels: csrc/tsv_format.hpp, csrc/mgx_format.hip)
against the existing host formatter: every test aligns a batch, fetches it through mgx_fetch_results, formats every query with
mgx_format_tsv_labeled and compares those lines byte for byte with the batch text; line_begin is compared with the running sum
of the host lines' lengths.  Needs a real MI355X."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import orc
from metagraph_amd import aligner, capi
from test_emu_vs_oracle import make_world, rand_seq, rc, KATS
from test_emu_canonical import canonical_world
from test_emu_primary import primary_world
from test_oracle_canonical import CANONICAL
from test_oracle_primary_goldens import PRIMARY

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASIC = 0


def gpu_graph(g, mode=BASIC):
    W, last, F, valid = g.export()
    return aligner.Graph(g.k, W, last, F, valid, mode=mode)


def _bytes(x):
    return x if isinstance(x, bytes) else x.encode("latin-1")


def host_lines(A, res, headers, reads, names=None):
    """the yardstick: mgx_format_tsv_labeled, query by query, on the fetched results"""
    L = capi.lib()
    mps = A.get_config().min_path_score
    nm = [_bytes(n) for n in (names or [])]
    arr = (C.c_char_p * len(nm))(*nm) if nm else None
    out = []
    for i, (h, q) in enumerate(zip(headers, reads)):
        h, q = _bytes(h), _bytes(q)
        need = L.mgx_format_tsv_labeled(C.byref(res), i, h, q, len(q), mps, arr, len(nm), None, 0)
        buf = C.create_string_buffer(need + 1)
        L.mgx_format_tsv_labeled(C.byref(res), i, h, q, len(q), mps, arr, len(nm), buf, need + 1)
        out.append(buf.raw[:need])
    return out


def check_batch(A, headers, reads, names=None):
    """after a batch on A: the batch text equals the host lines of the fetched results -> the lines"""
    res = A.fetch()
    lines = host_lines(A, res, headers, reads, names)
    text, lb = A.format_tsv_batch(headers, names)
    assert len(lb) == len(reads) + 1
    running = 0
    for i, ln in enumerate(lines):
        assert int(lb[i]) == running, "line_begin[%d]" % i
        assert text[running:running + len(ln)] == ln, "query %d: %r != %r" % (i, text[running:running + len(ln)], ln)
        running += len(ln)
    assert int(lb[-1]) == running == len(text)
    assert text == b"".join(lines)
    return lines


def align_host(A, reads):
    blob, offs = aligner.pack_queries(reads)
    C_ = capi.lib()
    assert C_.mgx_align_batch_device(A.h, blob, offs.ctypes.data, len(reads), 0) == 0, C_.mgx_last_error()


# ---- 1. the reference's CLI goldens -------------------------------------------------------------------------------------
def test_cli_goldens_batch_text(kernels):
    from test_oracle_kats import read_fasta, read_fastq
    cli = KATS["cli"]
    g = orc.Graph.build(cli["k"], read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])), 0, False)
    G = gpu_graph(g)
    reads = read_fastq(os.path.join(HERE, "golden", cli["reads_fastq"]))
    for spec in cli["runs"]:
        cfg = capi.config_cli(cli["k"])
        for key, val in spec["flags"].items():
            setattr(cfg, key, val)
        A = aligner.Aligner(G, cfg)
        align_host(A, [r[1] for r in reads])
        lines = check_batch(A, [r[0] for r in reads], [r[1] for r in reads])
        text, _ = A.format_tsv_batch([r[0] for r in reads])
        got = text.decode("latin-1").rstrip("\n").split("\n")
        assert len(got) == len(lines)
        for idx, want in spec["lines"].items():
            assert got[int(idx)] == want
        for idx, fields in spec["fields"].items():
            f = got[int(idx)].split("\t")
            for fi, fv in fields.items():
                assert f[int(fi)] == fv


# ---- 2., 3. random worlds ---------------------------------------------------------------------------------------------
WORLD_SEEDS = {"basic": 9101, "canonical": 9102, "primary": 9103}


def format_world(mode):
    """a random world of the mode plus reads built to print every kind of field: a read with an insertion, a deletion and a
    junk tail (I, D and S runs in one CIGAR), its reverse complement, a read from nowhere.  (Checked against the oracle on
    the CPU before the seeds were fixed: coverage() holds for every mode — the '-' orientation on the BASIC graph only, the
    two-alignment line with num_alternative_paths 4.)"""
    seed, k = WORLD_SEEDS[mode], 21
    build = {"basic": make_world, "canonical": canonical_world, "primary": primary_world}[mode]
    g, reads = build(seed, k, genome_len=6000, n_reads=120, read_len=150, n_variants=20)
    genome = rand_seq(random.Random(seed), 6000)                # (the builders draw the genome first)
    rng = random.Random(seed + 1)
    for p in (300, 1400, 2500, 3600):
        r = genome[p:p + 50] + rc(genome[p + 48:p + 50]) + "A" + genome[p + 50:p + 100] + genome[p + 103:p + 150] + rand_seq(rng, 14)
        reads += [r, rc(r)]
    # two places of the genome share this read: alternative alignments
    reads += [genome[700:775] + genome[4100:4175], rand_seq(rng, 150), ""]
    return g, reads


def coverage(lines):
    """what a batch of lines holds: a "*" line, a '-' orientation, a line with two or more alignments, a CIGAR with I, D and S"""
    star = minus = multi = ids = False
    for ln in lines:
        f = ln.rstrip(b"\n").split(b"\t")
        if f[2] == b"*":
            star = True
            continue
        n_aln = sum(1 for x in f[2:] if x in (b"+", b"-"))
        multi |= n_aln >= 2
        minus |= b"-" in f[2:]
        for j in range(2, len(f)):
            if f[j] in (b"+", b"-") and j + 4 < len(f):
                cg = f[j + 4]
                ids |= b"I" in cg and b"D" in cg and b"S" in cg
    return {"star": star, "minus": minus, "multi": multi, "ids": ids}


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reads", "device_reads"])
@pytest.mark.parametrize("num_alt", [1, 4])
@pytest.mark.parametrize("mode", ["basic", "canonical", "primary"])
def test_random_worlds_batch_text(mode, num_alt, on_device, kernels):
    g, reads = format_world(mode)
    cfg = capi.config_cli(21)
    cfg.num_alternative_paths = num_alt
    A = aligner.Aligner(gpu_graph(g, {"basic": BASIC, "canonical": CANONICAL, "primary": PRIMARY}[mode]), cfg)
    headers = ["read.%d/%s" % (i, mode) for i in range(len(reads))]
    if on_device:
        import torch
        blob, offs = aligner.pack_queries(reads)
        d_seqs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        A.align_device(d_seqs.data_ptr(), d_offs.data_ptr(), len(reads))
    else:
        align_host(A, reads)
    lines = check_batch(A, headers, reads)
    cov = coverage(lines)
    assert cov["star"] and cov["ids"], cov
    if mode == "basic":              # (on CANONICAL and PRIMARY graphs the oracle reports every alignment of these worlds as '+')
        assert cov["minus"], cov
    if num_alt > 1:
        assert cov["multi"], cov


# ---- 4. edge queries -----------------------------------------------------------------------------------------------------
def test_edge_queries_and_headers(kernels):
    k = 21
    g, reads = make_world(9200, k, genome_len=4000, n_reads=30, read_len=150)
    edge = [reads[0].lower(), reads[1][:60].lower() + reads[1][60:], reads[2][:40] + "N" * 30 + reads[2][70:], "N" * 90, "n" * 25,
            _bytes(reads[3][:70]) + b"\x80\xff\xc3\xa9" + _bytes(reads[3][74:]), b"\x80" * 40, b"\xfe", "", reads[4][:k - 1], reads[5][:3],
            "acgtnACGTN" * 9, reads[6][:k], "R" + reads[7][1:], reads[8].lower()[:80] + "~{|}" + reads[8][84:]]
    reads = [_bytes(r) for r in edge + reads[9:]]
    rng = random.Random(77)
    headers = []
    for i in range(len(reads)):
        if i % 4 == 0:
            headers.append(b"")
        elif i % 4 == 1:
            headers.append(bytes(33 + rng.randrange(94) for _ in range(1000)))
        else:
            headers.append(b"r%d some words:%d" % (i, i * i))
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(k))
    align_host(A, reads)
    lines = check_batch(A, headers, reads)
    assert lines[0].split(b"\t")[1] == _bytes(edge[0]).upper()                 # lower case is printed upper case ...
    assert lines[6].split(b"\t")[1] == b"\x7f" * 40                             # ... bytes >= 0x80 as 127
    assert lines[8].startswith(headers[8] + b"\t\t*\t*\t")                      # the empty query
    assert any(len(ln) > 1000 for ln in lines)


# ---- 5. label-aware ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", ["all", "fewer", "none"])
def test_labeled_batch_text(names):
    from labeled_worlds import labeled_world
    g, anno, reads = labeled_world(21, 15, n_strains=3, n_reads=40)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(15),
                        annotation=aligner.Annotation(g.n_edges, [anno.column_words(j) for j in range(anno.n_labels)]))
    all_names = ["strain%d" % j if j % 2 else "a/longer name for label %d" % j for j in range(anno.n_labels)]
    label_names = {"all": all_names, "fewer": all_names[:2], "none": None}[names]
    align_host(A, reads)
    lines = check_batch(A, ["q%d" % i for i in range(len(reads))], reads, label_names)
    text = b"".join(lines)
    assert b";" in text                                      # some alignment has several labels
    if names == "all":
        assert b"strain1" in text
    if names == "fewer":                                     # names and numbers side by side
        tokens = set()
        for ln in lines:
            f = ln.rstrip(b"\n").split(b"\t")
            for j in range(2, len(f)):
                if f[j] in (b"+", b"-") and j + 6 < len(f) and f[j + 6] not in (b"+", b"-"):
                    tokens.update(f[j + 6].split(b";"))
        assert b"strain1" in tokens and any(t.isdigit() for t in tokens), tokens


# ---- 6. capacity retry ---------------------------------------------------------------------------------------------------
def test_capacity_statuses_are_retried_and_spliced():
    g, reads = make_world(4242, 21, genome_len=6000, n_reads=200, read_len=150)
    cfg = capi.config_cli(21)
    G = gpu_graph(g)
    headers = ["cap%d" % i for i in range(len(reads))]
    # the yardstick: host lines of an aligner with default limits
    D = aligner.Aligner(G, cfg)
    align_host(D, reads)
    res = D.fetch()
    assert all(res.status[i] == 0 for i in range(len(reads)))
    want = host_lines(D, res, headers, reads)
    lim = capi.Limits()
    lim.cell_arena_bytes = 1600
    A = aligner.Aligner(G, cfg, lim)
    align_host(A, reads)
    before = aligner.format_kernel_launch_counts()
    text, lb = A.format_tsv_batch(headers)
    after = aligner.format_kernel_launch_counts()
    assert text == b"".join(want)
    assert [int(x) for x in lb] == [0] + list(np.cumsum([len(w) for w in want]))
    retried = A.stats()["n_capacity_retried"]
    assert after[2] - before[2] == retried and retried > 0
    # statuses handed to the caller: no text without those lines
    B = aligner.Aligner(G, cfg, lim)
    B.set_pipeline("retry_capacity=0")
    align_host(B, reads)
    with pytest.raises(aligner.MgxError) as e:
        B.format_tsv_batch(headers)
    assert e.value.code == capi.MGX_ERR_CAPACITY and "query" in str(e.value)


# ---- 7. post_chain_alignments --------------------------------------------------------------------------------------------
def test_post_chain_alignments_is_refused():
    g, reads = make_world(9300, 21, genome_len=3000, n_reads=20, read_len=120)
    cfg = capi.config_cli(21)
    cfg.post_chain_alignments = 1
    A = aligner.Aligner(gpu_graph(g), cfg)
    align_host(A, reads)
    with pytest.raises(aligner.MgxError) as e:
        A.format_tsv_batch(["h"] * len(reads))
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED and "post_chain_alignments" in str(e.value)


# ---- 8. the hook: kernels ran, the records did not travel ---------------------------------------------------------------
def test_kernels_run_and_only_the_text_travels():
    g, reads = make_world(9400, 21, genome_len=5000, n_reads=300, read_len=150)
    A = aligner.Aligner(gpu_graph(g), capi.config_cli(21))
    align_host(A, reads)
    headers = ["t%d" % i for i in range(len(reads))]
    before = aligner.format_kernel_launch_counts()
    text, lb = A.format_tsv_batch(headers)
    after = aligner.format_kernel_launch_counts()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[2] == before[2]
    # the text, the n + 1 offsets and 16 bytes of counters (the text's size, the number of capacity-status records: mgx.h)
    n = len(reads)
    assert after[3] - before[3] == len(text) + 8 * (n + 1) + 16
    assert after[3] - before[3] < 64 * n + len(text)                         # (the 64-byte records alone would be more)
    check_batch(A, headers, reads)


# ---- 9. the driver -------------------------------------------------------------------------------------------------------
def test_driver_format_on_device(tmp_path):
    from test_oracle_kats import read_fasta
    cli = KATS["cli"]
    g = orc.Graph.build(cli["k"], read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])), 0, False)
    W, last, F, _ = g.export()
    dump = tmp_path / "mt.boss"
    with open(dump, "wb") as f:
        f.write(struct.pack("<7Q", g.k, g.n_edges, *[int(x) for x in F]))
        f.write(W.tobytes())
        f.write(last.tobytes())
    exe = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
    reads = os.path.join(HERE, "golden", cli["reads_fastq"])
    for extra in ([], ["--align-only-forwards"], ["--query-batch-size", "300"]):
        base = [exe, str(dump), reads, "--align-min-exact-match", "0.0"] + extra
        ref = subprocess.run(base, capture_output=True, timeout=120)
        assert ref.returncode == 0, ref.stderr
        r = subprocess.run(base + ["--format-on-device"], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == ref.stdout and len(r.stdout) > 0
    for other in ("--rccl-gather", "--map"):
        r = subprocess.run([exe, str(dump), reads, "--format-on-device", other], capture_output=True, timeout=120)
        assert r.returncode == 1 and b"--format-on-device" in r.stderr and r.stdout == b""
