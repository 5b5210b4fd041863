"""mgx_format_map_batch on the GPU (k_mapfmt_size / k_mapfmt_write): the text of `align --map` for a whole batch, byte for byte
what the per-query host formatter mgx_format_map gives on a map_summary(..., want_nodes=True) of the same reads — the k = 11
genome.MT goldens, random BASIC / CANONICAL / PRIMARY worlds with awkward reads in all four formats, what travels and what is
launched, the refusals, reads handed over on the device by the parser, and host/mgx_align --map --map-on-device."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import orc
from metagraph_amd import aligner, capi
from map_goldens import BASIC_LINES, CANONICAL_LINES, HERE, K, SUBK_LENGTH, SUBK_LINES, read_fastq, triples
from test_gpu_map_summary import BASIC, NODE_BYTES, boss_dump, counters, gpu_graph, mt_fasta
from test_oracle_canonical import CANONICAL
from test_oracle_canonical_wrapper import PRIMARY
from test_emu_vs_oracle import make_world
from test_emu_canonical import canonical_world
from test_emu_primary import primary_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
NODES, COUNT, PRESENCE, FILTER = (capi.MGX_MAP_FMT_NODES, capi.MGX_MAP_FMT_COUNT_KMERS, capi.MGX_MAP_FMT_QUERY_PRESENCE,
                                  capi.MGX_MAP_FMT_FILTER_PRESENT)
FRACTIONS = [0.0, 0.5, 0.7, 1.0]


def host_texts(A, headers, reads, map_length, cases):
    """the yardstick: {(fmt, fraction): [text of every query]} by the mgx_format_map loop on a want_nodes summary"""
    A.map_summary(reads, map_length, want_nodes=True)
    m = A.last_map_summary
    return {(fmt, f): [A.format_map(m, i, headers[i], reads[i], fmt, map_length, f).encode("latin-1") for i in range(len(reads))]
            for fmt, f in cases}


def check_device_texts(A, headers, want):
    """format_map_batch of the staged batch against the yardstick: the text, and line_begin = the running sum"""
    for (fmt, f), lines in want.items():
        text, lb = A.format_map_batch(headers, fmt, f)
        assert text == b"".join(lines), (fmt, f)
        assert [int(x) for x in lb] == [0] + list(np.cumsum([len(l) for l in lines])), (fmt, f)


ALL_CASES = [(NODES, 0.7), (COUNT, 0.7)] + [(fmt, f) for fmt in (PRESENCE, FILTER) for f in FRACTIONS]


# ---- 1. the goldens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,lines,map_length", [(BASIC, BASIC_LINES, 0), (BASIC, SUBK_LINES, SUBK_LENGTH), (CANONICAL, CANONICAL_LINES, 0)])
def test_goldens(mode, lines, map_length):
    g = orc.Graph.build(K, mt_fasta(), mode, mode == CANONICAL)
    A = aligner.Aligner(gpu_graph(g, mode), capi.config_cli(K))
    recs = read_fastq()
    headers, reads = [r[0] for r in recs], [r[1] for r in recs]
    want = host_texts(A, headers, reads, map_length, [(NODES, 0.7)])
    A.map_summary(reads, map_length, keep_nodes=True)
    text, _ = A.format_map_batch(headers, COUNT)
    assert text == "".join(l + "\n" for l in lines).encode()
    check_device_texts(A, headers, want)
    assert text.count(b"\n") == 7 and [l.count(b"\n") for l in want[(NODES, 0.7)]] == [t[1] for t in triples(lines)]


# ---- 2. random worlds ----------------------------------------------------------------------------------------------------
def awkward(reads, k, seed):
    """the world's reads plus: empty, k - 1, k, k + 63, k + 64 characters, 400 and 5000 bp (the summary's long form), N runs, lower case"""
    rng = random.Random(seed)
    long_read = ""
    while len(long_read) < 5000:
        long_read += rng.choice(reads)
    out = list(reads)
    out += ["", reads[0][:k - 1], reads[1][:k], (reads[2] + reads[3])[:k + 63], (reads[4] + reads[5])[:k + 64],
            (reads[6] + reads[7] + reads[8])[:400], long_read[:5000], reads[9][:20] + "NNNNN" + reads[9][25:], reads[10].lower(),
            "N" * (k + 3), reads[11][:40].lower() + "n" + reads[11][41:]]
    return out


@pytest.mark.parametrize("kind", ["basic", "canonical", "primary"])
def test_worlds(kind):
    k = 21
    if kind == "basic":
        (g, reads), mode = make_world(9700, k, genome_len=6000, n_reads=120, read_len=150, mask=True), BASIC
    elif kind == "canonical":
        (g, reads), mode = canonical_world(9701, k, genome_len=6000, n_reads=120, read_len=150), CANONICAL
    else:
        (g, reads), mode = primary_world(9702, k, genome_len=6000, n_reads=120, read_len=150), PRIMARY
    reads = awkward(reads, k, 3)
    headers = ["r%d/%s" % (i, "x" * (i % 9)) for i in range(len(reads))]
    A = aligner.Aligner(gpu_graph(g, mode), capi.config_cli(k))
    for map_length in (0, k, 7):
        if mode == PRIMARY and map_length == 7:
            with pytest.raises(aligner.MgxError) as e:           # the summary's refusal comes through
                A.map_summary(reads, map_length, keep_nodes=True)
            assert e.value.code == capi.MGX_ERR_UNSUPPORTED
            continue
        want = host_texts(A, headers, reads, map_length, ALL_CASES)
        A.map_summary(reads, map_length, keep_nodes=True)
        check_device_texts(A, headers, want)
        # the batch shows both answers of the presence rule and the lower-case / N bytes as they came
        assert {l for l in want[(PRESENCE, 0.7)]} == {b"0\n", b"1\n"}
        nodes_text = b"".join(want[(NODES, 0.7)])
        assert b"n" in nodes_text and b"N" in nodes_text and b"a" in nodes_text
    # without nodes the three other forms are the same; the k-mer: node form is refused
    want = host_texts(A, headers, reads, 0, [c for c in ALL_CASES if c[0] != NODES])
    A.map_summary(reads, 0)
    check_device_texts(A, headers, want)


# ---- 3. what travels, what is launched -----------------------------------------------------------------------------------
def test_traffic_and_launches():
    g, reads = make_world(9710, 21, genome_len=6000, n_reads=200, read_len=150)
    A = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(21))
    headers = ["t%d" % i for i in range(len(reads))]
    before_map = counters()
    counts = A.map_summary(reads, keep_nodes=True)
    assert counters()[NODE_BYTES] == before_map[NODE_BYTES], "KEEP_NODES copied the node array to the host"
    m = A.last_map_summary
    assert not m.node_begin and not m.nodes
    before = aligner.format_map_kernel_launch_counts()
    text, lb = A.format_map_batch(headers, NODES)
    after = aligner.format_map_kernel_launch_counts()
    n = len(reads)
    assert counters()[NODE_BYTES] == before_map[NODE_BYTES]
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1
    assert after[2] - before[2] == len(text) + 8 * (n + 1) + 16
    # host-to-device: the headers and their offsets (the k-mer: node form looks up no presence threshold: one word)
    assert after[3] - before[3] == sum(len(h) for h in headers) + 8 * (n + 1) + 8
    assert text.count(b"\n") == sum(c[1] for c in counts) and int(lb[-1]) == len(text)


# ---- 4. the refusals -----------------------------------------------------------------------------------------------------
def test_refusals_and_unchanged_summaries():
    g, reads = make_world(9711, 21, genome_len=3000, n_reads=20, read_len=100)
    A = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(21))
    headers = ["h%d" % i for i in range(len(reads))]

    def refused(call, word):
        with pytest.raises(aligner.MgxError) as e:
            call()
        assert e.value.code == capi.MGX_ERR_INVALID and word in str(e.value), str(e.value)

    refused(lambda: A.format_map_batch(headers, COUNT), "has not run")                     # never run
    plain = A.map_summary(reads)
    L = capi.lib()
    t = capi.Text()
    hoff = np.arange(len(reads) + 1, dtype=np.uint64)
    for args in ((None, b"x" * len(reads), hoff.ctypes.data, COUNT, 0.7, C.byref(t)), (A.h, None, hoff.ctypes.data, COUNT, 0.7, C.byref(t)),
                 (A.h, b"x" * len(reads), None, COUNT, 0.7, C.byref(t)), (A.h, b"x" * len(reads), hoff.ctypes.data, COUNT, 0.7, None)):
        assert L.mgx_format_map_batch(*args) == capi.MGX_ERR_INVALID and b"null argument" in L.mgx_last_error()
    refused(lambda: A.format_map_batch(headers, 4), "unknown format")
    refused(lambda: A.format_map_batch(headers, -1), "unknown format")
    refused(lambda: A.format_map_batch(headers, NODES), "KEEP_NODES")                     # the summary kept no nodes
    A.format_map_batch(headers, COUNT)                                                     # (the batch itself is fine)
    A.align_batch(reads)
    refused(lambda: A.format_map_batch(headers, COUNT), "ran on this handle after")
    A.map_summary(reads, keep_nodes=True)
    A.map_batch(reads)
    refused(lambda: A.format_map_batch(headers, NODES), "ran on this handle after")
    # ... and the call that follows a fresh summary works
    A.map_summary(reads, keep_nodes=True)
    text, _ = A.format_map_batch(headers, NODES)
    assert text.count(b"\n") == sum(c[1] for c in plain)
    # the new flag changes nothing about the old ones: WANT_NODES nodes and KEEP_NODES counts against a plain run
    counts_w, nodes_w = A.map_summary(reads, want_nodes=True)
    B = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(21))
    counts_b, nodes_b = B.map_summary(reads, want_nodes=True)
    assert counts_w == plain == counts_b and nodes_w == nodes_b
    assert A.map_summary(reads, keep_nodes=True) == plain
    m = A.last_map_summary
    assert not m.node_begin and not m.nodes
    with pytest.raises(aligner.MgxError) as e:
        L_flags = capi.MapSummary()
        aligner._check(L.mgx_map_summary_batch(A.h, b"ACGT", hoff.ctypes.data, 0, 0, 0, 4, C.byref(L_flags)))
    assert e.value.code == capi.MGX_ERR_INVALID


# ---- 5. reads given on the device ------------------------------------------------------------------------------------------
def test_reads_from_the_parser():
    g, reads = make_world(9712, 21, genome_len=4000, n_reads=60, read_len=150)
    reads = awkward(reads, 21, 5)
    reads = [r for r in reads if r]                        # (a FASTQ record has a sequence line)
    names = ["q%d" % i for i in range(len(reads))]
    data = "".join("@%s some comment\n%s\n+\n%s\n" % (nm, r, "I" * len(r)) for nm, r in zip(names, reads)).encode()
    A = aligner.Aligner(gpu_graph(g, BASIC), capi.config_cli(21))
    cases = [(NODES, 0.7), (COUNT, 0.7), (PRESENCE, 0.5), (FILTER, 0.5)]
    want = host_texts(A, names, reads, 0, cases)
    parser = aligner.ReadParser()
    parsed = parser.parse(data)
    assert parsed.n_records == len(reads)
    A.map_summary(parsed.device_slice(), keep_nodes=True)
    check_device_texts(A, parsed.names_of(), want)
    # a sub-batch of the parse
    A.map_summary(parsed.device_slice(7, 20), keep_nodes=True)
    text, _ = A.format_map_batch(parsed.names_of(7, 20), NODES)
    assert text == b"".join(want[(NODES, 0.7)][7:27])


# ---- 6. the driver -------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "metagraph_amd", "_build", "mgx_align")
READS = os.path.join(HERE, "golden", "genome_MT1.fq")


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_on_device")
    dump, cdump = str(d / "mt.boss"), str(d / "mt.canonical.boss")
    boss_dump(orc.Graph.build(K, mt_fasta(), BASIC, False), dump)
    boss_dump(orc.Graph.build(K, mt_fasta(), CANONICAL, False), cdump)
    return {"basic": dump, "canonical": cdump}


def run(*args, status=0):
    r = subprocess.run([EXE] + list(args), capture_output=True, timeout=120)
    assert r.returncode == status, r.stderr
    return r


# the run(...) lines of test_gpu_map_summary.test_mgx_align_map_driver
DRIVER_LINES = [("basic", ["--map", "--count-kmers"]),
                ("basic", ["--map", "--count-kmers", "--align-length", "10"]),
                ("canonical", ["--canonical", "--map", "--count-kmers"]),
                ("basic", ["--map", "--query-presence", "--discovery-fraction", "0.5"]),
                ("canonical", ["--canonical", "--map", "--query-presence", "--discovery-fraction", "0.5"]),
                ("basic", ["--map", "--query-presence", "--filter-present", "--discovery-fraction", "0.5"]),
                ("basic", ["--map", "--count-kmers", "--align-length", "12"]),
                ("basic", ["--map"]),
                ("basic", ["--map", "--query-batch-size", "300", "--parse-chunk-bytes", "500"]),
                ("basic", ["--map", "--align-length", "10", "--query-batch-size", "300", "--parse-chunk-bytes", "500"])]


@pytest.mark.parametrize("line", range(len(DRIVER_LINES)))
def test_driver_map_on_device(dumps, line):
    graph, args = DRIVER_LINES[line]
    plain = run(dumps[graph], READS, *args).stdout
    assert len(plain) > 0
    assert run(dumps[graph], READS, *args, "--map-on-device").stdout == plain
    assert run(dumps[graph], READS, *args, "--map-on-device", "--parse-on-device").stdout == plain
    if line == 0:
        assert plain == "".join(l + "\n" for l in BASIC_LINES).encode()


def test_driver_fwd_and_reverse_and_time(dumps):
    args = [dumps["canonical"], READS, "--canonical", "--map", "--count-kmers", "--fwd-and-reverse"]
    plain = run(*args).stdout
    assert plain.count(b"\n") == 14
    assert run(*args, "--map-on-device").stdout == plain
    r = run(dumps["basic"], READS, "--map", "--map-on-device", "--parse-on-device", "--time")
    assert b"7 queries in 1 batches" in r.stderr


def test_driver_refusals(dumps):
    dump = dumps["basic"]
    for args, words in ((["--map", "--map-on-device", "--parse-on-device", "--fwd-and-reverse"], [b"--parse-on-device", b"--fwd-and-reverse"]),
                        (["--map", "--map-on-device", "--parse-on-device", "-p", "2"], [b"--parse-on-device", b"-p 1"]),
                        (["--map", "--map-on-device", "--parse-on-device", "--devices", "2"], [b"--parse-on-device", b"--devices 1"]),
                        (["--map-on-device"], [b"--map-on-device", b"--map"]),
                        (["--map-on-device", "--format-on-device"], [b"--map-on-device"])):
        r = run(dump, READS, *args, status=1)
        assert r.stdout == b"" and all(w in r.stderr for w in words), r.stderr
    # the two old refusals, unchanged
    r = run(dump, READS, "--format-on-device", "--map", status=1)
    assert b"--format-on-device" in r.stderr and r.stdout == b""
    r = run(dump, READS, "--parse-on-device", "--format-on-device", "--map", status=1)
    assert b"--parse-on-device" in r.stderr and b"--map" in r.stderr and r.stdout == b""
    # ... also with the new flag next to them
    r = run(dump, READS, "--format-on-device", "--map", "--map-on-device", status=1)
    assert b"--format-on-device" in r.stderr and r.stdout == b""
