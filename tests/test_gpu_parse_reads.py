"""mgx_parse_reads (FASTA / FASTQ text to read batches on the device: csrc/reads_parse.hpp, csrc/mgx_parse.hip) against the
restatement of the grammar in tests/reads_parse_cases.py, and the text-to-text path it opens: parse, align from the parser's
device arrays, format with the parser's names — compared with the existing host-input path.  Needs a real MI355X.

What pins the grammar: kseq.h (htslib) is not part of the reference tree (its submodules are empty), so the restatement is
written from kseq's documented behaviour and not checked against the header.  UNPINNED, because kseq versions differ there: the
removal of '\\r' in front of '\\n', and non-graphic bytes inside sequence lines."""
import ctypes as C
import glob
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import orc
import reads_parse_cases as rpc
from metagraph_amd import aligner, capi
from test_emu_vs_oracle import make_world, KATS
from test_emu_canonical import canonical_world
from test_emu_primary import primary_world
from test_oracle_canonical import CANONICAL
from test_oracle_primary_goldens import PRIMARY

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# device-to-host bytes of a parse of host text besides the names and the two offset arrays: the line count (4) and the counters (48)
PARSE_D2H_CONSTANT = 52


@pytest.fixture(scope="module")
def parser():
    p = aligner.ReadParser()
    yield p
    p.close()


def _arrays(r):
    seqs, offs = r.to_host()
    assert offs.tolist() == r.host_offsets.tolist()
    return rpc.records_of(offs, seqs, r.name_offsets, r.names)


def _feed(parser, data, sizes, device_text=None):
    """the chunk feeder of the model test on the device -> (names, seqs, format, calls) or raises MgxError"""
    names, seqs, fmt, at, have, calls = [], [], 0, 0, 0, 0
    for kx in range(10 ** 9):
        have += sizes[kx % len(sizes)]
        final = at + have >= len(data)
        if final:
            have = len(data) - at
        try:
            if device_text is not None:
                r = parser.parse(device_text + at, final=final, text_on_device=True, flags=fmt, n_bytes=have)
            else:
                r = parser.parse(data[at:at + have], final=final, flags=fmt)
        except aligner.MgxError as e:
            e.at = at
            raise
        calls += 1
        fmt = fmt or r.format
        nm, sq = _arrays(r)
        names += nm
        seqs += sq
        at += r.consumed
        have -= r.consumed
        if final:
            assert at == len(data)
            return names, seqs, fmt, calls


def _error_position(e):
    msg = str(e)
    assert "byte " in msg, msg
    return e.at + int(msg.split("byte ")[1].split()[0].rstrip(":"))


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------------
def test_goldens(parser):
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "*.fa")) + glob.glob(os.path.join(HERE, "golden", "*.fq")))
    assert len(paths) == 6
    for path in paths:
        data = open(path, "rb").read()
        # inside the grammar: LF only, a final newline, no empty lines; the FASTQ strictly four lines per record
        assert b"\r" not in data and data.endswith(b"\n") and b"\n\n" not in data
        want = rpc.restate(data)
        assert "invalid" not in want and want["format"] == (rpc.FASTQ if path.endswith(".fq") else rpc.FASTA)
        if path.endswith("genome_MT1.fq"):
            assert data.count(b"\n") == 4 * len(want["seqs"])
        r = parser.parse(data)
        assert r.n_records == len(want["seqs"]) > 0 and r.consumed == len(data) and r.format == want["format"]
        assert _arrays(r) == (want["names"], want["seqs"])
    mt = open(os.path.join(HERE, "golden", "genome.MT.fa"), "rb").read()
    assert b" " in mt[:mt.index(b"\n")] and parser.parse(mt).name_list()[0] == mt[1:mt.index(b" ")]


# ---- 2. random files, chunked, both text_on_device values, the refusals ----------------------------------------------------------
def test_random_files_whole_and_in_chunks(parser):
    import torch
    files = rpc.files(20251018, 220)
    assert len(files) >= 200
    rng = random.Random(11)
    n_chunked = 0
    for j, (data, names, seqs, fmt) in enumerate(files):
        want = rpc.restate(data)
        assert want.get("names") == names and want.get("seqs") == seqs
        r = parser.parse(data)
        assert (r.n_records, r.consumed, r.format) == (len(seqs), len(data), fmt if seqs else 0)
        assert _arrays(r) == (names, seqs)
        # the text in device memory, at every alignment of its first byte
        if data:
            mis = j % 16
            t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
            t[mis:mis + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            r = parser.parse(t.data_ptr() + mis, text_on_device=True, n_bytes=len(data))
            assert r.n_records == len(seqs) and _arrays(r) == (names, seqs)
            sizes = rpc.chunk_sizes(rng, len(data), 24)
            got = _feed(parser, data, sizes, device_text=(t.data_ptr() + mis) if j % 2 else None)
            assert got[:2] == (names, seqs)
            n_chunked += got[3] > 1
    assert n_chunked > len(files) // 3


@pytest.mark.parametrize("case", rpc.refusals(), ids=lambda c: c[0])
def test_refusals(parser, case):
    name, data, pos = case
    L = capi.lib()
    assert rpc.restate(data) == {"invalid": pos}
    for sizes in ([len(data)], [5], [1]):
        with pytest.raises(aligner.MgxError) as ei:
            _feed(parser, data, sizes)
        assert ei.value.code == capi.MGX_ERR_INVALID and _error_position(ei.value) == pos
    # `out` is untouched by a refused call
    out = capi.Reads()
    out.n_records = 12345
    buf = np.frombuffer(data, dtype=np.uint8)
    rc_ = L.mgx_parse_reads(parser.h, buf.ctypes.data, len(data), 0, 1, 0, C.byref(out))
    assert rc_ == capi.MGX_ERR_INVALID and out.n_records == 12345


def test_refused_parse_ends_previous_views(parser):
    """after a refusal the handle holds no records: a slice of the previous parse is an error, not stale data"""
    good = parser.parse(b"@a\nACGT\n+\nIIII\n@b\nGG\n+\nII\n")
    assert good.n_records == 2 and good.device_slice(1, 1)[2] == 1
    with pytest.raises(aligner.MgxError):
        parser.parse(b"@a\nACGT\n+\nIII\n")
    with pytest.raises(aligner.MgxError) as ei:
        good.device_slice(1, 1)
    assert ei.value.code == capi.MGX_ERR_INVALID
    offs = np.full(3, 77, dtype=np.uint64)
    assert capi.lib().mgx_read_parser_fetch(parser.h, None, offs.ctypes.data) == 0 and offs.tolist() == [0, 77, 77]


def test_limits(parser):
    out = capi.Reads()
    rc_ = capi.lib().mgx_parse_reads(parser.h, b">x\n", 1 << 32, 0, 1, 0, C.byref(out))
    assert rc_ == capi.MGX_ERR_INVALID and b"2^32" in capi.lib().mgx_last_error()


# ---- 3. text to text -----------------------------------------------------------------------------------------------------------
def _gpu_graph(g, mode=0):
    W, last, F, valid = g.export()
    return aligner.Graph(g.k, W, last, F, valid, mode=mode)


def _fastq(headers, reads):
    return b"".join(b"@" + h + b" a comment\n" + q + b"\n+\n" + b"I" * len(q) + b"\n" for h, q in zip(headers, reads))


def _text_to_text(parser, A, reads, label_names=None):
    reads = [q if isinstance(q, bytes) else q.encode("latin-1") for q in reads]
    reads = [q[:len(q) - i % 7] for i, q in enumerate(reads)]                 # mixed lengths: record boundaries at odd bytes
    headers = [b"read_%d/x" % i for i in range(len(reads))]
    # the existing host-input path
    blob, offs = aligner.pack_queries(reads)
    assert capi.lib().mgx_align_batch_device(A.h, blob, offs.ctypes.data, len(reads), 0) == 0, capi.lib().mgx_last_error()
    want, want_lb = A.format_tsv_batch(headers, label_names)
    assert want.count(b"\n") == len(reads)
    # the parser's device arrays and names
    r = parser.parse(_fastq(headers, reads))
    assert r.n_records == len(reads) and r.name_list() == headers
    A.align_batch_device(r)
    got, lb = A.format_tsv_batch(r.names_of(), label_names)
    assert got == want and lb.tolist() == want_lb.tolist()
    # ... cut into two sub-batches at a record in the middle whose sequence starts at no multiple of 16 bytes: the second
    # sub-batch's seqs pointer is misaligned and its offsets are rebased
    b = next(i for i in range(len(reads) // 2, len(reads)) if int(r.host_offsets[i]) % 16)
    parts = []
    for first, n in ((0, b), (b, len(reads) - b)):
        A.align_batch_device(r, first, n)
        parts.append(A.format_tsv_batch(r.names_of(first, n), label_names)[0])
    assert b"".join(parts) == want
    return want


@pytest.mark.parametrize("mode", ["basic", "canonical", "primary"])
def test_text_to_text(parser, mode):
    build = {"basic": make_world, "canonical": canonical_world, "primary": primary_world}[mode]
    g, reads = build(9201, 21, genome_len=6000, n_reads=96, read_len=150)
    G = _gpu_graph(g, {"basic": 0, "canonical": CANONICAL, "primary": PRIMARY}[mode])
    A = aligner.Aligner(G, capi.config_cli(21))
    text = _text_to_text(parser, A, reads)
    assert b"\t+\t" in text or b"\t-\t" in text


def test_text_to_text_labeled(parser):
    from labeled_worlds import labeled_world
    g, anno, reads = labeled_world(12, 15, n_strains=3, n_reads=40)
    W, last, F, valid = g.export()
    A = aligner.Aligner(aligner.Graph(15, W, last, F, valid), capi.config_cli(15),
                        annotation=aligner.Annotation(g.n_edges, [anno.column_words(j) for j in range(anno.n_labels)]))
    text = _text_to_text(parser, A, reads, ["strain_%d" % j for j in range(anno.n_labels)])
    assert b"strain_" in text


# ---- 4. what travels back -----------------------------------------------------------------------------------------------------
def test_copy_counter(parser):
    rng = random.Random(5)
    reads = [bytes(rng.choice(b"ACGT") for _ in range(150)) for _ in range(2000)]
    headers = [b"r%d" % i for i in range(len(reads))]
    data = _fastq(headers, reads)
    before = aligner.parse_kernel_launch_counts()
    r = parser.parse(data)
    after = aligner.parse_kernel_launch_counts()
    n = len(reads)
    assert r.n_records == n
    assert after[0] > before[0] and after[1] > before[1]
    assert after[2] - before[2] == len(data)                                    # the text crosses once
    assert after[3] - before[3] == len(b"".join(headers)) + 2 * 8 * (n + 1) + PARSE_D2H_CONSTANT
    assert after[3] - before[3] < 150 * n                                       # (the sequences alone would be more)
    assert _arrays(r) == (headers, reads)


# ---- 5. the driver --------------------------------------------------------------------------------------------------------------
def test_driver_parse_on_device(tmp_path):
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
    # a generated FASTQ of a few thousand reads of the graph's genome: several batches, several chunks
    genome = "".join(read_fasta(os.path.join(HERE, "golden", cli["graph_fasta"])))
    rng = random.Random(3)
    reads = []
    for i in range(3000):
        at = rng.randrange(0, len(genome) - 160)
        q = bytearray(genome[at:at + rng.randrange(40, 160)].encode())
        if i % 3 == 0:
            q[len(q) // 2] = ord("ACGT"[rng.randrange(4)])
        reads.append(bytes(q))
    many = tmp_path / "many.fq"
    many.write_bytes(_fastq([b"q%d" % i for i in range(len(reads))], reads))
    runs = [(os.path.join(HERE, "golden", "genome_MT1.fq"), []), (os.path.join(HERE, "golden", "transcripts_100.fa"), []),
            (str(many), ["--query-batch-size", "20000", "--parse-chunk-bytes", "50000"])]
    for path, extra in runs:
        base = [exe, str(dump), path, "--align-min-exact-match", "0.0", "--format-on-device"] + extra
        ref = subprocess.run(base, capture_output=True, timeout=300)
        assert ref.returncode == 0, ref.stderr
        r = subprocess.run(base + ["--parse-on-device"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == ref.stdout and len(r.stdout) > 0
    fq = runs[0][0]
    for args, word in ((["--format-on-device", "--map"], b"--map"), (["--format-on-device", "--rccl-gather"], b"--rccl-gather"),
                       ([], b"--format-on-device"), (["--format-on-device", "-p", "2"], b"-p 1")):
        r = subprocess.run([exe, str(dump), fq, "--parse-on-device"] + args, capture_output=True, timeout=120)
        assert r.returncode == 1 and b"--parse-on-device" in r.stderr and word in r.stderr and r.stdout == b""
    multi = tmp_path / "multi.fq"
    multi.write_bytes(b"@r1\nACGTACGTACGTACGTACGTACGT\nACGTACGTACGTACGTACGTACGT\n+\n" + b"I" * 24 + b"\n" + b"I" * 24 + b"\n")
    r = subprocess.run([exe, str(dump), str(multi), "--format-on-device", "--parse-on-device"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"byte 29" in r.stderr and b"without --parse-on-device" in r.stderr and r.stdout == b""
