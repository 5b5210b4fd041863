"""The FASTA / FASTQ parser's logic (metagraph_amd/csrc/reads_parse.hpp: the line, classify, records and copy passes of
mgx_parse_reads) compiled for the host against the wave model (tests/emu/wave.hpp) by tests/emu/reads_parse_check.cpp, and
compared with the restatement of the grammar in tests/reads_parse_cases.py.  CPU only.

What pins the grammar: kseq.h (htslib) is not part of the reference tree (its submodules are empty), so the restatement is
written from kseq's documented behaviour (`kseq_read`, restricted to files where it is unambiguous) and not checked against the
header.  UNPINNED, because kseq versions differ there: the removal of '\\r' in front of '\\n', and non-graphic bytes inside
sequence lines (copied verbatim).

Inputs (seeded, all inside the grammar): FASTA with line widths 1 - 200 and records on a single line, FASTQ, names of graphic
bytes with and without a comment behind a space or a tab, empty names, sequence lengths 0 - 1000 plus 40 000 and 5 000 000, LF
and CRLF, with and without a final newline, empty lines inside FASTA records and after the last FASTQ record, quality lines that
begin with '@' and '+', lower case, N and bytes >= 0x80.  Every file is parsed in one piece and in chunks of random sizes from
one byte to the whole file (following `consumed`), at every alignment of the text.  Refusals: each rule broken once."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import reads_parse_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads_parse")
    exe = str(d / "reads_parse_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + emu, "-o", exe, os.path.join(emu, "reads_parse_check.cpp")], check=True)

    def run(cases):
        """cases: [(data, flags, mis, sizes)] -> one dict per case"""
        src, dst = str(d / "cases.bin"), str(d / "results.bin")
        with open(src, "wb") as f:
            for data, flags, mis, sizes in cases:
                f.write(struct.pack("<QIIII", len(data), flags, mis, len(sizes), 0))
                f.write(np.asarray(sizes, dtype=np.uint64).tobytes())
                f.write(data)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok %d cases" % len(cases)), out.stdout + out.stderr
        raw, at, res = open(dst, "rb").read(), 0, []
        for _ in cases:
            code, err_pos, n, consumed, fmt, seq_bytes, name_bytes, calls = struct.unpack_from("<qQQQQQQQ", raw, at)
            at += 64
            offsets = np.frombuffer(raw, dtype=np.uint64, count=n + 1, offset=at); at += 8 * (n + 1)
            name_offsets = np.frombuffer(raw, dtype=np.uint64, count=n + 1, offset=at); at += 8 * (n + 1)
            seqs = raw[at:at + seq_bytes]; at += seq_bytes
            names = raw[at:at + name_bytes]; at += name_bytes
            res.append({"rc": code, "err_pos": err_pos, "n": n, "consumed": consumed, "format": fmt, "offsets": offsets,
                        "name_offsets": name_offsets, "seqs": seqs, "names": names, "calls": calls})
        assert at == len(raw)
        return res
    return run


def _check(got, data, names, seqs, fmt):
    want = rc.restate(data)
    assert "invalid" not in want, "the generator left the grammar"
    assert want["names"] == names and want["seqs"] == seqs          # the restatement reads back what the generator wrote
    assert got["rc"] == 0 and got["n"] == len(seqs) and got["consumed"] == len(data)
    assert got["format"] == (fmt if seqs else 0)
    assert int(got["offsets"][0]) == 0 and int(got["name_offsets"][0]) == 0
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64).tolist()
    assert got["name_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uint64).tolist()
    assert got["seqs"] == b"".join(seqs) and got["names"] == b"".join(names)


def test_generated_files_whole_and_in_chunks(checker):
    files = rc.files(20251017, 240)
    rng = random.Random(7)
    cases = []
    for data, names, seqs, fmt in files:
        cases.append((data, 0, rng.randrange(16), [max(1, len(data))]))                              # one final call
        cases.append((data, 0, rng.randrange(16), rc.chunk_sizes(rng, len(data), 400)))
        cases.append((data, 0, rng.randrange(16), rc.chunk_sizes(rng, len(data), 400)))
    res = checker(cases)
    n_chunked = 0
    for j, (data, names, seqs, fmt) in enumerate(files):
        for got in res[3 * j:3 * j + 3]:
            _check(got, data, names, seqs, fmt)
        assert res[3 * j]["calls"] == 1
        n_chunked += res[3 * j + 1]["calls"] > 1
    assert n_chunked > len(files) // 2
    # the generator covers what the issue lists
    blob = b"".join(f[0] for f in files[:240])
    assert b"\r\n" in blob and any(not f[0].endswith(b"\n") for f in files if f[0]) and any(b"" in f[1] for f in files)
    assert any(len(s) == 5000000 for f in files for s in f[2]) and any(len(s) == 40000 for f in files for s in f[2])
    assert any(0 in [len(s) for s in f[2]] for f in files) and b"\x80" in blob and b"\n\n>" in blob


def test_tiny_and_empty_inputs(checker):
    cases = [b"", b"\n", b"\r\n\n", b">", b">\n", b">a", b"@\n\n+\n\n", b"@a b\nA\n+a\n@", b">x\n\n\nAC\n\nG", b"@r\nAC\n+\n+@\n\n\n\n\n\n"]
    res = checker([(d, 0, 3, [max(1, len(d))]) for d in cases] + [(d, 0, 5, [1]) for d in cases])
    for j, got in enumerate(res):
        data = cases[j % len(cases)]
        want = rc.restate(data)
        _check(got, data, want["names"], want["seqs"], want["format"])
    assert res[len(cases) + 7]["calls"] > 4


def test_forced_format(checker):
    # a FASTA file whose first record is named "@..." read as FASTA although nothing else says so; a forced FASTQ on FASTA text is refused
    got = checker([(b">r\nAC\n", rc.FASTA, 0, [6]), (b">r\nAC\n+\nII\n", rc.FASTQ, 0, [12]), (b"ACGT\n>r\nAC\n", rc.FASTA, 0, [11])])
    assert got[0]["rc"] == 0 and got[0]["n"] == 1
    assert got[1]["rc"] == -1 and got[1]["err_pos"] == 0
    assert got[2]["rc"] == -1 and got[2]["err_pos"] == 0


@pytest.mark.parametrize("case", rc.refusals(), ids=lambda c: c[0])
def test_refusals(checker, case):
    name, data, pos = case
    assert rc.restate(data) == {"invalid": pos}
    rng = random.Random(len(data))
    for got in checker([(data, 0, 0, [len(data)]), (data, 0, 9, [1]), (data, 0, 2, rc.chunk_sizes(rng, len(data), 50))]):
        assert got["rc"] == -1 and got["err_pos"] == pos and got["n"] == 0
