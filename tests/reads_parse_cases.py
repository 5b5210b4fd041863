"""Shared by tests/test_reads_parse_model.py (CPU) and tests/test_gpu_parse_reads.py (GPU): a restatement of the FASTA / FASTQ
grammar of mgx_parse_reads, a seeded generator of files inside that grammar, the refusal cases, and the chunk feeder.

The grammar is kseq's `kseq_read` restricted to files where it is unambiguous.  kseq.h itself (htslib) is not part of the
reference tree (its submodules are empty), so `restate` below is written from kseq's documented behaviour and is what pins the
grammar — not the header.  Two points where kseq versions differ are therefore UNPINNED: the removal of '\\r' in front of
'\\n', and non-graphic bytes inside sequence lines (copied verbatim here)."""
import random

FASTA, FASTQ = 1, 2
SPACE = b" \t\n\v\f\r"


def _lines(data):
    """-> [(begin, payload)]: a line excludes its '\\n' and a '\\r' directly in front of it; an unterminated last line ends at the end"""
    out, at = [], 0
    parts = data.split(b"\n")
    last_terminated = data.endswith(b"\n")
    if last_terminated or not parts[-1]:
        parts.pop()
    for j, p in enumerate(parts):
        terminated = j + 1 < len(parts) or last_terminated
        begin = at
        at += len(p) + 1
        if terminated and p.endswith(b"\r"):
            p = p[:-1]
        out.append((begin, p))
    return out


def _name(payload):
    for j in range(1, len(payload)):
        if payload[j] in SPACE:
            return payload[1:j]
    return payload[1:]


def restate(data, flags=0):
    """One final parse of `data`.  -> {"format", "names": [bytes], "seqs": [bytes]} or {"invalid": byte position of the line}"""
    lines = _lines(data)
    first = next(((b, p) for b, p in lines if p), None)
    if first is None:
        return {"format": 0, "names": [], "seqs": []}
    if first[1][:1] not in (b">", b"@"):
        return {"invalid": first[0]}
    fmt = flags or (FASTA if first[1][:1] == b">" else FASTQ)
    errors, names, seqs = [], [], []
    if fmt == FASTA:
        for b, p in lines:
            if p[:1] == b">":
                names.append(_name(p))
                seqs.append([])
            elif p:
                if p[:1] in (b"@", b"+") or not seqs:
                    errors.append(b)
                else:
                    seqs[-1].append(p)
        seqs = [b"".join(s) for s in seqs]
    else:
        last = max(j + 1 for j, (_, p) in enumerate(lines) if p)
        groups, used = len(lines) // 4, (last + 3) // 4
        if used > groups:
            errors.append(lines[4 * groups][0])          # the last record has fewer than four lines
        for g in range(min(groups, used)):
            (b0, l0), (b1, l1), (b2, l2), (b3, l3) = lines[4 * g:4 * g + 4]
            if l0[:1] != b"@":
                errors.append(b0)
            if l1[:1] in (b"@", b"+", b">"):
                errors.append(b1)
            if l2[:1] != b"+":
                errors.append(b2)
            if len(l3) != len(l1):
                errors.append(b3)
            names.append(_name(l0) if l0 else b"")
            seqs.append(l1)
    if errors:
        return {"invalid": min(errors)}
    return {"format": fmt, "names": names, "seqs": seqs}


# ---- generator: only files inside the grammar --------------------------------------------------------------------------------
_GRAPHIC = bytes(range(33, 127))
_SEQ_ALPHABETS = [b"ACGT", b"ACGTN", b"acgtACGTNn", b"ACGT\x80\xff\xc3N", b"ACGTRYKMSWBDHVN-*."]


def _rand_name(rng):
    kind = rng.randrange(6)
    name = b"" if kind == 0 else bytes(rng.choice(_GRAPHIC) for _ in range(rng.randrange(1, 30)))
    comment = b""
    if rng.randrange(3) == 0:
        comment = rng.choice([b" ", b"\t"]) + bytes(rng.choice(_GRAPHIC + b" \t") for _ in range(rng.randrange(0, 25)))
    return name, name + comment


def _rand_seq(rng, n):
    alpha = rng.choice(_SEQ_ALPHABETS)
    if n > 5000:
        unit = bytes(rng.choice(alpha) for _ in range(997))
        return (unit * (n // 997 + 1))[:n]
    return bytes(rng.choice(alpha) for _ in range(n))


def make_file(rng, fmt, n_records=None, long_len=None, single_line=False):
    """-> (data, names, seqs).  long_len: the length of one long record; single_line (FASTA): every record on one line"""
    eol = b"\r\n" if rng.randrange(3) == 0 else b"\n"
    n_records = rng.randrange(0, 25) if n_records is None else n_records
    lens = [rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 150]) if rng.randrange(3) == 0 else rng.randrange(0, 1001) for _ in range(n_records)]
    if long_len is not None and n_records:
        lens[rng.randrange(n_records)] = long_len
    out, names, seqs = [], [], []
    width = None if single_line else rng.randrange(1, 201)
    if fmt == FASTA and rng.randrange(4) == 0:
        out += [b""] * rng.randrange(1, 3)                       # empty lines in front of the first header
    for L in lens:
        name, header = _rand_name(rng)
        seq = _rand_seq(rng, L)
        names.append(name)
        seqs.append(seq)
        if fmt == FASTA:
            out.append(b">" + header)
            w = width if width else max(1, L)
            if L > 5000 and width and width < 40:
                w = 60                                           # (a long record in one-byte lines would only make the test slow)
            for at in range(0, L, w):
                if rng.randrange(12) == 0 and L <= 5000:
                    out.append(b"")                              # an empty line inside the record
                out.append(seq[at:at + w])
            if rng.randrange(8) == 0:
                out.append(b"")
        else:
            kind = rng.randrange(6)
            qual = bytearray(rng.choice(_GRAPHIC) for _ in range(min(L, 1000)))
            if L > 1000:
                qual = bytearray((bytes(qual) * (L // 1000 + 1))[:L])
            if L and kind == 0:
                qual[0] = ord("@")
            if L and kind == 1:
                qual[0] = ord("+")
            out += [b"@" + header, seq, b"+" + (name if rng.randrange(5) == 0 else b""), bytes(qual)]
    if fmt == FASTQ and n_records and rng.randrange(4) == 0:
        out += [b""] * rng.randrange(1, 6)                       # empty lines after the last record
    data = b"".join(l + eol for l in out)
    # without the final newline (not where that would take the last record's empty fourth line away)
    if data and rng.randrange(3) == 0 and out[-1]:
        data = data[:-len(eol)]
    return data, names, seqs


def files(seed, n, with_long=True):
    """n seeded files, both formats; with_long: one record of 40 000 in each format and one FASTA record of 5 000 000 on one line"""
    rng = random.Random(seed)
    out = []
    for j in range(n):
        fmt = FASTA if j % 2 == 0 else FASTQ
        out.append(make_file(rng, fmt, single_line=(fmt == FASTA and j % 10 == 0)) + (fmt,))
    if with_long:
        out.append(make_file(rng, FASTA, n_records=3, long_len=40000) + (FASTA,))
        out.append(make_file(rng, FASTQ, n_records=3, long_len=40000) + (FASTQ,))
        out.append(make_file(rng, FASTA, n_records=2, long_len=5000000, single_line=True) + (FASTA,))
    return out


def chunk_sizes(rng, total, max_calls):
    """chunk sizes from 1 byte to the whole file (the feeder cycles through them); at most ~max_calls calls for the file"""
    floor = max(1, total // max_calls)
    scale = rng.choice([1, 7, 64, 1000, max(1, total // 3), max(1, total)])
    scale = min(max(scale, floor), max(1, total))
    return [rng.randrange(max(1, min(floor, scale)), scale + 1) for _ in range(16)]


# ---- refusals: each rule broken once -> (name, data, the byte position of the offending line) ------------------------------
def refusals():
    ok_fq = b"@r1 c\nACGT\n+\nIIII\n"
    cases = [
        ("fastq_line0_marker", ok_fq + b">r2\nAC\n+\nII\n", len(ok_fq)),
        ("fastq_line2_marker", ok_fq + b"@r2\nAC\n-\nII\n", len(ok_fq) + 7),
        ("fastq_unequal_lengths", ok_fq + b"@r2\nACG\n+\nII\n" + ok_fq, len(ok_fq) + 10),
        ("fastq_sequence_begins_with_at", ok_fq + b"@r2\n@CG\n+\nIII\n", len(ok_fq) + 4),
        ("fastq_multi_line", b"@r1\nACGT\nACGT\n+\nIIII\nIIII\n" + ok_fq, 9),
        ("fastq_truncated", ok_fq + b"@r2\nACG\n+\n", len(ok_fq)),
        ("first_line_no_marker", b"\nACGT\n>r1\nACGT\n", 1),
        ("fasta_plus_line", b">r1\nACGT\n+\nACGT\n>r2\nAC\n", 9),
        ("fasta_at_line", b">r1 x\nACGT\nAC\n@r2\nAC\n>r3\nA\n", 14),
    ]
    return cases


def records_of(offsets, seqs, name_offsets, names):
    n = len(offsets) - 1
    return ([bytes(names[int(name_offsets[r]):int(name_offsets[r + 1])]) for r in range(n)],
            [bytes(seqs[int(offsets[r]):int(offsets[r + 1])]) for r in range(n)])
