"""bench.py --dump-outputs on the CPU: dump_outputs() decodes raw result records in the device layout (ReadResult headers +
word stream, here written by the host model of the kernels) into float64 arrays, one per field, that hold every alignment
of the sampled reads exactly as the oracle computes them; over its byte budget it halves the sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import emu_drv  # noqa: E402
import orc  # noqa: E402
from metagraph_amd import capi  # noqa: E402
from test_emu_vs_oracle import make_world  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _to_py(a):
    """the dumped arrays as capi.results_to_py lists, one per sampled read"""
    out, nb, cb, sb = [], 0, 0, 0
    for q in range(len(a["read_index"])):
        alns = []
        for j in range(int(a["aln_begin"][q]), int(a["aln_begin"][q + 1])):
            nn, nc, ns = int(a["aln_n_nodes"][j]), int(a["aln_n_cigar"][j]), int(a["aln_seq_len"][j])
            d = {f: int(a["aln_" + f][j]) for f in ("score", "offset", "clipping", "end_clipping", "num_matches", "orientation")}
            d["nodes"] = [int(x) for x in a["nodes"][nb:nb + nn]]
            d["cigar"] = "".join("%d%s" % (int(ln), capi.OP_CHARS[int(op)])
                                 for ln, op in zip(a["cigar_len"][cb:cb + nc], a["cigar_op"][cb:cb + nc]))
            d["sequence"] = bytes(a["seqs"][sb:sb + ns].astype(np.uint8)).decode()
            nb, cb, sb = nb + nn, cb + nc, sb + ns
            alns.append(d)
        out.append(alns)
    return out


def _raw_world():
    k = 15
    g, reads = make_world(77, k, genome_len=3000, n_reads=60, read_len=90, n_variants=12)
    cfg = capi.config_cli(k)
    run = emu_drv.EmuRun(emu_drv.EmuGraph(g), cfg, reads)
    assert not run.error, run.error
    hb, sb = run.raw()
    return g, cfg, reads, np.frombuffer(hb, dtype=np.uint8), np.frombuffer(sb, dtype=np.uint8)


def test_dump_outputs_holds_the_decoded_results(tmp_path):
    g, cfg, reads, hb, sb = _raw_world()
    bench.dump_outputs(str(tmp_path), hb, sb, len(reads), False)
    a = _load(str(tmp_path))
    assert all(v.dtype == np.float64 for v in a.values())
    assert list(a["read_index"]) == list(range(len(reads)))          # (fewer reads than DUMP_READS: all of them, in order)
    assert (a["status"] == 0).all() and a["aln_begin"][-1] > 0
    assert _to_py(a) == orc.AlignRun(g, cfg, reads, validate=False).results()


def test_dump_outputs_is_seeded_and_keeps_to_its_budget(tmp_path, monkeypatch):
    g, cfg, reads, hb, sb = _raw_world()
    monkeypatch.setattr(bench, "DUMP_READS", 40)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 6000)
    outs = []
    for i in range(2):
        d = str(tmp_path / str(i))
        bench.dump_outputs(d, hb, sb, len(reads), False)
        outs.append(_load(d))
    a, b = outs
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= 6000 and 0 < len(a["read_index"]) < 40
    idx = a["read_index"].astype(np.int64)
    assert (np.diff(idx) > 0).all()
    assert _to_py(a) == orc.AlignRun(g, cfg, [reads[i] for i in idx], validate=False).results()
