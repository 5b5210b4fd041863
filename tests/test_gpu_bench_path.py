"""bench.py end to end at reduced size on one GPU, launched the way the driver launches N > 1 (torch.distributed.run,
backend nccl = RCCL): the synthetic workload generator (metagraph_amd/synth.py), the device-resident step, the
complete-alignment gather through RCCL (world size 1 executes mgx_device_results -> all_gather / gather), the
host-inclusive variant, and the oracle comparison of every read of the CPU sample (those legs run with --full); and the plain
run with the results it writes (--dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_step_under_torchrun_nccl_single_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MGX_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--reads", "30000", "--genome", "300000", "--snps", "600", "--cpu-sample", "30000", "--cpu-1t-sample", "300",
           "--host-steps", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["value_device_resident"] > 0 and out["value_is"].startswith("host-inclusive")
    assert out["parity"]["sample"] == 30000 and out["parity"]["mismatches"] == 0 and out["parity"]["capacity_errors"] == 0
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["single_thread"]["value"] > 0


@pytest.mark.gpu
def test_bench_config3_labels_at_reduced_size():
    """BASELINE config 3 through bench.py: the annotation built on the device from the genome's mapped nodes
    (mgx_map_batch -> mgx_annotation_create_sparse), the label-aware aligner on the 8-reads-per-wavefront labeled kernel,
    alignments AND label lists of the sample against the oracle's LabeledAligner"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--labels", "40", "--steps", "1", "--warmup", "1",
           "--reads", "40000", "--genome", "400000", "--snps", "800", "--parity-sample", "1500", "--host-steps", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert "label-aware" in out["config"]["workload"] and out["value"] > 0
    assert out["parity"]["sample"] == 1500 and out["parity"]["mismatches"] == 0 and out["parity"]["capacity_errors"] == 0
    assert out["parity"]["full_batch_capacity_errors"] == 0
    assert out["roofline"]["kernel_ms"]["k_extend"] > 0 and out["cpu_baseline"]["cores"] == 1


@pytest.mark.gpu
def test_bench_config3_1000_labels_at_a_million_reads():
    """BASELINE config 3 at its own graph and annotation (104 M-edge graph, 1000 labels) with 1 M reads: the lane-per-read kernel in
    front of the labeled group kernel (round 6) — most reads must finish in the lane — and every read of a 20 000-read sample
    equal to the oracle's LabeledAligner, label lists included."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--labels", "1000", "--reads", "1000000", "--steps", "1", "--warmup", "1",
           "--parity-sample", "20000", "--no-cpu-baseline", "--host-steps", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert "1000-label" in out["config"]["workload"] and out["config"]["graph_edges"] > 100_000_000
    assert out["parity"]["sample"] == 20000 and out["parity"]["mismatches"] == 0 and out["parity"]["capacity_errors"] == 0
    assert out["parity"]["full_batch_capacity_errors"] == 0
    km = out["roofline"]["kernel_ms"]
    assert km.get("k_lane", 0) > 0 and km["reads_finished_by_k_lane"] >= 0.9 * 1_000_000, km


def _bench_outputs(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) prints the headline alone: --steps timed batches of the host-inclusive path and nothing of the
    measurements --full adds.  --dump-outputs writes the last timed batch's results (a seeded sample of reads, float64) — the
    same arrays from the device-resident path (--host-steps 0), and every sampled read's alignments equal the oracle's."""
    import numpy as np
    small = ["--gpus", "1", "--warmup", "1", "--reads", "30000", "--genome", "300000", "--snps", "600"]
    outs = []
    for i, extra in enumerate((["--steps", "3"], ["--steps", "2", "--host-steps", "0"])):
        d = str(tmp_path / ("out%d" % i))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + extra + ["--dump-outputs", d],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        outs.append((json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]), _bench_outputs(d)))
    plain, dev = outs[0][0], outs[1][0]
    assert plain["value_is"].startswith("host-inclusive") and plain["steps"] == 3 and plain["ms_per_step"] > 0
    assert plain["value"] > 0 and plain["full"] is False and plain["dtype"] == "int32" and plain["higher_is_better"] is True
    assert not any(k in plain for k in ("roofline", "parity", "cpu_baseline", "value_device_resident"))
    assert dev["value_is"].startswith("device-resident") and dev["steps"] == 2 and dev["value_device_resident"] == dev["value"]
    a, b = outs[0][1], outs[1][1]
    assert sorted(a) == sorted(b) and all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    n = len(a["read_index"])
    assert n == 16384 and len(a["status"]) == n and len(a["aln_begin"]) == n + 1 and (a["status"] == 0).all()
    assert len(a["aln_score"]) == a["aln_begin"][-1] > 0.5 * n and len(a["nodes"]) == a["aln_n_nodes"].sum()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the sampled reads again, generated from the same seeds as bench.py does, through the oracle: every field of every alignment
    import ctypes as C
    import orc
    import torch
    from metagraph_amd import capi, synth
    dev = torch.device("cuda", 0)
    genome = synth.random_genome(300000, 20240501, dev)
    boss = synth.build_boss([genome[None, :], synth.snp_windows(genome, 600, 31, 20240502)], 31)
    reads = synth.sample_reads(genome, 30000, 150, 20240503).cpu().numpy()
    W, last = boss["W"].cpu().numpy(), boss["last"].cpu().numpy()
    view = capi.BossView()
    view.k, view.sigma, view.n_edges, view.mode, view.on_device = 31, 5, boss["n_edges"], 0, 0
    view.W, view.last = W.ctypes.data, last.ctypes.data
    Fc = (C.c_uint64 * 5)(*[int(x) for x in boss["F"]])
    view.F = C.cast(Fc, C.POINTER(C.c_uint64))
    og = orc.Graph(orc.L().orc_graph_from_boss(C.byref(view)))
    want = orc.AlignRun(og, capi.config_cli(31), [bytes(reads[i]) for i in a["read_index"].astype(np.int64)], validate=False).results()
    got, nb, cb, sb = [], 0, 0, 0
    for q in range(n):
        alns = []
        for j in range(int(a["aln_begin"][q]), int(a["aln_begin"][q + 1])):
            nn, nc, ns = int(a["aln_n_nodes"][j]), int(a["aln_n_cigar"][j]), int(a["aln_seq_len"][j])
            d = {f: int(a["aln_" + f][j]) for f in ("score", "offset", "clipping", "end_clipping", "num_matches", "orientation")}
            d["nodes"] = [int(x) for x in a["nodes"][nb:nb + nn]]
            d["cigar"] = "".join("%d%s" % (int(ln), capi.OP_CHARS[int(op)]) for ln, op in zip(a["cigar_len"][cb:cb + nc], a["cigar_op"][cb:cb + nc]))
            d["sequence"] = bytes(a["seqs"][sb:sb + ns].astype(np.uint8)).decode()
            nb, cb, sb = nb + nn, cb + nc, sb + ns
            alns.append(d)
        got.append(alns)
    assert got == want
