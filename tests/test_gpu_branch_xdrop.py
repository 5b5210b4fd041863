"""Per-branch x-drop (DBGAlignerConfig::global_xdrop = 0) of label-aware aligners on the GPU: the builds of the two label-aware
extension kernels with MGX_BRANCH_XDROP (mgx_lab64.hip, mgx_grp.hip) against the oracle's LabeledAligner under the same setting,
through the C-ABI: full alignment lists and label lists.  The CPU half (host model, and the proof that the worlds meet the feature)
is tests/test_branch_xdrop_emu.py.  Needs a real MI355X."""
import ctypes as C

import pytest

import orc
from metagraph_amd import aligner, capi
from labeled_worlds import labeled_world, with_labels
from test_branch_xdrop_emu import CONFIGS, cached_world, configure
from test_gpu_labels import gpu_annotation
from test_gpu_parity import gpu_graph
from test_oracle_labeled import CASES, build

pytestmark = pytest.mark.gpu

N_WORLDS = 20
# what an aligner with global_xdrop = 0 launches: "ext64=2" / "ext64=0" force the 64-lane or the 8-lane build
KERNELS = {"lab64_bx": ("ext64=2", capi.KERNEL_LAB64_BX), "grp8_lab_bx": ("ext64=0", capi.KERNEL_GRP8_LAB_BX)}
_oracle = {}


def oracle_results(name, seed):
    """the oracle's results of world `seed` under configuration `name` with global_xdrop = 0: computed once, shared, never changed"""
    if (name, seed) not in _oracle:
        k, g, anno, reads = cached_world(seed)
        o = orc.LabeledAlignRun(g, configure(name, k, 0), anno, reads)
        assert o.error == "", o.error
        _oracle[name, seed] = with_labels(o)
    return _oracle[name, seed]


_device = {}


def device_world(seed):
    if seed not in _device:
        k, g, anno, reads = cached_world(seed)
        _device[seed] = (gpu_graph(g), gpu_annotation(anno))
    return _device[seed]


def run_world(name, seed, kernel, options=(), limits=None):
    k, g, anno, reads = cached_world(seed)
    G, AN = device_world(seed)
    A = aligner.Aligner(G, configure(name, k, 0), limits=limits, annotation=AN)
    A.set_pipeline(KERNELS[kernel][0])
    for opt in options:
        A.set_pipeline(opt)
    got, status = A.align_batch(reads)
    assert all(s == 0 for s in status), status
    want = oracle_results(name, seed)
    for q in range(len(reads)):
        assert got[q] == want[q], (seed, q, reads[q], got[q], want[q])
    st = A.stats()
    assert st["extend_kernels"] == KERNELS[kernel][1], st["extend_kernels"]      # the per-branch build asked for is the one that ran
    assert st["n_lane_reads"] == 0 and st["n_lane_exact_reads"] == 0 and st["n_lane_exact_path_reads"] == 0, st
    return st


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", CONFIGS)
def test_worlds_against_the_oracle(name, kernel):
    for seed in range(N_WORLDS):
        run_world(name, seed, kernel)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("pipeline", ["general", "chain"])
@pytest.mark.parametrize("name", ["cli", "rel0.5"])
def test_general_and_chain_path(name, pipeline, kernel):
    n_fast = 0
    for seed in range(N_WORLDS):
        n_fast += run_world(name, seed, kernel, options=(pipeline,))["n_fast_columns"]
    assert (n_fast == 0) == (pipeline == "general"), n_fast


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_lane_kernels_stay_out(kernel):
    """lane=1, exact=2 mean "where the configuration allows it": per-branch x-drop does not (the lane kernels encode the global rule)"""
    for seed in range(N_WORLDS):
        run_world("cli", seed, kernel, options=("lane=1", "exact=2", "seed_lane=1"))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_label_kats_per_branch_on_gpu(name, kernel):
    """every graph mode (BASIC, CANONICAL, PRIMARY); the oracle under global_xdrop = 0 is the expectation, not the KAT's strings"""
    case = CASES[name]
    g, anno, cfg = build(case)
    cfg.global_xdrop = 0
    if case["mode"]:
        W, last, F, valid = g.export()
        G = aligner.Graph(g.k, W, last, F, valid, mode=case["mode"])
    else:
        G = gpu_graph(g)
    AN = gpu_annotation(anno)
    for query in case["expect"]:
        o = orc.LabeledAlignRun(g, cfg, anno, [query], validate=not (cfg.left_end_bonus or cfg.right_end_bonus))
        assert o.error == "", o.error
        A = aligner.Aligner(G, cfg, annotation=AN)
        A.set_pipeline(KERNELS[kernel][0])
        got, status = A.align_batch([query])
        assert status == [0], status
        assert got == with_labels(o), (query, got)
        assert A.stats()["extend_kernels"] == KERNELS[kernel][1]


def test_c_abi_accepts_it_for_label_aware_aligners_only():
    k, g, anno, reads = cached_world(0)
    G, AN = device_world(0)
    cfg = configure("cli", k, 0)
    with pytest.raises(aligner.MgxError) as e:              # a plain aligner: refused, as the reference's DBGAligner throws
        aligner.Aligner(G, cfg)
    assert e.value.code == capi.MGX_ERR_UNSUPPORTED and "global_xdrop" in str(e.value), str(e.value)
    A = aligner.Aligner(G, cfg, annotation=AN)
    assert A.get_config().global_xdrop == 0
    # the same annotation and graph under the global rule launch what they launched before
    for opt, bit in (("ext64=2", capi.KERNEL_LAB64), ("ext64=0", capi.KERNEL_GRP8_LAB)):
        B = aligner.Aligner(G, configure("cli", k, 1), annotation=AN)
        assert B.get_config().global_xdrop == 1
        B.set_pipeline(opt)
        got, status = B.align_batch(reads)
        assert all(s == 0 for s in status), status
        o = orc.LabeledAlignRun(g, configure("cli", k, 1), anno, reads)
        assert got == with_labels(o)
        assert B.stats()["extend_kernels"] == bit, B.stats()["extend_kernels"]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_capacity_retry_under_a_small_column_limit(kernel):
    """max_nodes_per_seq_char bounds a branch's depth under the per-branch rule, not the table: a table that outgrows max_columns is a
    capacity status, and the retry with doubled limits gives the oracle's results"""
    retried = 0
    for seed in (0, 1, 2):
        k = [11, 15, 21][seed % 3]
        g, anno, reads = labeled_world(seed, k, n_strains=5, n_reads=24, divergence=0.05, genome_len=1200, read_len=150)
        cfg = configure("cli", k, 0)
        o = orc.LabeledAlignRun(g, cfg, anno, reads)
        assert o.error == "", o.error
        lim = capi.Limits()
        lim.max_columns = 128
        A = aligner.Aligner(gpu_graph(g), cfg, limits=lim, annotation=gpu_annotation(anno))
        A.set_pipeline(KERNELS[kernel][0])
        got, status = A.align_batch(reads)
        assert all(s == 0 for s in status), status
        assert got == with_labels(o)
        retried += A.stats()["n_capacity_retried"]
    assert retried > 0
