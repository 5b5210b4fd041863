"""Per-branch x-drop (DBGAlignerConfig::global_xdrop = 0: a cut-off per branch of a fork, the node limit per branch,
scores_reached_) of label-aware aligners in the kernels' wave program under the host model, against the oracle's LabeledAligner
under the same setting.  CPU only; the GPU half is tests/test_gpu_branch_xdrop.py."""
import pytest

import emu_drv
import orc
from metagraph_amd import capi
from labeled_worlds import labeled_world, with_labels
from test_labeled_emu import compare_emu_labeled
from test_oracle_labeled import CASES, build

N_WORLDS = 20          # worlds of the precondition
# worlds (from the front) the host model runs under every configuration: all of them (a configuration takes about a second)
N_EMU_WORLDS = 20


def world(seed):
    k = [11, 15, 21][seed % 3]
    return (k,) + labeled_world(seed, k, n_strains=5, n_reads=24, divergence=0.05, genome_len=1200)


def configure(name, k, global_xdrop):
    cfg = capi.config_cli(k)
    if name == "rel0.5":
        cfg.rel_score_cutoff = 0.5
    elif name == "xdrop10":
        cfg.xdrop = 10
    elif name == "nodes0.5":
        cfg.max_nodes_per_seq_char = 0.5
    elif name == "ram0.01":
        cfg.max_ram_per_alignment = 0.01
    elif name == "alt2sub":
        cfg.num_alternative_paths = 2
        cfg.min_seed_length = 9
    else:
        assert name == "cli"
    cfg.global_xdrop = global_xdrop
    return cfg


CONFIGS = ["cli", "rel0.5", "xdrop10", "nodes0.5", "ram0.01", "alt2sub"]
_worlds = {}


def cached_world(seed):
    if seed not in _worlds:
        _worlds[seed] = world(seed)
    return _worlds[seed]


@pytest.mark.parametrize("name,at_least", [("rel0.5", 40), ("cli", 3), ("xdrop10", 4), ("nodes0.5", 1)])
def test_the_worlds_meet_the_feature(name, at_least):
    """the oracle alone: the two modes differ on these worlds, so the comparisons below run on inputs that meet the feature"""
    differ = 0
    for seed in range(N_WORLDS):
        k, g, anno, reads = cached_world(seed)
        res = []
        for gx in (1, 0):
            o = orc.LabeledAlignRun(g, configure(name, k, gx), anno, reads)
            assert o.error == "", o.error
            res.append(with_labels(o))
        differ += sum(1 for a, b in zip(*res) if a != b)
    print(name, "reads that differ between global_xdrop = 1 and 0:", differ)
    assert differ >= at_least, (name, differ)


@pytest.mark.parametrize("name", CONFIGS)
def test_host_model_against_the_oracle(name, monkeypatch):
    if name == "xdrop10":
        monkeypatch.setenv("MGX_EMU_SPLIT", "1")           # seeding phase, sort, extension phase (the device's pipeline)
    for seed in range(N_EMU_WORLDS):
        k, g, anno, reads = cached_world(seed)
        compare_emu_labeled(g, anno, configure(name, k, 0), reads)


@pytest.mark.parametrize("name", ["cli", "rel0.5"])
def test_host_model_general_path_only(name, monkeypatch):
    """every column through general_step (the `general` pipeline option): the chain path and the general path hold the same rule"""
    monkeypatch.setenv("MGX_NO_FAST", "1")
    for seed in range(4):
        k, g, anno, reads = cached_world(seed)
        compare_emu_labeled(g, anno, configure(name, k, 0), reads)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_label_kats_per_branch(name):
    """the reference's label tests (BASIC, CANONICAL and PRIMARY graphs) with global_xdrop = 0: the oracle under the same setting is
    the expectation, not the KAT's strings"""
    case = CASES[name]
    g, anno, cfg = build(case)
    cfg.global_xdrop = 0
    for query in case["expect"]:
        compare_emu_labeled(g, anno, cfg, [query], validate=not (cfg.left_end_bonus or cfg.right_end_bonus), mode=case["mode"])


def test_a_plain_aligner_still_refuses_it():
    k, g, anno, reads = cached_world(0)
    e = emu_drv.EmuRun(emu_drv.EmuGraph(g), configure("cli", k, 0), reads[:1])
    assert "global_xdrop" in e.error, e.error
