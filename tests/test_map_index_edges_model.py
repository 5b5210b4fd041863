"""The worlds of tests/test_gpu_map_index_edges.py (edge-count residues, single-block graphs, read lengths and invalid
characters at the word edges of the packed reads, PRIMARY node arrays) through the host model of the mapping kernels instead
of the GPU: the same sources (graph_build.hpp, map_pipe.hpp, dev_graph.hpp) under tests/emu/wave.hpp, against the same plain
k-mer dictionary.  What this catches needs no GPU to be found; the kernels as compiled for the device, their launch
geometry and mgx_graph_create's own sizing are the GPU file's.  CPU only."""
import os

import numpy as np
import pytest

import emu_drv
import map_index_worlds as worlds
from metagraph_amd import capi


class ModelGraph:
    def __init__(self, k, W, last, F, valid=None, mode=0):
        self.k, self.mode = k, mode
        self.arrays = (np.ascontiguousarray(W, dtype=np.uint8), np.ascontiguousarray(last, dtype=np.uint8),
                       np.asarray([int(x) for x in F], dtype=np.uint64), None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8))

    def export(self):
        return self.arrays


class Model:
    graph = ModelGraph

    @staticmethod
    def check(G, k, reads, want, machine, forward_only=True):
        """machine "map_pipe=0": the model of k_map_packed (map_lane_step_packed; the driver's MGX_MAP_LANES switch);
        "map_pipe=2": that of k_map_pipe (map_pipe_step); k > 32: the byte path (map_lane_step)"""
        old = os.environ.pop("MGX_MAP_LANES", None)
        if machine == "map_pipe=0":
            os.environ["MGX_MAP_LANES"] = "1"
        try:
            got = emu_drv.EmuRun(emu_drv.EmuGraph(G, mode=G.mode), capi.config_cli(k), reads, map_only=True).mapping()
        finally:
            os.environ.pop("MGX_MAP_LANES", None)
            if old is not None:
                os.environ["MGX_MAP_LANES"] = old
        assert got == want, worlds.first_difference(got, want, reads)


@pytest.mark.parametrize("residue", [0, 1, 2, 63])
@pytest.mark.parametrize("k", [3, 31, 33, 40, 63])
def test_edge_count_residues(k, residue):
    worlds.edge_count_residues(Model, k, residue)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("k", [3, 31, 33, 40])
def test_single_block_graphs(k, full):
    worlds.single_block_graphs(Model, k, full)


@pytest.mark.parametrize("k", [3, 31, 32, 33, 40, 63])
def test_read_lengths_and_invalid_characters_at_word_edges(k):
    worlds.read_lengths_and_invalid_characters_at_word_edges(Model, k)


@pytest.mark.parametrize("k,mask", [(12, False), (12, True), (31, False), (40, False)])
def test_primary_node_arrays(k, mask):
    worlds.primary_node_arrays(Model, k, mask)
