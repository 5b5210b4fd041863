"""The mapping kernels (k_map_packed: map_pipe=0; k_map_pipe: map_pipe=2; the byte path k_map: k > 32) and the device index
they walk, through mgx_graph_create + mgx_map_batch, against a plain k-mer dictionary (tests/kmer_dict.py, pinned to the
oracle by tests/test_kmer_dict.py) at the sizes and edges no other test reaches: every residue of the edge count that the
last-block clips depend on, single-block graphs, read lengths and invalid characters around the 32-base words of the packed
reads, graphs large enough for select-anchor shifts 7 and 8, and the node arrays of PRIMARY graphs.  Every comparison is
exact equality of node arrays.  Needs a real MI355X."""
import ctypes as C

import pytest

import map_index_worlds as worlds
from map_index_worlds import BYTE_PATH_KS, K_BIG, MACHINES
from metagraph_amd import aligner, capi

pytestmark = pytest.mark.gpu


class Gpu:
    """mgx_graph_create + mgx_map_batch"""

    @staticmethod
    def graph(k, W, last, F, valid=None, mode=0):
        return aligner.Graph(k, W, last, F, valid, mode=mode)

    @staticmethod
    def check(G, k, reads, want, machine, forward_only=True):
        """map_batch (both strands) and, for BASIC graphs, the forward-only launch of the same kernels (mgx_map_summary_batch
        with the node arrays: do_rc = 0) equal the dictionary's arrays"""
        A = aligner.Aligner(G, capi.config_cli(k))
        if machine in MACHINES:
            A.set_pipeline(machine)
        got = A.map_batch(reads)
        assert got == want, worlds.first_difference(got, want, reads)
        if forward_only:
            _, nodes = A.map_summary(reads, want_nodes=True)
            fwd = [f for f, _ in want]
            assert nodes == fwd, worlds.first_difference([(n, []) for n in nodes], [(f, []) for f in fwd], reads)


@pytest.mark.parametrize("residue", [0, 1, 2, 63])
@pytest.mark.parametrize("k", [3, 11, 31] + BYTE_PATH_KS)
def test_edge_count_residues(k, residue):
    """(n_edges + 1) mod 64 = 0 (the final block exactly full), 1 (one slot in it), 2 and 63: the clips of the last block in
    incoming / succ_W_code, mask_upto, the `i > n` cut of the block build, the valid and first-character packers"""
    worlds.edge_count_residues(Gpu, k, residue)


@pytest.mark.parametrize("full", [False, True], ids=["ragged", "exactly-full"])
@pytest.mark.parametrize("k", [3, 11, 31, 33, 40])
def test_single_block_graphs(k, full):
    """one 64-byte block is the whole index: n_edges < 64, and n_edges + 1 == 64 exactly.  (k = 63 has no such graph: the
    root edge, the 62 sentinel-prefixed edges in front of a sequence's first k-mer, one k-mer and its sink are 65 edges.)"""
    worlds.single_block_graphs(Gpu, k, full)


@pytest.mark.parametrize("k", [3, 31, 32] + BYTE_PATH_KS)
def test_read_lengths_and_invalid_characters_at_word_edges(k):
    """pack_read_word, packed_advance and kmask: one read of every length 0 .. 130, alone and with one N / lower-case /
    non-ACGT byte at 0, k - 1, 31, 32, 63, 64, 95, 96, L - k and L - 1, both strands and forward only; in one batch and in
    batches of 1, 63, 64, 65 and 257 reads (a lane's chain fetch crosses wavefront and workgroup edges).  k = 33, 40, 63: the
    byte path, as the control."""
    worlds.read_lengths_and_invalid_characters_at_word_edges(Gpu, k)


@pytest.mark.parametrize("machine", MACHINES)
def test_select_anchor_shift_7(machine):
    total_last = worlds.check_big(Gpu, "shift7", machine, 7)
    assert 8191 * 64 <= total_last < 8191 * 128


@pytest.mark.parametrize("machine", MACHINES)
def test_select_anchor_shift_8(machine):
    total_last = worlds.check_big(Gpu, "shift8", machine, 8)
    assert 8191 * 128 <= total_last < 8191 * 256


@pytest.mark.parametrize("machine", MACHINES)
def test_select_anchor_with_an_empty_last_segment(machine):
    total_last = worlds.check_big(Gpu, "span0", machine, 7)
    assert total_last % 128 == 0


def test_alignment_on_the_shift_7_graph_through_the_lane_kernels():
    """lane_read.hpp predicts the select of its children from the same anchors (global memory): one alignment batch on the
    shift-7 graph under the lane-per-read kernel options of the parity suite, against the host model"""
    import emu_drv
    (W, last, F), text, reads, _ = worlds.big_world("shift7")
    assert worlds.sel_anchor_shift(int(last[1:].sum())) == 7
    reads = reads[:260] + reads[4000:4020] + reads[4200:4220]
    assert len(reads) == 300
    cfg = capi.config_cli(K_BIG)
    e = emu_drv.EmuRun(emu_drv.EmuGraph(worlds.ArrayGraph(K_BIG, W, last, F)), cfg, reads)
    assert e.error == "", e.error
    want, status = e.results()
    assert all(s == 0 for s in status)

    def lane_launches():
        out = (C.c_uint64 * 5)()
        capi.lib().mgx_kernel_launch_counts(out)           # grp8, grp8_prim, grp8_alt, ext64, lane
        return int(out[4])

    before = lane_launches()
    A = aligner.Aligner(aligner.Graph(K_BIG, W, last, F), cfg)
    for opt in ("ext64=0", "lane=1", "groups_per_wave=0", "map_pipe=2", "seed_lane=1"):       # the "lane" variant of tests/conftest.py
        A.set_pipeline(opt)
    got, status = A.align_batch(reads)
    assert all(s == 0 for s in status), status
    for q in range(len(reads)):
        assert got[q] == want[q], (q, reads[q], got[q], want[q])
    assert sum(1 for a in got if a) > 250
    assert lane_launches() > before, "k_lane never ran"
    assert A.stats()["n_lane_reads"] > 0


@pytest.mark.parametrize("k,mask", [(12, False), (12, True), (31, False), (40, False)])
def test_primary_node_arrays(k, mask):
    """canon_merge_pair: a k-mer found forward keeps its id, its mirror image is id + n unless the k-mer is a palindrome
    (even k); one found only as reverse complement is id + n forward.  Even k: palindromic k-mers are planted in the genome
    and read on both strands."""
    worlds.primary_node_arrays(Gpu, k, mask)
