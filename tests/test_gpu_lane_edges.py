"""The lane-per-read extender on the GPU (mgx_lane.hip, extend_by_lanes in mgx.hip) at its hand-over reasons, limits and batch
shapes: the directed worlds of tests/lane_cases.py, whose per-read fates tests/test_lane_edges.py pins in the host model.  Per
case: every read against the oracle, and the kernel's histogram of hand-over reasons against the case's, key for key — the
one-atomic prefix sum of output words, the bail list, the histogram loop over a wavefront's distinct reasons are all in the way of
those numbers.  Then what no other GPU test reaches below a hundred thousand reads: one wavefront that takes several reads per
lane, and one handle whose scratch layout changes from batch to batch."""
import collections

import pytest

import lane_cases as lc
import orc
from labeled_worlds import with_labels
from metagraph_amd import aligner, capi
from test_gpu_parity import gpu_graph

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle(name):
    """the oracle's results of a case (run once per module)"""
    if name not in _oracle:
        c = lc.CASES[name]()
        if c.annotation is not None:
            o = orc.LabeledAlignRun(c.graph, c.config, c.annotation, c.reads, validate=False)
            assert o.error == "", o.error
            _oracle[name] = with_labels(o)
        else:
            o = orc.AlignRun(c.graph, c.config, c.reads, threads=8, validate=False)
            assert o.error == "", o.error
            _oracle[name] = o.results()
    return _oracle[name]


def histogram(expected):
    return {k: v for k, v in collections.Counter(expected).items() if k}


def handle(c, lane=1):
    an = None
    if c.annotation is not None:
        an = aligner.Annotation(c.graph.n_edges, [c.annotation.column_words(j) for j in range(c.annotation.n_labels)])
    A = aligner.Aligner(gpu_graph(c.graph), c.config, c.limits, annotation=an)
    A.set_pipeline("lane=%d" % lane)
    # (a batch with 24 seeds or more per read takes the multi-pass extension of its own accord, which has no lane kernel in front:
    # the cases with one seed per k-mer are such batches)
    A.set_pipeline("multi_pass=0")
    return A


def check_batch(A, reads, want, expected):
    """one batch through handle A against the oracle's results and the expected fates -> (results, the lane's statistics)"""
    got, status = A.align_batch(reads)
    assert all(s == 0 for s in status), status
    st = A.stats()
    for q in range(len(reads)):
        assert got[q] == want[q], (q, reads[q], got[q], want[q])
    assert st["extend_kernels"] & capi.KERNEL_LANE
    assert st["lane_bail_reads"] == histogram(expected), (st["lane_bail_reads"], histogram(expected))
    assert st["n_lane_reads"] + sum(st["lane_bail_reads"].values()) == len(reads)
    return got, (st["n_lane_reads"], st["lane_bail_reads"])


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case(name):
    c = lc.CASES[name]()
    want = oracle(name)
    A = handle(c)
    # (a read that left on a capacity guard meets the same limit in the group kernel: the batch's capacity retry aligns it, and the
    # statistics are the batch's own)
    got, _ = check_batch(A, c.reads, want, c.expected)
    A.set_pipeline("lane=0")
    got0, status0 = A.align_batch(c.reads)
    st0 = A.stats()
    assert all(s == 0 for s in status0) and got0 == got
    assert st0["n_lane_reads"] == 0 and not st0["lane_bail_reads"] and not (st0["extend_kernels"] & capi.KERNEL_LANE)


def test_one_wavefront_takes_many_reads(monkeypatch):
    """64 x 5 + 37 reads through ONE wavefront (MGX_LANE_BLOCKS_PCT=1 of ceil(n / 64) = 6): the persistent loop of k_lane, a lane's
    node table under the next read's tag, lanes that hold a read for its backward pass while their wave-mates fetch new ones —
    finishing reads, reads with a backward pass and six hand-over codes, interleaved"""
    name = "shape_%d" % lc.ONE_WAVEFRONT_READS
    c = lc.CASES[name]()
    assert len(c.reads) == lc.ONE_WAVEFRONT_READS and len(histogram(c.expected)) >= 4
    want = oracle(name)
    plain = check_batch(handle(c), c.reads, want, c.expected)
    # (extend_by_lanes: blocks = max(1, min(resident wavefronts, ceil(n / 64)) * pct / 100); nothing in the statistics tells how
    # many were launched: the test rests on that line)
    assert max(1, min(2048, -(-len(c.reads) // 64)) * 1 // 100) == 1
    monkeypatch.setenv("MGX_LANE_BLOCKS_PCT", "1")
    A = handle(c)
    one = check_batch(A, c.reads, want, c.expected)
    assert one == plain
    assert check_batch(A, c.reads, want, c.expected) == plain            # ... and again: every table entry of the first launch is stale


def test_one_handle_batches_whose_layout_changes():
    """250-bp reads, 100-bp reads, and both again through one handle: max_cols, hash_slots, rest_stride and wave_stride follow the
    batch's longest read, and the scratch is zeroed only when it grows — the second batch's node tables lie over what were column
    slots and S rows, the third's slots over node tables.  By design that is harmless: a foreign word reads as a free entry unless
    its upper 20 bits are the read's tag, and a false hit is caught by the slot's node word.  A false hit that changes a read's
    fate needs a 20-bit tag and a 32-bit node to coincide: over these few hundred reads the expected number is far below one, so
    the statistics are compared exactly."""
    names = ["layout_250", "layout_100"]
    cases = [lc.CASES[n]() for n in names]
    # (lane_types.hpp: max_cols = Lmax + min(Lmax, xdrop) + 8 with Lmax rounded up to 8, hash_slots = the power of two >= twice that)
    cols = [((max(len(r) for r in c.reads) + 7) & ~7) + 27 + 8 for c in cases]
    assert cols == [291, 139] and [1 << (2 * x - 1).bit_length() for x in cols] == [1024, 512]
    A = handle(cases[0])
    outs = []
    for x in (0, 1, 0, 1):
        outs.append(check_batch(A, cases[x].reads, oracle(names[x]), cases[x].expected))
    assert outs[2] == outs[0] and outs[3] == outs[1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_shapes(n):
    """all leave, none leave, n mixed, then the first again through one handle: results and statistics of the fourth call equal
    those of the first (cursors, bail list and histogram start afresh per batch)"""
    names = ["shape_all_leave", "shape_none_leave", "shape_%d" % n]
    cases = [lc.CASES[x]() for x in names]
    A = handle(cases[0])
    first = None
    for x in (0, 1, 2, 0):
        out = check_batch(A, cases[x].reads, oracle(names[x]), cases[x].expected)
        if first is None:
            first = out
    assert out == first
