"""extend_multi_pass (mgx.hip) on the device at every step of its seed limit, through the C-ABI: the worlds of
tests/multi_pass_worlds.py with the oracle's alignment lists as the expectation, no read left out.

tests/test_multi_pass_emu.py pins the worlds' extension counts and runs the host model's copy of the loop; what exists on the
device only is here: the host loop itself (two resume pools and two retry lists swapped, the 12-bit radix re-sort, cursors
cleared, the retry count clamped to the capacity), retry positions in the order the wavefronts reach the atomic, resumed reads
in arena slots whose generation-tagged tables belong to another read, fewer resume records than retrying reads (the option
resume_cap), and the three kernels the passes run on.  The number of passes is asserted through the launch counters: it follows
from the schedule (multi_pass_seed_limit: 1, 4, 16, none at pass 24) and the worlds' preconditions, it is not measured."""
import ctypes as C
import random

import pytest

import multi_pass_worlds as mpw
import orc
import test_gpu_format_batch as fb
import test_multi_pass_emu as cpu
from metagraph_amd import aligner, capi

pytestmark = pytest.mark.gpu

# the three kernel choices, spelled as conftest.py's variants spell them (the passes run no lane kernel in front)
KERNELS = {
    "ext64": ("ext64=1", "lane=0", "groups_per_wave=1"),           # one read per wavefront: the 64-lane kernel
    "grp8": ("ext64=0", "lane=0"),                                 # 8-lane groups, reads spread over wavefronts
    "grp8x8": ("ext64=0", "lane=0", "groups_per_wave=0"),          # ... 8 reads per wavefront
}
GRP8_BITS = capi.KERNEL_GRP8 | capi.KERNEL_GRP8_PRIM | capi.KERNEL_GRP8_ALT

_graphs = {}


def gpu_graph(w, cached=True):
    if cached and w.name in _graphs:
        return _graphs[w.name]
    W, last, F, valid = w.g.export()
    G = aligner.Graph(w.k, W, last, F, valid, mode=w.mode)
    if cached:
        _graphs[w.name] = G
    return G


def handle(w, n_alt=1, opts=(), limits=None, graph=None):
    A = aligner.Aligner(graph or gpu_graph(w), w.config(n_alt), limits if limits is not None else mpw.alt_limits(n_alt))
    for o in opts:
        A.set_pipeline(o)
    return A


def ext_launches():
    """launches of the extension kernels (8-lane groups, its _prim and _alt builds, the 64-lane kernel) since the library was loaded"""
    out = (C.c_uint64 * 5)()
    capi.lib().mgx_kernel_launch_counts(out)
    return sum(out[:4])


def run(A, reads, want=None):
    """one batch -> (results, stats, extension launches); every status 0, and with `want` every read against it"""
    before = ext_launches()
    got, status = A.align_batch(reads)
    launches = ext_launches() - before
    assert all(s == 0 for s in status), status
    if want is not None:
        for q in range(len(reads)):
            assert got[q] == want[q], (q, reads[q], got[q], want[q])
    return got, A.stats(), launches


def check_kernel(kernel, st, build_bit=0):
    if kernel == "ext64":
        assert st["extend_kernels"] & capi.KERNEL_EXT64 and not (st["extend_kernels"] & GRP8_BITS), st["extend_kernels"]
    else:
        assert st["extend_kernels"] & GRP8_BITS and not (st["extend_kernels"] & capi.KERNEL_EXT64), st["extend_kernels"]
        if build_bit:
            assert st["extend_kernels"] & GRP8_BITS == build_bit, st["extend_kernels"]


# ---- forced, every build -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_alt", [1, 2, 4])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_forced_deep(kernel, n_alt):
    """deep, and deep_alt (num_alternative_paths 2 and 4: a resume record carries up to four alignments, the _alt build)"""
    w = mpw.deep()
    A = handle(w, n_alt, KERNELS[kernel] + ("multi_pass=1",))
    _, st, launches = run(A, w.reads, mpw.oracle("deep", n_alt))
    check_kernel(kernel, st, capi.KERNEL_GRP8 if n_alt == 1 else capi.KERNEL_GRP8_ALT)
    # (a handle's first batch may redo the whole stage with larger buffers: whole multiples of the 25 passes)
    assert launches >= mpw.N_PASSES_DEEP and launches % mpw.N_PASSES_DEEP == 0
    if kernel == "grp8" and n_alt == 1:
        # text after passes: the staged batch is still the one the text kernels read
        headers = ["read%d" % i for i in range(len(w.reads))]
        fb.align_host(A, w.reads)
        fb.check_batch(A, headers, w.reads)


@pytest.mark.parametrize("tables", ["tables", "no-tables"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_forced_deep_primary(kernel, tables, monkeypatch):
    """the PRIMARY graph of deep's genome, every other read reverse-complemented: the _prim build, in both ways the device walks
    the wrapper (reverse-complement tables built at load time; MGX_PRIMARY_TABLES=0: re-derived per expansion)"""
    if tables == "no-tables":
        monkeypatch.setenv("MGX_PRIMARY_TABLES", "0")
    else:
        monkeypatch.delenv("MGX_PRIMARY_TABLES", raising=False)
    w = mpw.deep_primary()
    A = handle(w, 1, KERNELS[kernel] + ("multi_pass=1",), graph=gpu_graph(w, cached=False))
    _, st, launches = run(A, w.reads, mpw.oracle("deep_primary"))
    check_kernel(kernel, st, capi.KERNEL_GRP8_PRIM)
    assert launches >= mpw.N_PASSES_DEEP and launches % mpw.N_PASSES_DEEP == 0


# ---- the passes ran, and did the same work ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["ext64", "grp8"])
def test_the_passes_ran(kernel):
    """extend_multi_pass launches the extension kernel exactly once per pass (one launch_extension call in the body of its loop)
    and run_align exactly once under multi_pass=0, so the launches of deep are 25 times those of the one-pass run: passes
    0 .. 24, because deep has reads with live seeds left when the unlimited pass starts (test_multi_pass_emu.py::test_pass_counts)
    and no batch runs more.  A schedule of 1 throughout would go on for hundreds of passes.  The counters that travel in the
    resume record are the one-pass run's."""
    w = mpw.deep()
    want = mpw.oracle("deep")
    A = handle(w, 1, KERNELS[kernel] + ("multi_pass=0",))
    run(A, w.reads, want)                   # (a first batch may redo a stage whose buffers it found too small)
    _, st0, one = run(A, w.reads, want)
    assert one == 1
    A.set_pipeline("multi_pass=1")
    _, st1, many = run(A, w.reads, want)
    print("launches of deep: multi_pass=0 %d, multi_pass=1 %d" % (one, many))
    assert many == mpw.N_PASSES_DEEP * one
    for key in ("n_extensions", "n_columns", "n_fast_columns", "n_seeds"):
        assert st1[key] == st0[key] and st0[key] > 0, (key, st0[key], st1[key])
    s = mpw.shallow()
    B = handle(s, 1, KERNELS[kernel] + ("multi_pass=0",))
    run(B, s.reads, mpw.oracle("shallow"))
    _, sst0, one = run(B, s.reads, mpw.oracle("shallow"))
    B.set_pipeline("multi_pass=1")
    _, sst1, few = run(B, s.reads, mpw.oracle("shallow"))
    assert one == 1 and 1 <= few <= 2 * one
    for key in ("n_extensions", "n_columns", "n_fast_columns", "n_seeds"):
        assert sst1[key] == sst0[key], (key, sst0[key], sst1[key])


# ---- order independence ----------------------------------------------------------------------------------------------------------

def test_permuted_and_repeated_batches():
    """Three fixed permutations of deep, and deep three times on one handle: retry positions come in the order the wavefronts
    reach the atomic and a resumed read lands in the arena slot of whichever group fetches it — per-read results never differ."""
    w = mpw.deep()
    want = mpw.oracle("deep")
    A = handle(w, 1, KERNELS["grp8"] + ("multi_pass=1",))
    first = None
    for x in range(3):
        got, st, launches = run(A, w.reads, want)
        assert launches == mpw.N_PASSES_DEEP or x == 0          # (a handle's first batch may redo the stage with larger buffers)
        counters = [st[k] for k in ("n_extensions", "n_columns", "n_fast_columns")]
        assert first is None or (got, counters) == first
        first = (got, counters)
    n = len(w.reads)
    for seed in (1, 2, 3):
        perm = list(range(n))
        random.Random(seed).shuffle(perm)
        got, st, _ = run(A, [w.reads[i] for i in perm], [want[i] for i in perm])
        assert [st[k] for k in ("n_extensions", "n_columns", "n_fast_columns")] == first[1]


def test_3000_reads_through_fewer_groups():
    """deep tiled to 3000 reads, each compared with the oracle's result of the read it copies.  3000 reads alone would all be
    resident at once (one group per read up to the machine's 24 576): device_share=32 gives the handle 1 / 32 of the groups, a
    quarter of the batch, so that every group takes several work items per pass — retry positions come from several waves of items, and a resumed read
    finds the tables of the group's earlier reads in its slot."""
    w = mpw.deep()
    want = mpw.oracle("deep")
    n = len(w.reads)
    reads = [w.reads[i % n] for i in range(3000)]
    A = handle(w, 1, KERNELS["grp8"] + ("multi_pass=1", "device_share=32"))
    run(A, w.reads, want)                    # (the handle's buffers take the scale of the batch's seeds per read)
    got, st, launches = run(A, reads)
    assert launches == mpw.N_PASSES_DEEP
    for q in range(len(reads)):
        assert got[q] == want[q % n], (q, q % n)
    B = handle(w, 1, KERNELS["grp8"] + ("multi_pass=0",))
    _, st0, _ = run(B, w.reads, want)
    full, rest = divmod(len(reads), n)
    assert rest == 3000 - 36 * n
    C_rest = handle(w, 1, KERNELS["grp8"] + ("multi_pass=0",))
    _, st_rest, _ = run(C_rest, w.reads[:rest], want[:rest])
    for key in ("n_extensions", "n_columns", "n_fast_columns"):
        assert st[key] == full * st0[key] + st_rest[key], key


# ---- fewer records than retrying reads ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["ext64", "grp8"])
def test_fewer_resume_records_than_retrying_reads(kernel):
    """resume_cap = 2, 1, and one below the number of reads that want another pass after pass 0 (the host model's pass log): a
    read whose retry position is at or beyond the capacity goes on without a limit in the same launch, and the host clamps the
    count of the next pass to the capacity"""
    w = mpw.deep()
    want = mpw.oracle("deep")
    retried = cpu.retried_after_pass_0()
    print("reads of deep that retry after pass 0: %d" % retried)
    assert 3 < retried <= len(w.reads)
    A = handle(w, 1, KERNELS[kernel] + ("multi_pass=0",))
    _, st0, one = run(A, w.reads, want)
    A.set_pipeline("multi_pass=1")
    for cap in (2, 1, retried - 1, 0):
        A.set_pipeline("resume_cap=%d" % cap)
        _, st, launches = run(A, w.reads, want)
        assert 1 <= launches <= mpw.N_PASSES_DEEP, (cap, launches)
        if cap == 0:
            assert launches == 1
        for key in ("n_extensions", "n_columns", "n_fast_columns"):
            assert st[key] == st0[key], (cap, key)
    A.set_pipeline("resume_cap=-1")
    _, _, launches = run(A, w.reads, want)
    assert launches == mpw.N_PASSES_DEEP


# ---- automatic choice ----------------------------------------------------------------------------------------------------------------

def test_automatic_choice():
    """choose_multi_pass takes the multi-pass extension from 24 seeds per read on: deep is far above (the oracle's seed lists), shallow
    far below (test_multi_pass_emu.py::test_preconditions_of_the_worlds)"""
    assert cpu.deep_seeds_per_read() >= 2 * 24
    w = mpw.deep()
    want = mpw.oracle("deep")
    A = handle(w)
    run(A, w.reads, want)
    _, _, auto = run(A, w.reads, want)
    assert auto > 1 and auto == mpw.N_PASSES_DEEP
    s = mpw.shallow()
    B = handle(s)
    run(B, s.reads, mpw.oracle("shallow"))
    _, _, auto = run(B, s.reads, mpw.oracle("shallow"))
    B.set_pipeline("multi_pass=0")
    _, _, one = run(B, s.reads, mpw.oracle("shallow"))
    assert auto == one


# ---- one handle, changing shape ------------------------------------------------------------------------------------------------------

def test_one_handle_batches_of_changing_shape():
    """deep (multi-pass), a single-pass batch, deep cut to 120 bp (another Lmax: another resume record size in the same pools),
    deep again, an empty batch.  The handle is bound to deep's graph and configuration, under which even shallow's reads carry
    dozens of sub-k seeds: the second batch is shallow's reads on deep's graph with multi_pass=0 set for it; the others choose
    the passes themselves."""
    w = mpw.deep()
    want = mpw.oracle("deep")
    A = handle(w, 1, KERNELS["grp8"])
    run(A, w.reads, want)
    first = run(A, w.reads, want)
    assert first[2] == mpw.N_PASSES_DEEP
    s_reads = mpw.shallow().reads
    o = orc.AlignRun(w.g, w.config(), s_reads)
    assert o.error == ""
    A.set_pipeline("multi_pass=0")
    _, _, launches = run(A, s_reads, o.results())
    assert launches == 1
    A.set_pipeline("multi_pass=-1")
    short = mpw.cut(w.reads, 120)
    assert max(len(r) for r in short) == 120 < max(len(r) for r in w.reads)
    o = orc.AlignRun(w.g, w.config(), short)
    assert o.error == ""
    _, _, launches = run(A, short, o.results())
    assert 1 < launches <= mpw.N_PASSES_DEEP
    again = run(A, w.reads, want)
    assert again[0] == first[0] and again[2] == first[2]
    assert [again[1][k] for k in ("n_extensions", "n_columns", "n_fast_columns")] == [first[1][k] for k in ("n_extensions", "n_columns", "n_fast_columns")]
    got, status = A.align_batch([])
    assert got == [] and status == []


# ---- capacity in a late pass ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["ext64", "grp8"])
def test_capacity_in_a_late_pass(kernel):
    """max_columns so small that some reads of deep run out of columns after they have been resumed
    (test_multi_pass_emu.py::test_capacity_status_in_a_late_pass found the value and that such reads exist)"""
    w = mpw.deep()
    want = mpw.oracle("deep")
    lim = capi.Limits()
    lim.max_columns = mpw.LATE_CAPACITY_MAX_COLUMNS
    A = handle(w, 1, KERNELS[kernel] + ("multi_pass=1", "retry_capacity=0"), limits=lim)
    got, status = A.align_batch(w.reads)
    assert set(status) == {0, capi.MGX_ERR_CAPACITY}, status
    for q in range(len(w.reads)):
        if status[q] == 0:
            assert got[q] == want[q], (q, w.kinds[q])
    B = handle(w, 1, KERNELS[kernel] + ("multi_pass=1",), limits=lim)
    got, status = B.align_batch(w.reads)
    assert all(s == 0 for s in status), status
    assert got == want
    assert B.stats()["n_capacity_retried"] > 0
