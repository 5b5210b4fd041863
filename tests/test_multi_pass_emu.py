"""The multi-pass extension under the host model, at every step of its seed limit: the worlds of tests/multi_pass_worlds.py
through MGX_EMU_SPLIT=1 MGX_EMU_MULTIPASS=1, whose loop takes the limits of the product's (multi_pass_seed_limit,
host_common.hpp: 1, 4, 16, then none at pass 24), with full alignment lists against the oracle.  CPU only.

What is pinned here and nowhere else on the CPU: pass_limit_reached() at limits above 1, the count of seeds inside a pass, the
unlimited pass that ends the loop, reads that find no room for a resume record, and a capacity status that arises in a later
pass than a read's first.  tests/test_gpu_multi_pass.py runs the same worlds through extend_multi_pass on the device and takes
the pass counts and the retry count asserted here as its expectation."""
import collections
import functools
import os
import subprocess
import sys

import pytest

import emu_drv
import multi_pass_worlds as mpw
from metagraph_amd import capi

CAPS = ["n", "2", "0"]        # resume records a pass may write: one per read (the default), two, none

_ENV = ("MGX_EMU_SPLIT", "MGX_EMU_MULTIPASS", "MGX_EMU_RESUME_CAP")


Run = collections.namedtuple("Run", "results status ext stats passes retried error")


@functools.lru_cache(maxsize=None)
def emu_run(name, n_alt=1, cap="n", multi=True, max_columns=0):
    """one host-model run of a world (cached: the tests share them and never change them)"""
    w = mpw.WORLDS[name]()
    old = {k: os.environ.get(k) for k in _ENV}
    os.environ["MGX_EMU_SPLIT"] = "1"
    os.environ["MGX_EMU_MULTIPASS"] = "1" if multi else "0"
    if cap != "n":
        os.environ["MGX_EMU_RESUME_CAP"] = cap
    else:
        os.environ.pop("MGX_EMU_RESUME_CAP", None)
    try:
        lim = mpw.alt_limits(n_alt)
        if max_columns:
            lim = capi.Limits()
            lim.max_columns = max_columns
        e = emu_drv.EmuRun(emu_drv.EmuGraph(w.g, mode=w.mode), w.config(n_alt), w.reads, limits=lim)
        results, status = e.results() if e.error == "" else ([], [])
        return Run(results, status, [i["n_extensions"] for i in e.seed_info()] if e.error == "" else [], e.stats(), e.pass_items(),
                   e.retried(), e.error)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def in_bucket(ext, name):
    return sum(1 for x in ext if mpw.bucket_of(x) == name)


def test_preconditions_of_the_worlds():
    """Conditions on the worlds, not measurements: the extension counts per read that make reads retire under every seed limit,
    from the host model's seed info, and what the oracle aligns.  If a change of the generator empties a bucket, change the
    generator's parameters until this passes again; the buckets stay."""
    deep = mpw.deep()
    assert len(deep.repeat_reads()) >= 24
    assert {"exact", "sub1", "chimera", "edge"} <= set(deep.kinds)
    assert "" in deep.reads and any(0 < len(r) < deep.k for r in deep.reads) and any(r and set(r) == {"N"} for r in deep.reads)
    r = emu_run("deep")
    assert r.error == ""
    for name, _, _ in mpw.BUCKETS:
        assert in_bucket(r.ext, name) >= 4, (name, sorted(r.ext))
    want = mpw.oracle("deep")
    rep = deep.repeat_reads()
    assert 2 * sum(1 for i in rep if want[i]) > len(rep)
    assert max(len(a) for a in mpw.oracle("deep", 4)) > 2
    p = emu_run("deep_primary")
    assert p.error == ""
    assert sum(1 for x in p.ext if x > 40) >= 4, sorted(p.ext)
    assert mpw.deep_primary().reads[1::2] == [mpw.rc(x) for x in deep.reads[1::2]]
    s = emu_run("shallow")
    assert s.error == "" and max(s.ext) <= 2, sorted(s.ext)
    # the batch's seeds per read, on which the product's automatic choice rests (24 or more: multi-pass), is far from it on both sides
    assert deep_seeds_per_read() >= 2 * 24 and r.stats["seeds"] // len(deep.reads) >= 2 * 24
    assert s.stats["seeds"] // len(mpw.shallow().reads) < 24 // 2


def deep_seeds_per_read():
    """seeds per read of `deep` by the oracle's seed lists (both strands)"""
    import orc
    w = mpw.deep()
    o = orc.AlignRun(w.g, w.config(), w.reads)
    return sum(len(ss) for strand in (0, 1) for ss, _ in o.seeds(strand)) // len(w.reads)


WORLD_CASES = [("deep", 1), ("deep", 2), ("deep", 4), ("deep_primary", 1), ("shallow", 1)]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name,n_alt", WORLD_CASES)
def test_worlds_against_the_oracle(name, n_alt, cap):
    """full alignment lists of every world at every resume capacity; with 2 or 0 records per pass the other retrying reads go on
    without a limit in the same pass"""
    w = mpw.WORLDS[name]()
    r = emu_run(name, n_alt, cap)
    assert r.error == ""
    assert all(s == 0 for s in r.status), r.status
    want = mpw.oracle(name, n_alt)
    for q in range(len(w.reads)):
        assert r.results[q] == want[q], (q, w.kinds[q], w.reads[q])
    if name != "shallow":
        assert r.retried > 2          # more reads want a record than the small capacities have


def test_pass_counts():
    """deep runs passes 0 .. 24: a read with live seeds left after eight passes of one seed, eight of four and eight of sixteen is
    finished by the pass without a limit, which is the last whatever it leaves.  At least four reads are still at work under
    each limit.  shallow is done in two passes at the most.  The GPU tests expect these numbers of launches."""
    r = emu_run("deep")
    assert len(r.passes) == mpw.N_PASSES_DEEP, r.passes
    n = len(mpw.deep().reads)
    assert r.passes[0] == n and r.passes[1] == r.retried
    assert all(a >= b for a, b in zip(r.passes, r.passes[1:])), r.passes
    assert r.passes[8] >= 4 and r.passes[16] >= 4 and r.passes[24] >= 4, r.passes
    # two records per pass: passes of two reads, as long as two want to go on
    r2 = emu_run("deep", 1, "2")
    assert r2.passes[0] == n and set(r2.passes[1:]) <= {1, 2} and len(r2.passes) <= mpw.N_PASSES_DEEP, r2.passes
    assert emu_run("deep", 1, "0").passes == [n]
    assert len(emu_run("shallow").passes) <= 2


def test_the_other_deep_worlds_end_at_pass_24_too():
    for n_alt in (2, 4):
        assert len(emu_run("deep", n_alt).passes) == mpw.N_PASSES_DEEP
    assert len(emu_run("deep_primary").passes) == mpw.N_PASSES_DEEP


@pytest.mark.parametrize("name,n_alt", WORLD_CASES)
def test_counters_travel_in_the_resume_record(name, n_alt):
    """extensions, columns and fast columns of a read are part of its resume record (resume_save / resume_load): over the batch
    they equal those of the run without resume records (the model's two-pass form: a read that wants a second seed is started
    again without a limit and extends all its seeds in one go; the counters are those of that run).  With fewer records than
    retrying reads they still do: a read without a record is not started again, it goes on where it stopped."""
    one = emu_run(name, n_alt, "n", multi=False)
    assert one.error == "" and one.stats["extensions"] > 0
    for cap in CAPS:
        r = emu_run(name, n_alt, cap)
        for key in ("extensions", "columns", "fast_columns", "seeds", "capacity_errors"):
            assert r.stats[key] == one.stats[key], (cap, key, r.stats, one.stats)
        assert r.ext == one.ext


def test_capacity_status_in_a_late_pass():
    """A read that runs out of columns after it has been resumed: its status is MGX_ERR_CAPACITY, the reads around it are
    untouched.  Pass 0 extends one seed per read — one forward extension and, with one alignment per seed, at most one backward
    — so a capacity read with more than 2 extensions failed in a later pass."""
    w = mpw.deep()
    r = emu_run("deep", 1, "n", True, mpw.LATE_CAPACITY_MAX_COLUMNS)
    assert r.error == ""
    assert set(r.status) == {0, capi.MGX_ERR_CAPACITY}, collections.Counter(r.status)
    want = mpw.oracle("deep")
    for q in range(len(w.reads)):
        if r.status[q] == 0:
            assert r.results[q] == want[q], (q, w.kinds[q])
    late = [q for q in range(len(w.reads)) if r.status[q] == capi.MGX_ERR_CAPACITY and r.ext[q] > 2]
    assert late, [(q, r.ext[q]) for q in range(len(w.reads)) if r.status[q]]
    assert r.stats["capacity_errors"] == sum(1 for s in r.status if s)


def retried_after_pass_0():
    """reads of deep that want another pass after pass 0 (for the GPU tests' resume_cap one below it)"""
    return emu_run("deep").retried


@pytest.mark.parametrize("lanes", ["16", "8"])
def test_deep_in_the_group_models(lanes):
    """deep at every capacity, its pass counts and the capacity status in a late pass with 16 and 8 lanes per read (64: the tests above); a subprocess, because the
    model's lane count is a compile-time constant of the loaded library"""
    env = dict(os.environ, MGX_EMU_WAVE=lanes)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.abspath(__file__), "-k",
                        "(test_worlds_against_the_oracle and deep-1-) or test_pass_counts or test_capacity_status_in_a_late_pass", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, r.stdout[-500:]
