"""The lane-per-read extender (metagraph_amd/csrc/lane_read.hpp) at its hand-over reasons, limits and batch shapes, in the host
model: the directed worlds of tests/lane_cases.py, each read's fate pinned — which LANE_BAIL code sends it to the group kernel, or
that a lane finishes it — next to the alignments (label-aware: with their labels) of every read against the oracle.
(tests/test_gpu_lane_edges.py: the same cases through the kernel and its launch code.)"""
import collections
import os
import re

import pytest

import emu_drv
import lane_cases as lc
import orc
from labeled_worlds import with_labels


@pytest.fixture(autouse=True)
def _lane_env(monkeypatch):
    monkeypatch.setenv("MGX_EMU_SPLIT", "1")
    monkeypatch.setenv("MGX_EMU_LANE", "1")


@pytest.fixture(scope="module")
def oracle():
    """name -> the oracle's results of the case (run once per module)"""
    cache = {}

    def get(name):
        if name not in cache:
            c = lc.CASES[name]()
            if c.annotation is not None:
                o = orc.LabeledAlignRun(c.graph, c.config, c.annotation, c.reads, validate=False)
                assert o.error == "", o.error
                cache[name] = with_labels(o)
            else:
                o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
                assert o.error == "", o.error
                cache[name] = o.results()
        return cache[name]
    return get


def model(c, limits):
    anno = emu_drv.EmuAnnotation(c.annotation) if c.annotation is not None else None
    e = emu_drv.EmuRun(emu_drv.EmuGraph(c.graph), c.config, c.reads, limits=limits, annotation=anno)
    assert e.error == "", e.error
    return e


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case(oracle, name):
    c = lc.CASES[name]()
    assert 0 in c.expected or name == "shape_all_leave"            # (a kernel that hands everything over cannot pass)
    want = oracle(name)
    e = model(c, c.limits)
    got, status = e.results()
    reasons = e.lane_reasons()
    print(name, "reads", len(c.reads), "fates", dict(collections.Counter(reasons)))
    assert reasons == c.expected, [(i, reasons[i], c.expected[i]) for i in range(len(reasons)) if reasons[i] != c.expected[i]]
    ran, done = e.lane_stats()
    assert ran and done == c.expected.count(0)
    assert e.lane_bails() == {k: v for k, v in collections.Counter(c.expected).items() if k}
    # A read that left on a capacity guard meets the same limit in the group kernel, which reports it: the batch's capacity retry
    # aligns such reads with larger limits (mgx_align_batch; the host model has no retry: the default limits stand in for it).
    # Every other read has its alignments now.
    capacity = [q for q, s in enumerate(status) if s != 0]
    assert all(status[q] == -5 and c.expected[q] in lc.CAPACITY for q in capacity), status
    assert not capacity or c.limits is not None
    for q in range(len(c.reads)):
        if q not in capacity:
            assert got[q] == want[q], (q, c.reads[q], got[q], want[q])
    if capacity:
        e2 = model(c, None)
        got2, status2 = e2.results()
        assert all(s == 0 for s in status2), status2
        for q in capacity:
            assert got2[q] == want[q], (q, c.reads[q], got2[q], want[q])


def test_cigar_run_counts(oracle):
    """the reads of cigar_runs() sit where the case claims: the oracle's alignments have 15, 16, 17 runs and one"""
    assert [len(re.findall(r"\d+[=XIDS]", r[0]["cigar"])) for r in oracle("cigar_runs")] == lc.CIGAR_RUNS


def test_many_seeds_counts():
    """the reads of many_seeds() have the seeds the case claims, all on one strand: 513, 510 and 576 against LANE_MAX_SEEDS = 512"""
    c = lc.many_seeds()
    o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
    assert [len(o.seeds(0)[q][0]) for q in range(3)] == lc.MANY_SEEDS and not any(o.seeds(1)[q][0] for q in range(3))


def test_merged_vector_seeds():
    """the reads of merged_vector() with a wrong last character take the branch the case was written for: a second seed, below
    k, whose node is the first seed's first node; the read of K + 1 genome characters has another node there"""
    c = lc.merged_vector()
    o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
    for q, r in enumerate(c.reads):
        ss = o.seeds(0)[q][0] or o.seeds(1)[q][0]
        assert len(ss) == 2 and ss[0]["offset"] == 0 and (ss[1]["length"], ss[1]["offset"]) == (19, 2), ss
        assert (ss[1]["nodes"][0] == ss[0]["nodes"][0]) == (q < 4), ss


def test_backward_reads_take_two_extensions():
    """the reads of backward() and shape_backward_mixed() are finished by a lane in two passes (LR_AGAIN), the plain ones in one"""
    for c in (lc.backward(), lc.shape_backward_mixed()):
        info = model(c, None).seed_info()
        sub = [q for q in range(len(c.reads)) if c.reads[q] not in lc.main_world()[1] and lc.rc(c.reads[q]) not in lc.main_world()[1]]
        assert len(sub) >= len(c.reads) // 2
        assert all(info[q]["n_extensions"] == (2 if q in sub else 1) for q in range(len(c.reads)))


def test_every_code_is_in_the_table():
    """every LANE_BAIL code of lane_read.hpp is some read's expected fate, or argued unreachable in lane_cases.py, or listed there
    as not reached; and the table at the head of lane_cases.py names each code exactly once"""
    src = open(os.path.join(emu_drv.ROOT, "metagraph_amd", "csrc", "lane_read.hpp")).read()
    codes = {int(x) for x in re.findall(r"LANE_BAIL\((\d+)\)", src)}
    seen = set()
    for b in lc.CASES.values():
        seen |= set(b().expected)
    seen.discard(0)
    assert seen == lc.REACHED, (sorted(seen), sorted(lc.REACHED))
    assert not (lc.REACHED & lc.UNREACHABLE) and not (lc.REACHED & lc.NOT_REACHED) and not (lc.UNREACHABLE & lc.NOT_REACHED)
    assert codes == lc.REACHED | lc.UNREACHABLE | lc.NOT_REACHED, sorted(codes)
    table = lc.__doc__[lc.__doc__.index("The codes (LANE_BAIL"):]
    listed = []
    for line in table.splitlines():
        m = re.match(r"^ {1,2}(\d+(?:, \d+)*)(?::|  )", line)
        if m:
            listed += [int(x) for x in m.group(1).split(", ")]
    assert sorted(listed) == sorted(codes), listed
    # DESIGN 5.1 carries the same table
    design = open(os.path.join(emu_drv.ROOT, "DESIGN.md")).read()
    assert table.strip() in design

