"""The lane-per-read seeder (metagraph_amd/csrc/seed_lane.hpp) at its leave reasons and buffer limits, in the host model: the
directed worlds of tests/seed_lane_cases.py, each read's fate pinned — which SL_LEAVE code sends it on, or that a lane seeds it —
next to seed lists, num_matching and alignments of every read against the oracle.  (tests/test_gpu_seed_lane_edges.py: the same
cases through the kernel and its launch code.)"""
import collections

import pytest

import emu_drv
import orc
import seed_lane_cases as slc
from test_seed_lane import run, seedlane_env  # noqa: F401


def model(case):
    e = emu_drv.EmuRun(emu_drv.EmuGraph(case.graph), case.config, case.reads, limits=case.limits)
    assert e.error == "", e.error
    return e


@pytest.mark.parametrize("name", list(slc.CASES))
def test_case(seedlane_env, name):
    c = slc.CASES[name]()
    ran, done, why = run(c.graph, c.config, c.reads, limits=c.limits)     # seeds, num_matching, alignments, statuses against the oracle
    e = model(c)
    assert ran
    reasons = e.seedlane_reasons()
    final = [r[0] for r in reasons]
    print(name, "reads", len(c.reads), "final", dict(collections.Counter(final)), "first pass", dict(collections.Counter(r[1] for r in reasons)))
    assert final == c.expected, [(i, final[i], c.expected[i]) for i in range(len(final)) if final[i] != c.expected[i]]
    assert why == {k: v for k, v in collections.Counter(final).items() if k}
    assert done + sum(why.values()) == len(c.reads)
    for i, code in c.first_pass.items():
        assert reasons[i][1] == code, (i, reasons[i], code)


@pytest.mark.parametrize("name", slc.first_pass_cases())
def test_first_pass_alone(seedlane_env, monkeypatch, name):
    """the boundary pairs: the read at the limit is finished by the first pass, the read one above is left by it"""
    monkeypatch.setenv("MGX_EMU_SEEDLANE_ONE", "1")
    c = slc.CASES[name]()
    assert c.first_pass
    e = model(c)
    got, status = e.results()
    assert all(s == 0 for s in status)
    o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
    assert got == o.results()
    reasons = e.seedlane_reasons()
    ran, done, why = e.seedlane_stats()
    assert ran and done + sum(why.values()) == len(c.reads)
    for i, code in c.first_pass.items():
        assert reasons[i] == (code, code, 0), (i, reasons[i], code)
    assert done == sum(1 for r in reasons if r[0] == 0)


def test_entries_32_counts():
    """the buffer entries of entries_32()'s reads are their seeds (min_seed_length == k: no pending records): the oracle's counts
    say that the reads sit where the case claims — 32, 33 and 34 against SL_SEEDS_1 = 32"""
    c = slc.entries_32()
    o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
    assert [len(o.seeds(0)[q][0]) + len(o.seeds(1)[q][0]) for q in range(len(c.reads))] == slc.ENTRIES_32_SEEDS


def test_many_counts():
    """likewise one seed per k-mer: 192 / 194 / 193 and 288 / 290 / 289 seeds against SL_SEEDS_1_MANY, SL_SEEDS_2 and the _LONG sizes"""
    for case, want in ((slc.many_192(), [192, 194, 193]), (slc.many_288(), [288, 290, 289])):
        o = orc.AlignRun(case.graph, case.config, case.reads, validate=False)
        assert [len(o.seeds(0)[q][0]) + len(o.seeds(1)[q][0]) for q in range(3)] == want


def test_tail_position_reports_after_all():
    """read 0 of tail_positions(1) takes the path the case was written for: the oracle has two seeds of 15 characters at a
    tail position (85 >= n = 80) behind the last k-mer's seed; the usual read next to it has none"""
    c = slc.tail_positions(1)
    o = orc.AlignRun(c.graph, c.config, c.reads, validate=False)
    sub = [[(x["clipping"], x["length"], x["offset"]) for x in o.seeds(0)[q][0] if x["offset"]] for q in (0, 1)]
    assert sub == [slc.TAIL_REPORTS, []]


def test_every_code_has_a_case():
    """every SL_LEAVE code of seed_lane.hpp is some read's expected fate, or argued unreachable in seed_lane_cases.py, or — code
    9 — listed there as not reached by any case"""
    import os
    import re
    src = open(os.path.join(emu_drv.ROOT, "metagraph_amd", "csrc", "seed_lane.hpp")).read()
    codes = {int(x) for x in re.findall(r"SL_LEAVE\((\d+)\)", src)}
    seen = set()
    for b in slc.CASES.values():
        c = b()
        seen |= set(c.expected) | set(c.first_pass.values())
    unreachable, not_reached = {2, 5, 14}, {9}                    # (the arguments: the head of seed_lane_cases.py)
    assert codes - seen == unreachable | not_reached, (sorted(codes), sorted(seen))
