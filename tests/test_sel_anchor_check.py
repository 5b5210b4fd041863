"""The select anchors of the device index (graph_build.hpp: sel_anchor_shift, build_sel_anchor; dev_graph.hpp: sel_predict,
select_last_scan) and the rank / select / pred / succ primitives beside them, compiled for the host against the wave model
(tests/emu/wave.hpp) and compared with plain loops for EVERY rank and index of random tables: anchor shifts 6 .. 12 at table
sizes of a few thousand edges (max_entries 4 .. 64 where the device has 8192), totals of (m << shift) - 1, m << shift and
(m << shift) + 1, one `last` bit in 5 up to all ones, ragged and exactly full final blocks.  The program counts every block
load and refuses one outside the table; it is built with the address and undefined-behaviour sanitizers.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O0", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-DMGX_MAX_ALT=4", "-DMGX_WITH_PRIMARY=1", "-DMGX_WITH_LABELS=1", "-w"]


def test_select_anchors_and_index_primitives_equal_the_plain_loops(tmp_path):
    exe = str(tmp_path / "sel_anchor_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++"] + FLAGS + ["-I" + emu, "-I" + os.path.join(ROOT, "metagraph_amd", "csrc"), "-o", exe,
                                      os.path.join(emu, "sel_anchor_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout)
    m = re.match(r"ok (\d+) \(r, shift\) pairs on (\d+) tables, shifts 6\.\.12:((?: \d+){7});", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 1000000 and all(int(x) > 10000 for x in m.group(3).split())
    # the guard counts: every select loads at least one block through the counted loader, none of them outside the table
    loads = re.search(r"; (\d+) block loads, (\d+) outside the table$", r.stdout.rstrip())
    assert loads, r.stdout
    assert int(loads.group(1)) >= 2 * int(m.group(1)) and int(loads.group(2)) == 0
