"""The per-read counting of `align --map` (metagraph_amd/csrc/map_summary.hpp: the three graph-mode rules, the short-read and the
long-read form of k_map_summary) compiled for the host against the wave model (tests/emu/wave.hpp) and compared with a std::set
brute force on random node arrays with many repeats and zeros, 0 ... 33 000 k-mers per read.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_summary_equals_the_brute_force(tmp_path):
    exe = str(tmp_path / "map_summary_check")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + emu, "-o", exe, os.path.join(emu, "map_summary_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok "), out
