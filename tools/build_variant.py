#!/usr/bin/env python3
"""A/B build of libmgx.so: tools/build_variant.py TAG UNITS [extra hipcc flags ...]
-> metagraph_amd/_build/libmgx_TAG.so (run with MGX_LIB_PATH=metagraph_amd/_build/libmgx_TAG.so).  Not a product build.

UNITS names, separated by commas, the units that are compiled again with the extra flags (as NAME_TAG.o); every other unit is
linked as the product build left it, so run __graft_entry__.py first.  A name is an object name of __graft_entry__.UNITS —
mgx_grp8 (the extension kernel), mgx_lane, mgx_seedlane, ... — or `host`: what used to be mgx.hip, i.e. the host units and both
builds of the seeding kernel (the -DMGX_PROBES switches live there).  Examples:
    tools/build_variant.py wps2 mgx_grp8 -DMGX_GRP_WAVES_PER_SIMD=2
    tools/build_variant.py timers mgx_lane -DMGX_LANE_TIMERS=1
    tools/build_variant.py probes host -DMGX_PROBES
    tools/build_variant.py all mgx_grp8,host -DMGX_ABLATE_BUILD"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS, UNITS  # noqa: E402

HOST = ["mgx", "mgx_graph", "mgx_map", "mgx_results", "mgx_text", "mgx_seed", "mgx_seed_primary"]


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    tag, chosen, flags = argv[0], [], argv[2:]
    for name in argv[1].split(","):
        chosen += HOST if name == "host" else [name]
    unknown = [n for n in chosen if n not in [u[0] for u in UNITS]]
    if unknown:
        sys.exit("unknown unit(s) %s; the units: host, %s" % (", ".join(unknown), ", ".join(u[0] for u in UNITS)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    build = os.path.join(ROOT, "metagraph_amd", "_build")
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    objects, procs = [], []
    for name, src, extra in UNITS:
        obj = os.path.join(build, name + ("_" + tag if name in chosen else "") + ".o")
        objects.append(obj)
        if name in chosen:
            procs.append((name, subprocess.Popen([hipcc] + cflags + extra + flags + ["-c", "-o", obj, os.path.join(ROOT, "metagraph_amd", "csrc", src)])))
        elif not os.path.exists(obj):
            sys.exit(obj + " is missing: build the product first (python __graft_entry__.py)")
    for name, pr in procs:
        if pr.wait() != 0:
            sys.exit("hipcc failed on " + name)
    lib = os.path.join(build, "libmgx_%s.so" % tag)
    subprocess.run([hipcc] + HIPCC_FLAGS + ["-o", lib] + objects, check=True)
    print("built " + lib)


if __name__ == "__main__":
    main(sys.argv[1:])
