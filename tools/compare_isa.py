#!/usr/bin/env python3
"""Did a change leave the device code of libmgx.so as it was?  A plain text comparison, per symbol, of two builds' gfx950 assembly.

    tools/compare_isa.py emit OUT_DIR          every unit of __graft_entry__.UNITS of this tree -> OUT_DIR/NAME.s (product flags plus
                                               --cuda-device-only -S, compiled from the tree's root so that paths in it are relative)
    tools/compare_isa.py diff OLD_DIR NEW_DIR  compare the *.s of two such directories

diff takes every kernel and every non-inlined device function (the symbols of type @function) of NEW_DIR and looks for a
function of the same name in OLD_DIR, in whichever unit, with the same instruction text (comments stripped, the numbering of
.LBBn_ / .Ltmpn labels normalised) and, for kernels, the same .amdhsa_ descriptor block.  One line per symbol that is new, gone or
different (with both instruction counts), one line of totals per unit; exit status 1 if any symbol differs or is new or gone."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(out_dir):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS, UNITS
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"]
    procs = [(name, subprocess.Popen([hipcc] + flags + extra + ["-o", os.path.abspath(os.path.join(out_dir, name + ".s")),
                                      os.path.join("metagraph_amd", "csrc", src)], cwd=ROOT)) for name, src, extra in UNITS]
    for name, pr in procs:
        if pr.wait() != 0:
            sys.exit("hipcc failed on " + name)


def functions(path):
    """{symbol: (instruction text, descriptor text, instruction count)} of one assembly file"""
    lines = open(path).read().split("\n")
    funcs = set(m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m)
    body, desc, cur, in_desc = {}, {}, None, None
    for ln in lines:
        ln = ln.split(";")[0].strip()
        if not ln:
            continue
        m = re.match(r"(\S+):$", ln)
        if m and m.group(1) in funcs:
            cur = m.group(1)
            body[cur] = []
        elif re.match(r"\.Lfunc_end\d+:$", ln):
            cur = None
        elif ln.startswith(".amdhsa_kernel "):
            in_desc = ln.split()[1]
            desc[in_desc] = []
        elif ln == ".end_amdhsa_kernel":
            in_desc = None
        elif in_desc:
            desc[in_desc].append(ln)
        elif cur and (not ln.startswith(".") or ln.endswith(":")):      # instructions and labels, no directives
            body[cur].append(ln)
    out = {}
    for sym, text in body.items():
        tmp = {}
        norm = []
        for ln in text:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), ".Ltmp%d" % len(tmp)), ln)
            norm.append(ln)
        out[sym] = ("\n".join(norm), "\n".join(desc.get(sym, [])), sum(1 for ln in norm if not ln.endswith(":")))
    return out


def load(d):
    return {f[:-2]: functions(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".s")}


def diff(old_dir, new_dir):
    old, new = load(old_dir), load(new_dir)
    old_by_sym = {}
    for unit, fs in old.items():
        for sym, f in fs.items():
            old_by_sym.setdefault(sym, []).append((unit, f))
    bad = 0
    seen = set()
    for unit, fs in new.items():
        same = 0
        whole = unit in old and open(os.path.join(old_dir, unit + ".s")).read() == open(os.path.join(new_dir, unit + ".s")).read()
        for sym, f in sorted(fs.items()):
            seen.add(sym)
            cands = old_by_sym.get(sym)
            if not cands:
                print("NEW        %s  %s  (%d instructions)" % (unit, sym, f[2]))
                bad += 1
            elif any(o[0] == f[0] and o[1] == f[1] for _, o in cands):
                same += 1
            else:
                ou, o = cands[0]
                print("DIFFERENT  %s  %s  text %s (%d instructions, %s: %d), descriptor %s" % (
                    unit, sym, "same" if o[0] == f[0] else "differs", f[2], ou, o[2], "same" if o[1] == f[1] else "differs"))
                bad += 1
        print("unit %-18s %4d functions, %4d identical to the old build%s" % (unit, len(fs), same, "; the whole file is identical" if whole else ""))
    for sym, cands in sorted(old_by_sym.items()):
        if sym not in seen:
            print("GONE       %s  %s  (%d instructions)" % (cands[0][0], sym, cands[0][1][2]))
            bad += 1
    print("%d symbol(s) new, gone or different" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "emit":
        emit(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
