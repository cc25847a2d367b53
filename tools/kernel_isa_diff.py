#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two source trees, kernel by kernel.

    tools/kernel_isa_diff.py OLD_TREE NEW_TREE --old FILE.hip ... --new FILE.hip ...

Each FILE (relative to its tree) is compiled device-only to assembly, the assembly is cut by kernel symbol, and what depends on a
kernel's position in its file (the function index of basic-block labels, the .Lfunc_* labels) is normalised.  Per demangled kernel
name: whether the two instruction texts are identical, and each side's VGPRs, SGPRs, scratch bytes, LDS bytes and occupancy.  Whole
texts are compared; nothing is searched for.  Exit status 1 when a name is on one side only or a text differs.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]
FIELDS = [".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size"]
SHORT = ["vgpr", "sgpr", "scratch", "lds", "occ"]


def compile_asm(tree, rel, out):
    subprocess.run([HIPCC] + FLAGS + [os.path.join(tree, rel), "-o", out], check=True, cwd=tree)
    return open(out).read().split("\n")


def kernels(lines):
    """{mangled name: (normalised text, [vgpr, sgpr, scratch, lds, occupancy])} of one assembly file"""
    names = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    text, res, cur, body, desc = {}, {n: [None] * 5 for n in names}, None, None, None
    for l in lines:
        s = l.strip()
        if body is None and ":" in s and s.split(":")[0] in names:          # "name:    ; @name"
            cur, body = s.split(":")[0], []
        elif body is not None and s.startswith(".section"):                 # the kernel descriptor follows the last instruction
            text[cur], body = "\n".join(body), None
        elif body is not None:
            s = re.sub(r"\s+", " ", re.sub(r"(\.L)?BB\d+_(\d+)", r"BB_\2", s))   # (the index's width moves the comment column)
            body.append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s))
        elif s.startswith(".amdhsa_kernel "):
            desc = s.split()[1]
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc and s.split(" ")[0] in FIELDS:
            res[desc][FIELDS.index(s.split()[0])] = int(s.split()[1], 0)
        elif cur and s.startswith("; Occupancy:"):
            res[cur][4] = int(s.split(":")[1])
    return {n: (text[n], res[n]) for n in names}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, (re.sub(r"^void ", "", d).split("(")[0] for d in out.split("\n"))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree"), ap.add_argument("new_tree")
    ap.add_argument("--old", nargs="+", required=True), ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    jobs = [(os.path.abspath(a.old_tree), f, 0) for f in a.old] + [(os.path.abspath(a.new_tree), f, 1) for f in a.new]
    side = [{}, {}]
    with tempfile.TemporaryDirectory() as td, concurrent.futures.ThreadPoolExecutor(4) as ex:
        futs = [(ex.submit(compile_asm, t, f, os.path.join(td, "%d.s" % i)), s) for i, (t, f, s) in enumerate(jobs)]
        for fut, s in futs:
            ks = kernels(fut.result())
            dm = demangle(sorted(ks))
            side[s].update({dm[n]: v for n, v in ks.items()})
    old, new = side
    bad = 0
    for only, where in ((set(old) - set(new), "old"), (set(new) - set(old), "new")):
        for n in sorted(only):
            print("ONLY-%s  %s" % (where.upper(), n))
            bad += 1
    same = 0
    for n in sorted(set(old) & set(new)):
        eq = old[n][0] == new[n][0]
        same += eq
        bad += not eq
        fmt = lambda r: " ".join("%s=%s" % kv for kv in zip(SHORT, r))
        print("%s  %s\n    old: %s\n    new: %s%s" % ("IDENTICAL" if eq else "DIFFERENT", n, fmt(old[n][1]), fmt(new[n][1]),
                                                    "" if old[n][1] == new[n][1] else "    <- resources differ"))
    print("kernels: old %d, new %d, in both %d, identical text %d, different text %d" % (len(old), len(new), len(set(old) & set(new)), same,
                                                                                       len(set(old) & set(new)) - same))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
