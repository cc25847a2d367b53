#!/usr/bin/env python3
"""Which waits stand in front of the loads of a kernel's loops: the gfx950 assembly of one source file, read loop by loop.

    tools/sweep_waits.py [TREE] [--file pandepth_amd/csrc/pd_direct.hip] [--kernel SUBSTRING ...] [--loads REGEX] [--asm FILE.s] [--priming N] [--assert-no-drain]

The file is compiled device-only to assembly as tools/kernel_isa_diff.py does.  For every kernel whose demangled name contains one of
the SUBSTRINGs (default: the two cover forms of k_direct_c8) the loops are found from the backward branches: loops that overlap or nest
count as one, a loop that holds an s_barrier (the walk over the tiles) is not one of them.  Per loop that holds a load matching REGEX (default: the 16-byte loads, global_load_dwordx4): each such load
in text order, and in front of it every `s_waitcnt` that names vmcnt between the load before it in that loop (or the loop's header)
and the load itself.  A software pipeline keeps its loads in flight when each of those waits leaves as many loads pending as were
issued behind the chunk about to be worked on; `vmcnt(0)` in front of a loop's load drains the pipeline there.  Overlapping backward
branches are merged, so a listed loop may take in loads that stand in front of the rotation proper: --priming N says that the first N loads of each
listed loop are such (the narrow cover form's two priming loads; the wide form's lie outside its loop) — they are marked and not judged.
--assert-no-drain makes the criterion an exit status: 2 when a load of a rotation stands behind vmcnt(0).
Per kernel: VGPRs, SGPRs, scratch bytes, LDS bytes, occupancy.
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_isa_diff as kid  # noqa: E402

COVER_FORMS = ["k_direct_c8<7, 4, false, true, 1, true, true>", "k_direct_c8<7, 4, false, true, 1, true, false>"]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s*s_c?branch\w*\s+(\.LBB\d+_\d+)")


def bodies(lines):
    """{mangled name: [the kernel's lines]} of one assembly file"""
    names = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    out, cur = {}, None
    for l in lines:
        s = l.strip()
        if cur is None and ":" in s and s.split(":")[0] in names:
            cur = s.split(":")[0]
            out[cur] = []
        elif cur is not None and s.startswith(".section"):
            cur = None
        elif cur is not None:
            out[cur].append(l.rstrip())
    return out


def loops_of(body):
    """[(first line, last line)] of a kernel's load loops: a branch to a label that stands before it closes a loop; a loop that holds an
    s_barrier (the walk over tiles) is left out, and loops that overlap or nest (the structured control flow of ONE source loop) are one"""
    at = {m.group(1): i for i, l in enumerate(body) for m in [LABEL.match(l)] if m}
    found = []
    for j, l in enumerate(body):
        m = BRANCH.match(l)
        if m and m.group(1) in at and at[m.group(1)] < j and not any("s_barrier" in x for x in body[at[m.group(1)]:j]):
            found.append((at[m.group(1)], j))
    merged = []
    for i, j in sorted(found):
        if merged and i <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(j, merged[-1][1]))
        else:
            merged.append((i, j))
    return merged


def report(name, body, res, loads, out, priming=0):
    out.write("%s\n    %s\n" % (name, " ".join("%s=%s" % kv for kv in zip(kid.SHORT, res))))
    loops = loops_of(body)
    inner, drains = {}, 0
    for k, l in enumerate(body):
        if loads.search(l.split(";")[0]):
            for i, j in loops:
                if i < k < j:
                    inner.setdefault((i, j), []).append(k)
    if not inner:
        out.write("    no loop holds such a load\n")
    for (i, j), ks in sorted(inner.items()):
        out.write("    loop %s, %d lines, %d loads\n" % (body[i].split(":")[0], j - i + 1, len(ks)))
        prev = i
        for n, k in enumerate(ks):
            waits = [re.sub(r"\s+", " ", body[x].split(";")[0].strip()) for x in range(prev, k) if "s_waitcnt" in body[x] and "vmcnt" in body[x]]
            where = "%d lines behind the loop's header" % (k - i) if prev == i else "%d lines behind the load before it" % (k - prev)
            rot = n >= priming
            out.write("        %-44s %s%s\n" % (re.sub(r"\s+", " ", body[k].split(";")[0].strip()), where, "" if rot else "   [priming load, in front of the rotation]"))
            out.write("            in front of it: %s\n" % (", ".join(waits) if waits else "no wait on vmcnt"))
            drains += rot and any(w.endswith("vmcnt(0)") or "vmcnt(0) " in w for w in waits)
            prev = k
    out.write("    loads of a rotation behind a vmcnt(0): %d\n\n" % drains)
    return drains


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--file", default="pandepth_amd/csrc/pd_direct.hip")
    ap.add_argument("--kernel", nargs="+", default=COVER_FORMS)
    ap.add_argument("--loads", default=r"\bglobal_load_dwordx4\b")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--priming", type=int, default=0, help="the first N loads listed per loop are priming loads in front of the rotation (the narrow cover form: 2)")
    ap.add_argument("--assert-no-drain", action="store_true", help="exit status 2 when a load of a rotation stands behind vmcnt(0)")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.asm:
        lines = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as td:
            lines = kid.compile_asm(tree, a.file, os.path.join(td, "k.s"))
    res, body = kid.kernels(lines), bodies(lines)
    dm = kid.demangle(sorted(body))
    loads = re.compile(a.loads)
    hit = drains = 0
    for want in a.kernel:
        for n in sorted(body, key=lambda n: dm[n]):
            if want.replace(" ", "") in dm[n].replace(" ", ""):
                drains += report(dm[n], body[n], res[n][1], loads, sys.stdout, a.priming)
                hit += 1
    if not hit:
        return 1
    return 2 if a.assert_no_drain and drains else 0


if __name__ == "__main__":
    sys.exit(main())
