#!/usr/bin/env python3
"""Timeline of one steady bench step (rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -- python bench.py ...): every
kernel, fill and copy of the step with its start, its duration and the idle gap in front of it.  tools/timeline.py reads a decode run
(it looks for k_inflate_wave); this one reads the device step: a cycle runs from one k_direct_c8 start to the next, so it holds that
call's kernels and copies back followed by the next step's reset and uploads — the same events as one step, rotated.
Usage: tools/step_timeline.py <dir with *_kernel_trace.csv and *_memory_copy_trace.csv> [cycles to skip at the front, default 8]"""
import csv
import glob
import os
import sys


def short(name):
    for k in ("k_direct_c8", "k_direct_tiles_heavy", "k_c8_heavy", "k_window_gather", "k_reset_spans", "fillBuffer", "copyBuffer"):
        if k in name:
            return k
    return name.split("(")[0][:40]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main(d, skip):
    kf = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    cf = glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True)
    ev = []
    for r in csv.DictReader(open(kf)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    if cf:
        for r in csv.DictReader(open(cf[0])):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Direction"].replace("MEMORY_COPY_", "copy ")))
    ev.sort()
    marks = [i for i, e in enumerate(ev) if e[2] == "k_direct_c8"]
    if len(marks) < skip + 3:
        print("only %d k_direct_c8 launches in the trace" % len(marks)); return
    cycles = [ev[a:b] for a, b in zip(marks[skip:], marks[skip + 1:])]
    shape = [e[2] for e in cycles[len(cycles) // 2]]
    same = [c for c in cycles if [e[2] for e in c] == shape]
    print("%d cycles (k_direct_c8 start to the next one's) behind the first %d, %d of them with the middle cycle's %d events" % (len(cycles), skip, len(same), len(shape)))
    length = [(b[0][0] - a[0][0]) / 1e3 for a, b in zip(cycles, cycles[1:])]
    print("cycle length: median %.1f us, range %.1f-%.1f" % (median(length), min(length), max(length)))
    print("the middle cycle, us from its k_direct_c8 start:")
    print("  %-24s %10s %10s %10s" % ("event", "start", "duration", "gap before"))
    c = cycles[len(cycles) // 2]
    for j, e in enumerate(c):
        print("  %-24s %10.1f %10.1f %10.1f" % (e[2], (e[0] - c[0][0]) / 1e3, (e[1] - e[0]) / 1e3, (e[0] - c[j - 1][1]) / 1e3 if j else 0.0))
    print("medians over the %d cycles of that shape, us:" % len(same))
    print("  %-24s %10s %10s %10s" % ("event", "start", "duration", "gap before"))
    busy = 0.0
    for j, name in enumerate(shape):
        dur = median([s[j][1] - s[j][0] for s in same]) / 1e3
        gap = median([s[j][0] - s[j - 1][1] for s in same]) / 1e3 if j else 0.0
        busy += dur
        print("  %-24s %10.1f %10.1f %10.1f" % (name, median([s[j][0] - s[0][0] for s in same]) / 1e3, dur, gap))
    print("sum of the median durations %.1f us" % busy)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8)
