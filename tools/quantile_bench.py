"""Cost of the depth percentiles (-quantile) on the bench's sample: pd_window_quantiles at w = 100, 1000 and 10 000 000 with one
and five percentages, and pd_depth_quantiles over one row per contig, each beside pd_reduce_windows on the same cells with the
same w (the memory-bound pass over the same 4 B per cell); then the launch shapes against each other at the widths where the
thresholds ("quantile_wave_max", "quantile_split_cells") decide, and the executable with and without `-quantile 50`.

    python tools/quantile_bench.py [--records 1e9] [--reps 3] [--e2e-records 2e7]

Kernel times are device time between events around each launch (pd_profile), summed over the call's launches; `call_ms` is the
host's clock around the whole call (batches, piece lists, results back).  Prints one JSON object."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["quantile_narrow", "quantile_block", "quantile_pieces", "quantile_pick"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1.0e9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--e2e-records", type=float, default=2.0e7)
    a = ap.parse_args()
    import torch
    import pandepth_amd as pda
    from tools import synth

    dev = torch.device("cuda", 0)
    names, lens = synth.genome_c2()
    first, other = synth.gen_runs_torch(lens, int(a.records), dev, seed=42)
    torch.cuda.synchronize()
    eng = pda.Engine(lens.astype(np.uint32), device=0)
    eng.push_intervals_device(first.data_ptr(), int(first.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
    eng.push_intervals_device(other.data_ptr(), int(other.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_DISORDER(synth.MAX_SPAN))
    eng.synchronize()
    eng.scan(0)
    del first, other
    cells = int(lens.sum())

    def timed(names_, fn):
        eng.profile(False)
        fn()                                     # warm-up (scratch, LDS reservation)
        eng.profile(True)
        rows = []
        for _ in range(a.reps):
            before = [eng.profile_get(n) for n in names_]
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            after = [eng.profile_get(n) for n in names_]
            rows.append((sum(x[0] - y[0] for x, y in zip(after, before)), wall,
                         {n: round(x[0] - y[0], 3) for n, x, y in zip(names_, after, before) if x[1] != y[1]}))
        eng.profile(False)
        rows.sort(key=lambda r: r[0])
        k, wall, parts = rows[len(rows) // 2]
        return {"kernel_ms": round(k, 3), "call_ms": round(wall, 1), "GBps": round(cells * 4 / (k / 1e3) / 1e9, 1) if k else None, "kernels": parts}

    out = {"records": int(a.records), "genome_cells": cells, "reps": a.reps, "timing": "median of reps; device events (pd_profile) and host clock"}
    cov = tot = None
    out["windows"] = {}
    for w in (100, 1000, 10_000_000):
        n = int(eng.window_layout(w)[-1])
        cov, tot = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        row = {"rows": n, "reduce_windows": timed(["reduce_windows"], lambda: eng.reduce_windows(w, 1, out=(cov, tot)))}
        for pct in ([50], [5, 25, 50, 75, 95]):
            r = timed(KERNELS, lambda: eng.window_quantiles(w, pct))
            r["x_reduce_windows"] = round(r["kernel_ms"] / row["reduce_windows"]["kernel_ms"], 2)
            row["Q" + "_".join(map(str, pct))] = r
        out["windows"][str(w)] = row
    segs = np.array([[t, 1, int(ln)] for t, ln in enumerate(lens)], dtype=np.int32)
    roff = np.arange(len(lens) + 1, dtype=np.uint64)
    r = timed(KERNELS, lambda: eng.depth_quantiles(segs, roff, [5, 25, 50, 75, 95]))
    r["x_reduce_windows_10Mb"] = round(r["kernel_ms"] / out["windows"]["10000000"]["reduce_windows"]["kernel_ms"], 2)
    out["whole_contig_rows"] = dict(r, rows=len(lens))
    # the launch shapes against each other where a threshold decides
    shapes = {}
    for w, forms in ((100, {"lanes": (1024, 262144), "workgroup": (0, 0xFFFFFFFF)}),
                     (1000, {"lanes": (1024, 262144), "workgroup": (0, 0xFFFFFFFF)}),
                     (2048, {"lanes": (2048, 262144), "workgroup": (0, 0xFFFFFFFF)}),
                     (100000, {"workgroup": (0, 0xFFFFFFFF), "pieces": (0, 0)}),
                     (262144, {"workgroup": (0, 0xFFFFFFFF), "pieces": (0, 0)}),
                     (1000000, {"workgroup": (0, 0xFFFFFFFF), "pieces": (0, 0)}),
                     (10_000_000, {"workgroup": (0, 0xFFFFFFFF), "pieces": (0, 0)})):
        got, row = None, {}
        for name, (wm, sp) in forms.items():
            eng.set_param("quantile_wave_max", wm)
            eng.set_param("quantile_split_cells", sp)
            q = [None]
            row[name] = timed(KERNELS, lambda: q.__setitem__(0, eng.window_quantiles(w, [5, 50, 95])[1]))
            row[name]["same_bits"] = True if got is None else bool(np.array_equal(got, q[0]))
            got = q[0] if got is None else got
        shapes[str(w)] = row
    out["launch_shapes_Q5_50_95"] = shapes
    eng.close()
    del eng
    torch.cuda.empty_cache()
    # the executable: -w 1000 with and without -quantile 50 on a generated BAM
    gen, cli = os.path.join(ROOT, "tools", "bamgen"), os.path.join(ROOT, "pandepth_amd", "pandepth")
    if a.e2e_records > 0 and os.access(gen, os.X_OK) and os.access(cli, os.X_OK):
        with tempfile.TemporaryDirectory() as td:
            bam = os.path.join(td, "w.bam")
            g = subprocess.run([gen, "-o", bam, "-n", str(int(a.e2e_records)), "-t", "16"], check=True, stderr=subprocess.PIPE, timeout=900)
            e2e = {"bam": g.stderr.decode().strip().replace("bamgen: ", "")}
            for label, extra in (("plain", []), ("quantile_50", ["-quantile", "50"]), ("quantile_5_25_50_75_95", ["-quantile", "5,25,50,75,95"])):
                best = None
                for rep in range(2):
                    t0 = time.perf_counter()
                    p = subprocess.run([cli, "-i", bam, "-w", "1000", "-o", os.path.join(td, label), "-t", "16"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                       env=dict(os.environ, PANDEPTH_TIMING="1"), timeout=600)
                    wall = time.perf_counter() - t0
                    assert p.returncode == 0, p.stderr.decode()[-400:]
                    marks = [ln.strip() for ln in p.stderr.decode().splitlines() if "depth quantiles" in ln or "scan + statistics" in ln]
                    if best is None or wall < best[0]:
                        best = (wall, marks)
                e2e[label] = {"wall_s": round(best[0], 3), "timing_marks": best[1]}
            e2e["tables_identical"] = open(os.path.join(td, "plain.win.stat.gz"), "rb").read() == open(os.path.join(td, "quantile_50.win.stat.gz"), "rb").read()
            out["executable_w1000"] = e2e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
