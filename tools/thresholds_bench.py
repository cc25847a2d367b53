"""Cost of the threshold counts (-thresholds) on the bench's sample: pd_window_thresholds at w = 1000 and w = 10 000 000 with K = 1,
4 and 16 thresholds, each beside what a user had to do for the same columns before — K calls of pd_reduce_windows with
min_dep = T_j over the same cells (that entry point is untouched by the feature) — then the two launch shapes against each other
at the widths around "threshold_wave_max", and pd_depth_thresholds over one row per contig.

    python tools/thresholds_bench.py [--records 1e9] [--reps 5]

Kernel times are device time between events around each launch (pd_profile), summed over the call's launches; `call_ms` is the
host's clock around the whole call (batches, piece lists, results back).  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["threshold_narrow", "threshold_pieces"]
THR = {1: [10], 4: [1, 10, 20, 30], 16: [1, 2, 3, 5, 8, 10, 15, 20, 25, 30, 40, 50, 60, 80, 100, 200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1.0e9)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import pandepth_amd as pda
    from tools import synth

    dev = torch.device("cuda", 0)
    t_build = time.perf_counter()
    names, lens = synth.genome_c2()
    first, other = synth.gen_runs_torch(lens, int(a.records), dev, seed=42)
    torch.cuda.synchronize()
    eng = pda.Engine(lens.astype(np.uint32), device=0)
    eng.push_intervals_device(first.data_ptr(), int(first.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
    eng.push_intervals_device(other.data_ptr(), int(other.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_DISORDER(synth.MAX_SPAN))
    eng.synchronize()
    eng.scan(0)
    del first, other
    t_build = time.perf_counter() - t_build
    cells = int(lens.sum())

    def timed(names_, fn):
        eng.profile(False)
        fn()                                     # warm-up (scratch)
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

    out = {"records": int(a.records), "genome_cells": cells, "bytes_per_pass": cells * 4, "sample_build_s": round(t_build, 1), "reps": a.reps,
           "timing": "median of reps after one warm-up; device events (pd_profile) and host clock"}
    out["windows"] = {}
    for w in (1000, 10_000_000):
        n = int(eng.window_layout(w)[-1])
        cov, tot = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        row = {"rows": n}
        for K, thr in THR.items():
            def k_calls():
                for t in thr:
                    eng.reduce_windows(w, t, out=(cov, tot))
            base = timed(["reduce_windows"], k_calls)
            cnt = [None]
            one = timed(KERNELS, lambda: cnt.__setitem__(0, eng.window_thresholds(w, thr)[1]))
            eng.reduce_windows(w, thr[-1], out=(cov, tot))
            one["last_column_is_cover"] = bool(np.array_equal(cnt[0][:, -1], cov[:n]))
            one["x_k_calls"] = round(one["kernel_ms"] / base["kernel_ms"], 3)
            row["K%d" % K] = {"reduce_windows_k_calls": base, "thresholds": one}
        out["windows"][str(w)] = row
    shapes = {}
    for w in (256, 1000, 2048, 4096, 16384, 65536, 100000, 262144, 1000000, 10_000_000):
        got, row = None, {}
        for name, wm in (("lanes", 0xFFFFFFFF), ("pieces", 0)):
            eng.set_param("threshold_wave_max", wm)
            cnt = [None]
            row[name] = timed(KERNELS, lambda: cnt.__setitem__(0, eng.window_thresholds(w, THR[4])[1]))
            row[name]["same_bits"] = True if got is None else bool(np.array_equal(got, cnt[0]))
            got = cnt[0] if got is None else got
        shapes[str(w)] = row
    eng.set_param("threshold_wave_max", 65536)
    out["launch_shapes_K4"] = shapes
    segs = np.array([[t, 1, int(ln)] for t, ln in enumerate(lens)], dtype=np.int32)
    roff = np.arange(len(lens) + 1, dtype=np.uint64)
    out["whole_contig_rows_K4"] = dict(timed(KERNELS, lambda: eng.depth_thresholds(segs, roff, THR[4])), rows=len(lens))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
