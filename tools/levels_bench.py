"""Cost of the depth levels (-levels) on the bench's sample: pd_depth_levels over whole contigs (k_levels count, k_levels_scan,
k_levels emit; chunks of at most 2^24 cells, as the executable walks them) with the edges 0,1,5,15 and in exact mode, against
the yardstick that reads the same 4 B per cell of the same materialised depth once: pd_depth_histogram over whole contigs
(k_sweep_hist from depth).  The quantised call reads the cells in the count pass and again, for the waves in which a run opens,
in the emit pass, and writes 8 B per run.

    python tools/levels_bench.py [--records 1e9] [--reps 5]        (under rocprofv3 --kernel-trace --stats for the kernel table)

Times are device time between events around each call's kernels (pd_profile), summed over the calls of one walk of the genome;
bytes are the 4 B per cell of one read of the depth.  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0          # MI355X HBM3E
CHUNK = 1 << 24            # the executable's default (-X levels_chunk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1.0e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", default="0,1,5,15")
    a = ap.parse_args()
    import torch
    import pandepth_amd as pda
    from tools import synth

    dev = torch.device("cuda", 0)
    names, lens = synth.genome_c2()
    first, other = synth.gen_runs_torch(lens, int(a.records), dev, seed=42)
    torch.cuda.synchronize()
    eng = pda.Engine(lens.astype(np.uint32), device=0)
    cells = int(lens.sum())
    eng.push_intervals_device(first.data_ptr(), int(first.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
    eng.push_intervals_device(other.data_ptr(), int(other.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_DISORDER(synth.MAX_SPAN))
    eng.synchronize()
    del first, other
    eng.scan(0)

    def timed(name, fn, reps):
        eng.profile(False)
        fn()                                     # warm-up (scratch)
        eng.profile(True)
        ms = []
        for _ in range(reps):
            before = eng.profile_get(name)
            fn()
            after = eng.profile_get(name)
            ms.append(after[0] - before[0])
        eng.profile(False)
        ms.sort()
        return ms[len(ms) // 2], ms

    def rate(ms, passes=1.0):
        gbs = cells * 4 * passes / (ms / 1e3) / 1e9
        return {"ms": round(ms, 3), "GBps_one_read": round(cells * 4 / (ms / 1e3) / 1e9, 1), "frac_peak_one_read": round(cells * 4 / (ms / 1e3) / 1e9 / PEAK_GBS, 3),
                "passes_over_the_cells": passes, "frac_peak_bytes_moved": round(gbs / PEAK_GBS, 3)}

    edges = [int(x) for x in a.edges.split(",")]
    count = {}

    def walk(ed, key):
        n_runs = calls = 0
        for t, ln in enumerate(lens):
            for beg in range(0, int(ln), CHUNK):
                n = min(CHUNK, int(ln) - beg)
                n_runs += eng.depth_levels(t, beg, n, ed).shape[0]
                calls += 1
        count[key] = (n_runs, calls)

    out = {"records": int(a.records), "genome_cells": cells, "reps": a.reps, "chunk_cells": CHUNK, "edges": edges,
           "timing": "median of reps, device events (pd_profile), summed over the calls of one walk of every contig"}
    h_ms, _ = timed("depth_histogram", lambda: eng.depth_histogram(201), a.reps)
    out["depth_histogram_201"] = rate(h_ms)
    q_ms, _ = timed("depth_levels", lambda: walk(edges, "q"), a.reps)
    x_ms, _ = timed("depth_levels", lambda: walk(None, "x"), max(1, min(a.reps, 3)))
    q_runs, calls = count["q"]
    x_runs, _ = count["x"]
    # bytes per cell: 4 for the count pass, 4 more for every wave (2048 cells) the emit pass loads, 8 per run written and copied
    out["levels_quantised"] = dict(rate(q_ms), runs=q_runs, calls=calls, ratio_to_histogram=round(q_ms / h_ms, 3), runs_per_kilobase=round(q_runs * 1e3 / cells, 4),
                                   bytes_per_cell_at_most=round(8 + 8.0 * q_runs / cells, 3))
    out["levels_exact"] = dict(rate(x_ms), runs=x_runs, calls=calls, ratio_to_histogram=round(x_ms / h_ms, 3), runs_per_kilobase=round(x_runs * 1e3 / cells, 2),
                               bytes_per_cell_at_most=round(8 + 8.0 * x_runs / cells, 3))
    out["quantised_within_2p5x_of_histogram"] = bool(q_ms <= 2.5 * h_ms)
    # correctness of what was timed, on one contig: numpy run-finding on the cells read back
    t = int(np.argmin(lens))
    d = eng.read_depth(t, 0, int(lens[t])).astype(np.int64)
    for ed, key in ((edges, "quantised"), (None, "exact")):
        cls = d if ed is None else np.searchsorted(np.asarray(ed, dtype=np.int64), d, side="right") - 1
        idx = np.nonzero(np.concatenate([[True], cls[1:] != cls[:-1]]))[0]
        ref = np.stack([idx, cls[idx] & 0xFFFFFFFF], axis=1).astype(np.uint32)
        got = np.concatenate([eng.depth_levels(t, b, min(CHUNK, int(lens[t]) - b), ed) for b in range(0, int(lens[t]), CHUNK)])
        keep = np.concatenate([[True], got[1:, 1] != got[:-1, 1]])           # (chunk seams)
        out["smallest_contig_equals_numpy_" + key] = bool(np.array_equal(got[keep], ref))
    eng.close()
    print(json.dumps(out))
    if not (out["smallest_contig_equals_numpy_quantised"] and out["smallest_contig_equals_numpy_exact"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
