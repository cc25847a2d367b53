"""Cost of the depth distribution (-dist) on the bench's sample: the fused histogram sweep (pd_scan_depth_histogram,
k_sweep_hist) against the fused window sweep on the same cells (pd_scan_reduce_windows with the 10 Mb bins of whole-chromosome
mode, k_sweep<false, true, false>), for several bin counts and the four LDS forms of the kernels (pd_set_param "hist_variant":
bit 0 = one counter copy per workgroup instead of one per wave, bit 1 = no folding of equal neighbours); then the histogram over
the materialised depth (pd_depth_histogram: whole contigs, and 200 000 exon-sized regions).

    python tools/dist_bench.py [--records 1e9] [--reps 5]          (under rocprofv3 --kernel-trace --stats for the kernel table)

Times are device time between events around each call's kernel (pd_profile); bytes are the 4 B per cell the sweep reads.
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0          # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1.0e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", default="2,201,1001,4097")
    a = ap.parse_args()
    import torch
    import pandepth_amd as pda
    from tools import synth

    dev = torch.device("cuda", 0)
    names, lens = synth.genome_c2()
    first, other = synth.gen_runs_torch(lens, int(a.records), dev, seed=42)
    torch.cuda.synchronize()
    eng = pda.Engine(lens.astype(np.uint32), device=0)
    n_cells = int(eng.device_layout()[0])
    cells = int(lens.sum())
    eng.push_intervals_device(first.data_ptr(), int(first.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
    eng.push_intervals_device(other.data_ptr(), int(other.shape[0]), pda.PD_PUSH_SORTED | pda.PD_PUSH_DISORDER(synth.MAX_SPAN))
    eng.synchronize()

    def timed(name, fn, reps):
        eng.profile(False)
        fn()                                     # warm-up (LDS reservation, scratch)
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

    def rate(ms):
        gbs = n_cells * 4 / (ms / 1e3) / 1e9
        return {"ms": round(ms, 3), "GBps": round(gbs, 1), "frac_peak": round(gbs / PEAK_GBS, 3)}

    out = {"records": int(a.records), "genome_cells": cells, "buffer_cells": n_cells, "reps": a.reps, "timing": "median of reps, device events (pd_profile)"}
    win_ms, _ = timed("scan_reduce_windows", lambda: eng.scan_reduce_windows(10_000_000, 1, 0), a.reps)
    out["window_sweep_10Mb"] = rate(win_ms)
    bins = [int(x) for x in a.bins.split(",")]
    out["fused_histogram"] = {}
    ref = None
    ok = [True]
    for nb in bins:
        row = {}
        for var in range(4):
            eng.set_param("hist_variant", var)
            h = [None]
            ms, _ = timed("scan_depth_histogram", lambda: h.__setitem__(0, eng.scan_depth_histogram(nb, 0)), a.reps)
            if var == 0:
                ref = h[0]
            r = rate(ms)
            # every form must give the same bits, and every contig's row must add up to its length
            r["same_as_per_wave_folded"] = bool(np.array_equal(h[0], ref))
            r["rows_sum_to_lengths"] = bool(np.array_equal(h[0].sum(axis=1), lens.astype(np.uint64)))
            if not (r["same_as_per_wave_folded"] and r["rows_sum_to_lengths"]):
                bad = np.nonzero(h[0].sum(axis=1) != lens.astype(np.uint64))[0]
                r["contigs_off"] = [[int(t), int(h[0][t].sum()) - int(lens[t])] for t in bad[:8]]
                r["entries_differing"] = int((h[0] != ref).sum())
                ok[0] = False
            row[["per_wave_folded", "per_wg_folded", "per_wave_unfolded", "per_wg_unfolded"][var]] = r
        out["fused_histogram"][str(nb)] = row
        if nb == 201:
            tot = ref.sum(axis=0)
            out["depth_mode_201"] = int(np.argmax(tot[1:200])) + 1
            out["cells_by_depth_201"] = {"0": int(tot[0]), "1-199": int(tot[1:200].sum()), ">=200": int(tot[200])}
    eng.set_param("hist_variant", 0)
    eng.scan(0)
    out["depth_histogram_whole"] = {}
    for nb in (201, 1001):
        ms, _ = timed("depth_histogram", lambda: eng.depth_histogram(nb), a.reps)
        out["depth_histogram_whole"][str(nb)] = rate(ms)
    # exome-like targets: 200 000 regions of 200 cells, spread over the genome
    rng = np.random.default_rng(1)
    regs = []
    per = np.maximum(1, (lens / lens.sum() * 200_000).astype(np.int64))
    for t, (ln, k) in enumerate(zip(lens, per)):
        s = np.sort(rng.choice(int(ln) // 400, size=min(int(k), int(ln) // 400), replace=False)) * 400 + 1
        regs.append(np.stack([np.full_like(s, t), s, s + 199], axis=1))
    regs = np.concatenate(regs).astype(np.int32)
    ms, _ = timed("depth_histogram_regions", lambda: eng.depth_histogram(1001, regs), a.reps)
    out["depth_histogram_regions"] = {"regions": int(regs.shape[0]), "cells": int(regs.shape[0]) * 200, "ms": round(ms, 3)}
    ok_after = np.array_equal(eng.depth_histogram(201).sum(axis=1), lens.astype(np.uint64))
    out["all_forms_agree_and_add_up"] = bool(ok[0] and ok_after)
    eng.close()
    print(json.dumps(out))
    if not out["all_forms_agree_and_add_up"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
