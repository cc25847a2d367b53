"""Cost of the GC-bias pass (-gcbias) on the bench's sample with a synthetic reference of the genome's size: pd_depth_gc_bias at
W = 100 and W = 1000 beside pd_depth_histogram over the same cells in the same run — the histogram reads the same 4 bytes per cell,
this pass 5, so at equal efficiency it takes 1.25 times as long — and the two launch shapes against each other.

    python tools/gcbias_bench.py [--records 1e9] [--reps 5] [--out profiles/gcbias_bench.json]
    python tools/gcbias_bench.py --cli SAMPLE.bam REF.fa [--rounds 5]      # the executable: with / without -gcbias, alternating
    python tools/gcbias_bench.py --cli-gen 2e7 [--rounds 5]                # the same on a BAM made by tools/bamgen and a synthetic FASTA for its contigs

Kernel times are device time between events around each launch (pd_profile), summed over the pieces of a call; `call_ms` is the
host's clock around the whole call (staging the bases, the copies, the kernels, the results back).  Prints one JSON object."""
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

PEAK_GBPS = 8000.0


def synthetic_bases(n, seed=7, block=1 << 26):
    """n bases: a 64 MiB block of ACGT (GC share drifting from 256 bases to the next, a lower-case stretch, an N every 2^16 bases
    or so) repeated — the kernel's work does not depend on what the valid bases are"""
    rng = np.random.default_rng(seed)
    m = min(n, block)
    p_gc = np.clip(0.41 + 0.12 * rng.standard_normal((m + 255) // 256), 0.05, 0.95).repeat(256)[:m]
    gc = rng.random(m) < p_gc
    pick = rng.integers(0, 2, m)
    b = np.where(gc, np.frombuffer(b"CG", dtype=np.uint8)[pick], np.frombuffer(b"AT", dtype=np.uint8)[pick]).astype(np.uint8)
    b[m // 3:m // 3 + (1 << 16)] |= 0x20
    b[rng.integers(0, m, max(1, m >> 16))] = ord("N")
    return np.tile(b, (n + m - 1) // m)[:n]


def engine_part(a):
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
    genome = synthetic_bases(cells)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = [genome[off[t]:off[t + 1]] for t in range(len(lens))]

    def timed(names_, fn, bytes_per_cell):
        eng.profile(False)
        fn()                                     # warm-up (scratch, code objects)
        eng.profile(True)
        rows = []
        for _ in range(a.reps):
            before = [eng.profile_get(n) for n in names_]
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            after = [eng.profile_get(n) for n in names_]
            rows.append((sum(x[0] - y[0] for x, y in zip(after, before)), wall, sum(x[1] - y[1] for x, y in zip(after, before))))
        eng.profile(False)
        rows.sort(key=lambda r: r[0])
        k, wall, launches = rows[len(rows) // 2]
        gbps = cells * bytes_per_cell / (k / 1e3) / 1e9 if k else None
        return {"kernel_ms": round(k, 3), "kernel_ms_min_max": [round(rows[0][0], 3), round(rows[-1][0], 3)], "launches": int(launches), "call_ms": round(wall, 1),
                "bytes_per_cell": bytes_per_cell, "GBps": round(gbps, 1) if gbps else None, "of_peak": round(gbps / PEAK_GBPS, 3) if gbps else None}

    out = {"records": int(a.records), "genome_cells": cells, "reps": a.reps, "peak_GBps": PEAK_GBPS,
           "timing": "median of reps after one warm-up; device events (pd_profile) summed over the pieces, and the host clock around the call"}
    hist = timed(["depth_histogram"], lambda: eng.depth_histogram(64), 4)
    out["depth_histogram_64"] = hist
    for w in (100, 1000):
        res = [None]
        row = timed(["gc_bias"], lambda: res.__setitem__(0, eng.depth_gc_bias(w, bases)), 5)
        row["x_histogram"] = round(row["kernel_ms"] / hist["kernel_ms"], 3)
        row["windows"], row["skipped"] = int(res[0][0].sum()), res[0][2]
        row["bins_in_use"] = int((res[0][0] > 0).sum())
        shapes = {}
        for name, wm in (("lanes", 1 << 20), ("workgroup", 0)):
            eng.set_param("gcbias_wave_max", wm)
            got = [None]
            shapes[name] = timed(["gc_bias"], lambda: got.__setitem__(0, eng.depth_gc_bias(w, bases)), 5)
            shapes[name]["same_numbers"] = bool(np.array_equal(got[0][0], res[0][0]) and np.array_equal(got[0][1], res[0][1]) and got[0][2] == res[0][2])
        eng.set_param("gcbias_wave_max", 4096)
        row["launch_shapes"] = shapes
        out["gc_bias_W%d" % w] = row
    eng.close()
    return out


def cli_part(a):
    """the executable with and without -gcbias W, alternating; PANDEPTH_TIMING's phase lines give the split"""
    exe = os.path.join(ROOT, "pandepth_amd", "pandepth")
    bam, fasta = a.cli
    out = {"input": os.path.basename(bam), "rounds": a.rounds}

    def once(extra):
        with tempfile.TemporaryDirectory() as td:
            t0 = time.perf_counter()
            p = subprocess.run([exe, "-i", bam, "-o", os.path.join(td, "o"), "-t", "16"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env=dict(os.environ, PANDEPTH_TIMING="1"))
            wall = time.perf_counter() - t0
            assert p.returncode == 0, p.stderr.decode()[-400:]
            phases = {ln[9:38].strip(): float(ln[38:47]) for ln in p.stderr.decode().splitlines() if ln.startswith("[timing] ") and " s   (total" in ln}
            return wall, phases

    for w in (100, 1000):
        arms = {"without": [], "with": ["-r", fasta, "-gcbias", str(w)], "with_host": ["-r", fasta, "-gcbias", str(w), "-X", "gcbias_device=0"]}
        walls = {k: [] for k in arms}
        phase = {k: {} for k in arms}
        for _ in range(a.rounds):
            for k, extra in arms.items():
                wall, ph = once(extra)
                walls[k].append(wall)
                for n, v in ph.items():
                    phase[k].setdefault(n, []).append(v)
        out["W%d" % w] = {k: {"wall_s_min_median_max": [round(min(v), 3), round(float(np.median(v)), 3), round(max(v), 3)],
                              "phases_median_s": {n: round(float(np.median(x)), 3) for n, x in phase[k].items()}} for k, v in walls.items()}
    return out


def generate(records, td):
    """a BAM of tools/bamgen and a FASTA of synthetic bases for its contigs (names and lengths from the executable's own chr table)"""
    import gzip
    bam, fasta = os.path.join(td, "s.bam"), os.path.join(td, "s.fa")
    subprocess.run([os.path.join(ROOT, "tools", "bamgen"), "-o", bam, "-n", str(int(records)), "-t", "16"], check=True, stderr=subprocess.PIPE)
    subprocess.run([os.path.join(ROOT, "pandepth_amd", "pandepth"), "-i", bam, "-o", os.path.join(td, "hdr"), "-t", "16"], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    rows = [ln.split("\t") for ln in gzip.open(os.path.join(td, "hdr.chr.stat.gz"), "rt") if not ln.startswith("#")]
    with open(fasta, "wb") as f:
        for k, r in enumerate(rows):
            f.write(b">" + r[0].encode() + b"\n" + synthetic_bases(int(r[1]), seed=k).tobytes() + b"\n")
    return bam, fasta, sum(int(r[1]) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1.0e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli", nargs=2, metavar=("BAM", "FASTA"))
    ap.add_argument("--cli-gen", type=float, metavar="RECORDS")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.cli_gen:
        with tempfile.TemporaryDirectory() as td:
            bam, fasta, cells = generate(a.cli_gen, td)
            a.cli = (bam, fasta)
            out = dict(cli_part(a), records=int(a.cli_gen), genome_cells=cells)
    else:
        out = cli_part(a) if a.cli else engine_part(a)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
