"""The bench step on the compact sample only (pd_runs_create, then three direct window calls: k_direct_c8 and the pile-up pass), for rocprofv3 --pmc passes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import pandepth_amd as pda
from tools import synth

R = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 9
dev = torch.device("cuda", 0)
names, lens = synth.genome_c2()
first, other = synth.gen_runs_torch(lens, R, dev, seed=42)
torch.cuda.synchronize()
with pda.Engine(lens.astype(np.uint32), device=0) as e:
    e.keep_deferred(True)
    runs = e.runs_create(first.data_ptr(), int(first.shape[0]), other.data_ptr(), int(other.shape[0]))
    for it in range(3):
        e.reset()
        e.push_runs(runs, pda.PD_PUSH_MORE)
        e.scan_reduce_windows(10000000, 1, 0)
    e.reset()
    e.runs_destroy(runs)
print("done")
