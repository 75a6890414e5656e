"""Periodic MAC loop (Taylor-Green, rmt_mac_per_steps) on one GPU: ms per step.
    python tools/macp_bench.py [N] [steps] [--integrator explicit|imex] [--fused 0,1]
                               [--repeats 5] [--warmup 20]
One JSON line per repeat and setting of macp_fused; several settings (--fused 0,1) alternate
within each repeat, each on a simulation and context of its own.  A timing is `steps` steps
between two HIP events, after `warmup` steps; leave profilers off for it."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyrmt_amd.mac import MacTaylorGreen

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=1024)
ap.add_argument("steps", nargs="?", type=int, default=200)
ap.add_argument("--integrator", default="explicit")
ap.add_argument("--fused", default="0,1")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()

nu = 0.05
dx = 2 * np.pi / a.N
dt = min(2e-4, 0.1 * dx * dx / nu)      # inside the explicit viscous limit at every N
sims = {int(f): MacTaylorGreen(a.N, nu, dt, a.integrator, options={"macp_fused": int(f)})
        for f in a.fused.split(",")}
for s in sims.values():
    s.step(a.warmup)
torch.cuda.synchronize()
for r in range(a.repeats):
    for f, s in sims.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.step(a.steps)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        print(json.dumps({"N": a.N, "integrator": s.integrator, "macp_fused": f, "repeat": r,
                          "steps": a.steps, "ms_per_step": ms,
                          "cell_updates_per_s": a.N * a.N / ms * 1e3,
                          "umax": float(s.u.abs().max())}), flush=True)
