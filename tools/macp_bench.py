"""Periodic MAC loop (Taylor-Green, rmt_mac_per_steps) on one GPU: ms per step.
    python tools/macp_bench.py [N] [steps] [--integrator explicit|imex] [--fused 0,1]
                               [--repeats 5] [--warmup 20] [--semilag [--cfl 2]]
One JSON line per repeat and setting of macp_fused; several settings (--fused 0,1) alternate
within each repeat, each on a simulation and context of its own.  A timing is `steps` steps
between two HIP events, after `warmup` steps; leave profilers off for it.
--semilag: the semi-Lagrangian loop (rmt_mac_per_steps_sl) at dt = cfl * dx alternates with
the IMEX loop at the default dt instead; the field is set back to t = 0 ahead of every timing,
so that at --cfl 2 every timed step takes the SL branch (sl_steps in the line says how many
did)."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyrmt_amd.mac import MacTaylorGreen, tg_exact

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=1024)
ap.add_argument("steps", nargs="?", type=int, default=200)
ap.add_argument("--integrator", default="explicit")
ap.add_argument("--fused", default="0,1")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--semilag", action="store_true")
ap.add_argument("--cfl", type=float, default=2.0)
a = ap.parse_args()

nu = 0.05
dx = 2 * np.pi / a.N
dt = min(2e-4, 0.1 * dx * dx / nu)      # inside the explicit viscous limit at every N
if a.semilag:
    sims = {"imex": MacTaylorGreen(a.N, nu, dt, "imex"),
            "imex-sl": MacTaylorGreen(a.N, nu, a.cfl * dx, semilag=True)}
else:
    sims = {int(f): MacTaylorGreen(a.N, nu, dt, a.integrator, options={"macp_fused": int(f)})
            for f in a.fused.split(",")}
for s in sims.values():
    s.step(a.warmup)
torch.cuda.synchronize()
for r in range(a.repeats):
    for f, s in sims.items():
        if a.semilag:
            s.set(*tg_exact(*s.faces, nu, 0.0))
            s.sl_steps = 0
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.step(a.steps)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        line = {"N": a.N, "integrator": s.integrator, "macp_fused": f, "repeat": r,
                "steps": a.steps, "ms_per_step": ms, "cell_updates_per_s": a.N * a.N / ms * 1e3,
                "umax": float(s.u.abs().max())}
        if a.semilag:
            line.update({"macp_fused": 0, "loop": f, "dt": s.dt, "sl_steps": s.sl_steps})
        print(json.dumps(line), flush=True)
