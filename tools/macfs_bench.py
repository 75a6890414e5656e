"""The free-slip MAC loop (mac_disc_in_tg_convergence.py, one disc in the Taylor-Green
vortex) on one GPU: ms per step of MacDiscTaylorGreen, and of the lid loop with one disc of
the same size and place at the same N beside it (only the predictor's ghosts differ).
    python tools/macfs_bench.py [N ...] [--steps K] [--only freeslip|lid]"""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyrmt_amd.mac import MacDiscTaylorGreen, MacMultiDisc

ap = argparse.ArgumentParser()
ap.add_argument("N", type=int, nargs="*", default=[1024, 4096])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--only", choices=("freeslip", "lid"))
a = ap.parse_args()


def time_loop(sim, K):
    sim.step(2)
    torch.cuda.synchronize()
    t = time.perf_counter()
    sim.step(K)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / K * 1e3


for N in a.N:
    for walls in ("freeslip", "lid"):
        if a.only and a.only != walls:
            continue
        t0 = time.perf_counter()
        sim = (MacDiscTaylorGreen(N) if walls == "freeslip" else
               MacMultiDisc(N, specs=[(0.15, 0.5, 0.7)], mu_s=0.1, eta=0.0))
        init = time.perf_counter() - t0
        ms = time_loop(sim, a.steps)
        d = sim.diagnostics()
        print(json.dumps({"N": N, "walls": walls, "steps": a.steps, "ms_per_step": ms,
                          "init_s": init, "cell_updates_per_s": N * N / ms * 1e3,
                          "minJ": float(d["minJ"][-1]), "maxJ": float(d["maxJ"][-1]),
                          "umax": float(d["umax"][-1]), "cx": d["cx"][-1].tolist()}),
              flush=True)
        del sim
