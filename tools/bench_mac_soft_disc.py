"""Measurements of DESIGN.md section 17: one JSON line each on stdout, appended to the file
named by RMT_BENCH_OUT when set (profiles/mac_soft_disc/mac_soft_disc_bench.jsonl is such a file).
Usage: python tools/bench_mac_soft_disc.py [loop] [force] [sl] [N ...]      (N: 256 1024)
  loop    MacSoftDisc ms / step and the steps to t_end = 1 of explicit, imex and imex-elastic at
          their default dt and of imex-sl at 5 x the explicit dt, from a state 20 steps in
  force   rmt_mac_solid_force against its unfused composition, alternating in one process,
          device events
  sl      imex-sl at 5 x the explicit dt run to t_end = 1 (N <= 256): the steps that took the
          semi-Lagrangian branch, and the largest advective CFL the run could reach
"""
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pyrmt_amd  # noqa: E402,F401
from pyrmt_amd import functions as F, mac as M  # noqa: E402
from _bench import emit, timed  # noqa: E402
from mac_faces_np import faces_of_stress  # noqa: E402

T_END = 1.0


def rungs(N):
    dt_exp = M.MacSoftDisc.default_dt(N, "explicit")
    return (("explicit", None), ("imex", None), ("imex-elastic", None), ("imex-sl", 5.0 * dt_exp))


def bench_loop(N, warm=20, steps=40):
    for name, dt in rungs(N):
        sim = M.MacSoftDisc(N, integrator=name, dt=dt)
        sim.step(warm)
        torch.cuda.synchronize()
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter(); s0.record()
        sim.step(steps)
        s1.record(); torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / steps
        n_end = math.ceil(T_END / sim.dt)
        emit(what="loop", N=N, integrator=sim.integrator, dt=sim.dt, steps=steps,
             ms_per_step_wall=wall, ms_per_step_device=s0.elapsed_time(s1) / steps,
             steps_to_t_end=n_end, s_to_t_end=n_end * wall / 1e3, pcg_iters=list(sim.pcg_iters),
             sl_steps=sim.sl_steps, cfl_bound=sim.dt * sim.U_LID / sim.dx, diverged=sim.diverged)


def bench_force(N, reps=15):
    sim = M.MacSoftDisc(N, integrator="explicit")
    sim.step(20)
    dx, X1, X2, phi = sim.dx, sim.X1, sim.X2, sim.phi

    def fused():
        return M.solid_force(X1, X2, phi, dx, dx, sim.w_t, sim.mu_s)

    def unfused():
        sxx, sxy, syy, J = F.solid_cauchy_stress(X1, X2, dx, dx, sim.mu_s, 0.0, phi)
        H = F.smoothed_heaviside(phi, sim.w_t)
        Sxx = (1 - H) * sxx; Sxy = (1 - H) * sxy; Syy = (1 - H) * syy
        return (*faces_of_stress(F, Sxx, Sxy, Syy, dx, dx), J)

    t_f, t_u = timed(fused, reps, unfused)
    r0, r1 = fused(), unfused()
    same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(r0, r1))
    nbytes = (3 * N * N + N * (N + 1) + (N + 1) * N + N * N) * 8
    emit(what="force", N=N, reps=reps, ms_fused=t_f, ms_unfused=t_u, speedup=t_u / t_f,
         same_bits=bool(same), algorithmic_bytes=nbytes, GBps_fused=nbytes / t_f / 1e6)


def bench_sl(N):
    dt = 5.0 * M.MacSoftDisc.default_dt(N, "explicit")
    t0 = time.perf_counter()
    traj, sim = M.mac_soft_disc_run(N, T_END, integrator="imex-sl", dt=dt, return_sim=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    cfl = dt * max(float(sim.u.abs().max()) / sim.dx, float(sim.v.abs().max()) / sim.dy)
    emit(what="sl", N=N, dt=dt, steps=len(traj), sl_steps=sim.sl_steps, s_wall=wall,
         cfl_last=cfl, cfl_bound=dt * sim.U_LID / sim.dx, cfl_switch=0.9, diverged=sim.diverged,
         t=float(traj[-1, 0]), cx=float(traj[-1, 1]), cy=float(traj[-1, 2]))


if __name__ == "__main__":
    args = sys.argv[1:]
    sizes = [int(a) for a in args if a.isdigit()] or [256, 1024]
    what = [a for a in args if not a.isdigit()] or ["loop", "force", "sl"]
    for N in sizes:
        if "loop" in what:
            bench_loop(N)
        if "force" in what:
            bench_force(N)
        if "sl" in what and N <= 256:
            bench_sl(N)
