"""Measurements of DESIGN.md section 18: one JSON line each on stdout, appended to the file
named by RMT_BENCH_OUT when set (profiles/viscoelastic/ve_bench.jsonl is such a file).
Usage: python tools/bench_viscoelastic.py [steps] [tg] [loop]
  steps   N = 1024 and 4096: one explicit and one Strang log-conformation step (device events,
          ms and the algorithmic 10 planes x 8 B a cell over it), and 50 steps in one launch
          against 50 launches of one step, alternating in one process
  tg      tg_run_compare(64, dt=5e-3): wall time of both 400-step runs and the three numbers,
          beside the reference's NumPy time for the same call (REF_TG_SECONDS, taken once on
          the development host's CPU)
  loop    UniformExtension(96): ms / step over 40 steps after 5
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pyrmt_amd  # noqa: E402,F401
from pyrmt_amd import _lib as L, functions as F, viscoelastic as VE  # noqa: E402
from _bench import emit, timed  # noqa: E402
import viscoelastic_np as V  # noqa: E402

# the reference's run_compare(64, 0.5, 5e-3, 2.0) in NumPy: 0.93 s and 0.84 s in two runs
REF_TG_SECONDS = 0.84


def bench_steps(N, reps, fused=50, tau=0.5, dt=5e-3):
    lib, ctx, n = L.lib(), F.ctx_for(N, N), N * N
    Lc = [torch.from_numpy(a.copy()).cuda() for a in V.tg_velocity_gradient(N)]
    p0 = VE.logconf_local_step(*[torch.zeros((N, N), dtype=torch.float64, device="cuda")] * 3,
                               *Lc, tau, dt, nsteps=20)      # a state away from psi = 0
    p0 = [p.clone() for p in p0]
    o1 = [torch.empty_like(p) for p in p0]
    o2 = [torch.empty_like(p) for p in p0]
    ip, Lp, op1, op2 = map(F._plane_ptrs, (p0, Lc, o1, o2))

    def steps(k, strang, op):
        return lambda: lib.rmt_ve_logconf_steps(ctx.bind(), n, ip, Lp, tau, dt, k, strang, op)

    def singles(strang):
        def run():
            h = ctx.bind()
            lib.rmt_ve_logconf_steps(h, n, ip, Lp, tau, dt, 1, strang, op2)
            for _ in range(fused - 1):
                lib.rmt_ve_logconf_steps(h, n, op2, Lp, tau, dt, 1, strang, op2)
        return run

    nbytes = 10 * 8 * n
    for strang in (0, 1):
        name = "strang" if strang else "explicit"
        t1 = timed(steps(1, strang, op1), 4 * reps)
        t_f, t_s = timed(steps(fused, strang, op1), reps, singles(strang))
        same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(o1, o2))
        emit(what="steps", stepper=name, N=N, reps=reps, ms_single_step=t1,
             algorithmic_bytes=nbytes, GBps_single_step=nbytes / t1 / 1e6, fused=fused,
             ms_per_step_fused=t_f / fused, ms_per_step_single_launches=t_s / fused,
             speedup=t_s / t_f, fused_no_slower=bool(t_f <= t_s), same_bits=bool(same))


def bench_tg():
    VE.tg_run_compare(16, 0.5, 5e-3, 0.25)      # warm-up: code objects, the context
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = VE.tg_run_compare(64, 0.5, 5e-3, 2.0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    emit(what="tg_run_compare", N=64, tau=0.5, dt=5e-3, T=2.0, seconds_wall=wall, diff=res[0],
         min_eig_explicit=res[1], min_eig_strang=res[2], reference_numpy_seconds=REF_TG_SECONDS,
         reference_numpy_host="the development host's CPU, one run")


def bench_loop(N=96, warm=5, steps=40):
    sim = VE.UniformExtension(N)
    sim.step(warm)
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter(); s0.record()
    sim.step(steps)
    s1.record(); torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    emit(what="loop", N=N, steps=steps, ms_per_step_wall=wall / steps,
         ms_per_step_device=s0.elapsed_time(s1) / steps, t=sim.t, lam_max=sim.record[-1][1],
         bxx_centre=sim.record[-1][2], stopped=sim.stopped)


if __name__ == "__main__":
    what = sys.argv[1:] or ["steps", "tg", "loop"]
    if "steps" in what:
        bench_steps(1024, reps=10)
        bench_steps(4096, reps=5)
    if "tg" in what:
        bench_tg()
    if "loop" in what:
        bench_loop()
