"""Measurements of DESIGN.md section 16: one JSON line each on stdout, appended to the file
named by RMT_BENCH_OUT when set (profiles/mac_reinit/mac_reinit_bench.jsonl is such a file).
Usage: python tools/bench_mac_reinit.py [multi] [force] [loop]
  multi   N=2048: rmt_advect_sl_rk4_multi on six masked planes against six times
          rmt_advect_sl_rk4 + rmt_mask_solid, alternating in one process, device events
  force   N=2048: rmt_mac_total_force against its unfused composition
  loop    N=1024: MacReinitDisc ms / step and the share of its three extrapolations
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pyrmt_amd  # noqa: E402
from pyrmt_amd import _lib as L, functions as F, mac as M  # noqa: E402
from _bench import emit, timed  # noqa: E402
from mac_faces_np import faces_of_stress  # noqa: E402


def state(N):
    """A MacReinitDisc state some steps in (Fs != I, a real velocity), as device tensors."""
    sim = M.MacReinitDisc(N, reinit_J=1.02)
    sim.step(8)
    return sim


def bench_multi(N=2048, reps=15):
    sim = state(N)
    ctx, lib = sim.ctx, L.lib()
    u, v = sim.u, sim.v
    a = (0.5 * (u[:, :-1] + u[:, 1:])).contiguous(); b = (0.5 * (v[:-1, :] + v[1:, :])).contiguous()
    qs = [sim.X1, sim.X2] + sim.Fs
    phi = sim.phi
    outs = [torch.empty_like(q) for q in qs]
    outs1 = [torch.empty_like(q) for q in qs]
    dt, dx = sim.dt, sim.dx
    p = F._p

    def multi():
        F._advect_sl_rk4_multi(ctx, qs, a, b, sim.Xg, sim.Yg, dt, dx, dx, phi, outs)

    def six():
        h = ctx.bind()
        for q, o in zip(qs, outs1):
            lib.rmt_advect_sl_rk4(h, p(q), p(a), p(b), p(sim.Xg), p(sim.Yg), dt, dx, dx, p(o))
            lib.rmt_mask_solid(h, p(o), p(phi), p(o))

    t_multi, t_six = timed(multi, reps, six)
    same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(outs, outs1))
    cell = N * N * 8
    emit(what="multi", N=N, reps=reps, ms_multi=t_multi, ms_six_single=t_six,
         speedup=t_six / t_multi, same_bits=bool(same), model_planes_multi=17, model_planes_six=54,
         model_GBps_multi=17 * cell / t_multi / 1e6)
    return sim


def bench_force(sim, reps=15):
    N, dx = sim.N, sim.dx
    X1, X2, Fs, phi = sim.X1, sim.X2, sim.Fs, sim.phi

    def fused():
        return M.total_force(X1, X2, Fs, phi, dx, dx, sim.w_t, sim.mu_s)

    def unfused():
        Sxx, Sxy, Syy, J = M.total_stress(X1, X2, Fs, phi, dx, dx, sim.w_t, sim.mu_s)
        return (*faces_of_stress(F, Sxx, Sxy, Syy, dx, dx), J)

    t_f, t_u = timed(fused, reps, unfused)
    r0, r1 = fused(), unfused()
    same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(r0, r1))
    nbytes = (7 * N * N + N * (N + 1) + (N + 1) * N + N * N) * 8
    emit(what="force", N=N, reps=reps, ms_fused=t_f, ms_unfused=t_u, speedup=t_u / t_f,
         same_bits=bool(same), algorithmic_bytes=nbytes, GBps_fused=nbytes / t_f / 1e6)


def bench_loop(N=1024, warm=5, steps=20):
    sim = M.MacReinitDisc(N, reinit_J=1.8)
    sim.step(warm)
    spans, orig = [], M.extrapolate_reference_map

    def tapped(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = orig(*a); e1.record()
        spans.append((e0, e1))
        return out

    M.extrapolate_reference_map = tapped
    try:
        torch.cuda.synchronize()
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter(); s0.record()
        sim.step(steps)
        s1.record(); torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        M.extrapolate_reference_map = orig
    ext = sum(a.elapsed_time(b) for a, b in spans)
    dev = s0.elapsed_time(s1)
    emit(what="loop", N=N, steps=steps, ms_per_step_wall=wall / steps, ms_per_step_device=dev / steps,
         extrapolations_per_step=len(spans) / steps, ms_extrapolations_per_step=ext / steps,
         extrapolation_share=ext / dev, n_reinit=sim.n_reinit, diverged=sim.diverged)


if __name__ == "__main__":
    what = sys.argv[1:] or ["multi", "force", "loop"]
    sim = None
    if "multi" in what:
        sim = bench_multi()
    if "force" in what:
        bench_force(sim or state(2048))
    if "loop" in what:
        bench_loop()
