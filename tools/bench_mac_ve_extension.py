"""Measurements of DESIGN.md section 19: one JSON line each on stdout, appended to the file
named by RMT_BENCH_OUT when set (profiles/ve_extension/bench.jsonl is such a file).
Usage: python tools/bench_mac_ve_extension.py [N ...]        (default 128 512)
For each N and each integrator of the ladder, a MacViscoelasticExtension(N, tau=0.5) at the
short step 0.2 dx^2 / mu_f (stable for all three) is advanced 10 steps, then
  ms_per_step   wall time of 20 further steps with their host reads, over 20
  phases        the median device-event ms of each phase of the step, run by itself on the
                state reached (the state does not advance): kinematics, phi + advection, the
                three extrapolations, log-conformation + sym_exp, face force, predictor, lock,
                projection, record
  extrap_share  the three extrapolations' share of the phases' sum
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import pyrmt_amd  # noqa: E402,F401
from pyrmt_amd import _lib as L, mac as M  # noqa: E402
from pyrmt_amd.functions import (_advect_sl_rk4_multi, _p, _plane_ptrs,  # noqa: E402
                                 extrapolate_reference_map)
from _bench import emit, timed  # noqa: E402

MU_F, WARM, STEPS, REPS = 0.05, 10, 20, 15


def phases(sim):
    lib, N, dx, dy, rho, dt = L.lib(), sim.N, sim.dx, sim.dy, sim.rho, sim.dt
    n, at = N * N, (N // 2) * N + N // 2
    kin, be, ff, star = sim.kin, sim.be, sim.ff, sim.star
    Lp = _plane_ptrs([kin[2], kin[3], kin[4], kin[5]])
    bp = _plane_ptrs([be[0], be[1], be[2]])
    phi = sim.phi.clone()
    qs = [sim.X1, sim.X2] + sim.psi
    outs = [torch.empty_like(q) for q in qs]
    psi = [p.clone() for p in sim.psi]
    pp = _plane_ptrs(psi)
    us, vs = star[0], star[1]
    u2, v2, p2 = (torch.empty_like(sim.u) for _ in range(3))
    mode = M.VE_LOCK_MODES[sim.integrator]
    c = sim.ctx.bind

    def advect():
        lib.rmt_rebuild_phi_disc(c(), _p(sim.X1), _p(sim.X2), 0.5, 0.5, sim.R, _p(phi))
        _advect_sl_rk4_multi(sim.ctx, qs, kin[0], kin[1], sim.Xg, sim.Yg, dt, dx, dy, phi, outs)

    def extrap():
        extrapolate_reference_map(outs[0], outs[1], phi, dx, dy, sim.LAYERS)
        extrapolate_reference_map(outs[2], outs[3], phi, dx, dy, sim.LAYERS)
        extrapolate_reference_map(outs[4], sim.zero, phi, dx, dy, sim.LAYERS)

    def logconf():
        lib.rmt_ve_logconf_steps(c(), n, _plane_ptrs(sim.psi), Lp, sim.tau, dt, 1, int(sim.imex), pp)
        lib.rmt_ve_sym_exp(c(), n, pp, bp)

    def predictor():
        if sim.elastic:
            c_el = dt * dt * (sim.G / rho)
            lib.rmt_mac_per_predictor_imex_elastic(
                c(), _p(sim.u), _p(sim.v), 2 * dx, 2 * dy, dx**2, dy**2, dt, c_el,
                dt * sim.nu + c_el, float(rho), _p(ff[4]), _p(ff[0]), _p(ff[1]), M._hp(sim.lx),
                M._hp(sim.ly), _p(us), _p(vs))
        elif sim.imex:
            lib.rmt_mac_per_predictor_imex(c(), _p(sim.u), _p(sim.v), 2 * dx, 2 * dy, dt,
                                           dt * sim.nu, M._hp(sim.lx), M._hp(sim.ly), _p(us),
                                           _p(vs))
        else:
            lib.rmt_mac_per_predictor(c(), _p(sim.u), _p(sim.v), float(sim.nu), dx**2, dy**2,
                                      2 * dx, 2 * dy, dt, _p(us), _p(vs))

    def lock():
        for s, w, f, H, mill in ((us, sim.u, ff[0], ff[2], sim.u_mill),
                                 (vs, sim.v, ff[1], ff[3], sim.v_mill)):
            lib.rmt_mac_ve_lock(c(), mode, n, _p(s), _p(w), _p(f), _p(H), _p(mill), dt, sim.BETA,
                                float(rho), _p(s))

    table = {
        "kinematics": lambda: lib.rmt_mac_ve_centre_kinematics(
            c(), _p(sim.u), _p(sim.v), dx, dy, _p(kin[0]), _p(kin[1]), Lp),
        "phi_advection": advect, "extrapolations": extrap, "logconf_symexp": logconf,
        "face_force": lambda: lib.rmt_mac_ve_face_force(
            c(), bp, _p(phi), float(sim.G), sim.w_t, dx, dy, *[_p(ff[k]) for k in range(5)]),
        "predictor": predictor, "lock": lock,
        "projection": lambda: lib.rmt_mac_per_project(
            c(), _p(us), _p(vs), dx, dy, float(rho / dt), float(dt / rho), M._hp(sim.lx),
            M._hp(sim.ly), _p(u2), _p(v2), _p(p2)),
        "record": lambda: lib.rmt_mac_ve_record(c(), n, bp, _p(phi), _p(sim.u), at,
                                                _p(sim.stats)),
    }
    return {k: timed(f, REPS) for k, f in table.items()}


def bench(N):
    for name in M.INTEGRATORS:
        dt = 0.2 * (1.0 / N) ** 2 / MU_F
        sim = M.MacViscoelasticExtension(N, tau=0.5, mu_f=MU_F, integrator=name, dt=dt)
        sim.step(WARM)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.step(STEPS)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / STEPS
        ph = phases(sim)
        total = sum(ph.values())
        emit(what="ve_extension_step", N=N, integrator=name, dt=dt, steps=STEPS,
             ms_per_step=ms, phases_ms=ph, phases_sum_ms=total,
             extrap_share=ph["extrapolations"] / total, stopped=sim.stopped)


if __name__ == "__main__":
    for N in [int(a) for a in sys.argv[1:]] or [128, 512]:
        bench(N)
