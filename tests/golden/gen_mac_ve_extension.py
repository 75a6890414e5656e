"""Golden-vector generator for the four-roll-mill viscoelastic driver: runs the pyRMT reference
(benchmarks/mac_viscoelastic_extension.py and pyRMT/mac.py, imported exactly as gen_golden.py
does) and writes

    tests/golden/mac_ve_extension_ops.npz   the driver's expressions (:106-155, :159-171) and
                                            momentum_predictor_periodic_imex_elastic on
                                            tests/mac_ve_extension_np.py's shared inputs; the
                                            (33, 70) shape keeps the arithmetic results only
    tests/golden/mac_ve_extension_runs.npz  run() on the twelve short configurations and the
                                            large-step one (per-step record, final state), and
                                            the reference's record of the eight N = 40 runs of
                                            its test_ve_imex_fsi.py and test_elastic_imex.py

The loop is not restated here: the driver's own run() is called and its state captured by
wrapping the names the driver module looks up per call.  The operator expressions are the
driver's lines applied to the shared inputs with the reference's functions.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_mac_ve_extension.py [ops] [runs]
"""
import contextlib
import io
import multiprocessing
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import save, M, F, U as UT  # noqa: E402
import numpy as np  # noqa: E402
import benchmarks.mac_viscoelastic_extension as X  # noqa: E402
import mac_ve_extension_np as E  # noqa: E402

ST = np.stack


def ref_ops(g, arith_only):
    """The driver's lines on the shared inputs (reference functions throughout)."""
    dx, dy, dt, rho, beta, G, w_t = E.DX, E.DY, E.DT, E.RHO, E.BETA, E.G, E.W_T
    u, v = g["u"], g["v"]
    gxf, gyf = UT.grad_central_x_2nd, UT.grad_central_y_2nd
    r = {}
    u_c = 0.5 * (u + np.roll(u, -1, 1)); v_c = 0.5 * (v + np.roll(v, -1, 0))           # :106
    r["kin"] = ST([u_c, v_c, gxf(u_c, dx), gyf(u_c, dy), gxf(v_c, dx), gyf(v_c, dy)])  # :119-120
    be11, be12, be22, phi = g["be11"], g["be12"], g["be22"], g["phi"]
    H = F.smoothed_heaviside(phi, w_t)                                                 # :125-131
    Sxx = (1 - H) * G * be11; Sxy = (1 - H) * G * be12; Syy = (1 - H) * G * be22
    divx = gxf(Sxx, dx) + gyf(Sxy, dy)
    divy = gxf(Sxy, dx) + gyf(Syy, dy)
    f_su = 0.5 * (divx + np.roll(divx, 1, 1)); f_sv = 0.5 * (divy + np.roll(divy, 1, 0))
    Hu = 0.5 * (H + np.roll(H, 1, 1)); Hv = 0.5 * (H + np.roll(H, 1, 0))
    chi = 1.0 - H
    ny, nx = phi.shape
    le = M.lap_eigs_periodic(nx, ny, dx, dy)
    # mac.py:560-584 with the solve taken out: a unit symbol makes the FFT pair the identity
    # to rounding, so the right-hand side is captured by wrapping np.fft.fft2 instead
    seen = []
    orig = np.fft.fft2
    np.fft.fft2 = lambda a: (seen.append(a.copy()), orig(a))[1]
    try:
        pred = M.momentum_predictor_periodic_imex_elastic(u, v, E.NU, dx, dy, dt, le, E.CS2, chi,
                                                          g["fu"], g["fv"], rho)
    finally:
        np.fft.fft2 = orig
    r["rhs"] = ST(seen)
    fu, fv, us, vs, um, vm = g["fu"], g["fv"], g["us"], g["vs"], g["um"], g["vm"]
    lu = fu + Hu * beta * (um - u); lv = fv + Hv * beta * (vm - v)                      # :152-155
    r["lock_explicit"] = ST([us + dt * lu / rho, vs + dt * lv / rho])
    sm = phi <= 0                                                                      # :159-164
    r["record"] = np.array([float(X._lam_max(be11, be12, be22)[sm].max()), float(sm.sum()),
                            float(be11[ny // 2, nx // 2]), float(np.max(np.abs(u))),
                            float(np.all(np.isfinite(u)))])
    if arith_only:
        return r
    r["force"] = ST([f_su, f_sv, Hu, Hv, chi])
    r["pred"] = ST(pred)
    epu = np.exp(-dt * beta * Hu / rho); epv = np.exp(-dt * beta * Hv / rho)           # :139-150
    r["lock_imex-elastic"] = ST([um + (us - um) * epu, vm + (vs - vm) * epv])
    a = us + dt * fu / rho; b = vs + dt * fv / rho
    r["lock_imex"] = ST([um + (a - um) * epu, vm + (b - vm) * epv])
    return r


def gen_ops():
    out = {}
    for shape in E.SHAPES:
        g = E.op_inputs(shape)
        out[E.key(shape) + "_checksum"] = np.array([float(np.sum(g[k])) for k in sorted(g)])
        for name, val in ref_ops(g, shape == E.ARITH_ONLY).items():
            out[f"{E.key(shape)}_{name}"] = val
    save("mac_ve_extension_ops", **out)


class Tap:
    """Wraps the driver module's operators; one dict per step."""

    NAMES = ("rebuild_phi_from_reference_map", "extrapolate_reference_map", "logconf_local_step",
             "logconf_local_step_strang", "sym_exp", "project_per")

    def __init__(self):
        self.steps, self.orig = [], {k: getattr(X, k) for k in self.NAMES}

    def __enter__(self):
        for k in self.NAMES:
            setattr(X, k, getattr(self, "w_" + k))
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(X, k, f)

    def w_rebuild_phi_from_reference_map(self, *a):
        phi = self.orig["rebuild_phi_from_reference_map"](*a)
        self.steps.append(dict(phi=phi.copy(), n_extrap=0))
        return phi

    def w_extrapolate_reference_map(self, *a):
        out = self.orig["extrapolate_reference_map"](*a)
        if self.steps:      # (the initial extrapolation comes before the first step)
            s = self.steps[-1]
            s["n_extrap"] += 1
            if s["n_extrap"] == 1:
                s["X1"], s["X2"] = out[0].copy(), out[1].copy()
        return out

    def _local(self, name, a):
        out = self.orig[name](*a)
        self.steps[-1].update(psi=ST(out), dt=a[-1], tau=a[-2], stepper=name)
        return out

    def w_logconf_local_step(self, *a):
        return self._local("logconf_local_step", a)

    def w_logconf_local_step_strang(self, *a):
        return self._local("logconf_local_step_strang", a)

    def w_sym_exp(self, *a):
        out = self.orig["sym_exp"](*a)
        self.steps[-1]["be"] = ST(out)
        return out

    def w_project_per(self, *a):
        out = self.orig["project_per"](*a)
        self.steps[-1].update(u=out[0].copy(), v=out[1].copy())
        return out


def tapped_run(kw):
    """run(**kw) with the tap: (per-step record, dts, solid cells, min |phi|, final state)."""
    kw = dict(kw)
    tau = kw.pop("tau")
    with Tap() as tap, contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"), \
            tempfile.TemporaryDirectory() as tmp:
        t_ret, hist = X.run(tau=tau, save_frames=False, write=False, out_root=tmp, **kw)
    S, N = tap.steps, kw["N"]
    rec, t = [], 0.0
    for s in S:
        t += s["dt"]
        sm = s["phi"] <= 0
        lam = float(X._lam_max(*s["be"])[sm].max()) if sm.any() else np.nan
        rec.append((t, lam, float(s["be"][0][N // 2, N // 2]), float(np.max(np.abs(s["u"])))))
    assert t == t_ret
    if hist:
        assert hist[-1] == rec[-1], (hist[-1], rec[-1])         # run()'s own last record
    last = S[-1]
    return dict(record=np.array(rec), dts=np.array([s["dt"] for s in S]),
                cells=np.array([int((s["phi"] <= 0).sum()) for s in S]),
                min_abs_phi=np.array([float(np.abs(s["phi"]).min()) for s in S]),
                stepper=last["stepper"], **{k: last[k] for k in E.STATE})


def _short(case):
    return E.short_key(*case), tapped_run(E.short_kwargs(*case))


def _large(_):
    full = tapped_run(E.large_kwargs(E.SHORT_STEPS))      # the condition, step by step
    print(f"  large32 over {E.SHORT_STEPS} steps: cells={full['cells']}, "
          f"min|phi|={full['min_abs_phi']}")
    return E.LARGE["key"], tapped_run(E.large_kwargs())


def _long(name):
    kw = dict(E.LONG_CFG, **E.LONG[name]) if name in E.LONG else dict(E.SAT_CFG, **E.SAT[name])
    t_end = kw["t_end"]
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"), \
            tempfile.TemporaryDirectory() as tmp:
        steps = []
        orig = X.rebuild_phi_from_reference_map
        X.rebuild_phi_from_reference_map = lambda *a: (steps.append(0), orig(*a))[1]
        try:
            t, hist = X.run(save_frames=False, write=False, out_root=tmp, **kw)
        finally:
            X.rebuild_phi_from_reference_map = orig
    last = hist[-1] if hist else (np.nan,) * 4
    return name, np.array([float(E.reached(hist, t_end)), float(len(steps)), t, *last])


def _job(job):
    return {"short": _short, "large": _large, "long": _long}[job[0]](job[1])


def gen_runs():
    jobs = ([("long", n) for n in (*E.LONG, *E.SAT)] + [("large", None)]
            + [("short", c) for c in E.short_cases()])
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 4)) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    out = {}
    for (kind, _), (k, r) in zip(jobs, res):
        if kind == "long":
            out["long_" + k] = r
            print(f"  {k}: reached_end={bool(r[0])} steps={int(r[1])} t={r[2]!r} last={r[3:]!r}")
            continue
        nsteps = len(r["dts"])
        ok = [n for n in range(1, nsteps + 1)
              if np.all(r["cells"][:n] == r["cells"][0])]
        print(f"  {k}: {nsteps} steps, min|phi|={r['min_abs_phi'].min():.3e}, cells={r['cells']}, "
              f"stepper={r['stepper']}, constant-count prefix {max(ok)}")
        assert nsteps == (E.SHORT_STEPS if kind == "short" else E.LARGE["steps"])
        assert r["dts"][-1] < 0.75 * r["dts"][0]
        assert r["min_abs_phi"].min() >= E.MIN_ABS_PHI and max(ok) == nsteps, k
        for name, val in r.items():
            if name != "stepper":
                out[f"{k}_{name}"] = val
    save("mac_ve_extension_runs", **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["ops", "runs"]
    if "ops" in what:
        gen_ops()
    if "runs" in what:
        gen_runs()
