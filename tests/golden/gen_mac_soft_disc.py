"""Golden-vector generator for the soft disc in the lid cavity under the integrator ladder
(benchmarks/mac_soft_disc_lid.py, pyRMT/mac.py:43-78, 698-721): runs the pyRMT reference in
pure-Python mode (imported exactly as gen_golden.py does) and writes

    tests/golden/mac_soft_disc.npz        the seven N = 32 traces of tests/mac_soft_disc_np.py
                                          (TRACES): the record, the branch, CFL and PCG counts of
                                          every step, the state before and after the kept steps
    tests/golden/mac_soft_disc_ops.npz    the new operators on its off-square inputs (two files:
                                          each stays under the size limit of a committed file)

The driver's loop is not restated: its own run(N=32, write=False, ...) is called, and state is
captured by wrapping the names the driver module looks up per call (rebuild_phi_from_reference_map:
the maps a step starts from and every level set; the three predictors: u, v, the face forces;
solid_cauchy_stress: J; project: the new velocity; extrapolate_reference_map: the maps a step
ends with).  The PCG counts come through the reference's own `count` argument, and every CG goes
through a recording wrapper of scipy's cg (the solve itself untouched).

Asserted per trace (other parameters are to be picked if one fails, none is to be loosened):
both branches occur in each -sl trace and no step's CFL is within 1e-6 of cfl_switch; every
PCG solve returns the same count at rtol * 1.05 and rtol / 1.05 (||r|| / atol >= 1.05 on every
trip that runs, <= 1 / 1.05 where it stops); no cell's |phi| is below 1e-9 on any step; no trace
diverges and the row count is the step count; at every kept step the reference's own step (the
oracle's restatement, first checked against the captured step) answers a one-ulp change of one
velocity value with at most a tenth of the one-step bar, on u, v and on the maps
(tests/mac_soft_disc_np.py: map_noise and the note at TRACES).

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz file is data.

Usage:  python -B tests/golden/gen_mac_soft_disc.py
"""
import contextlib
import io
import os
import sys
import tempfile
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository: oracle/
from gen_golden import F, M, OUT, save  # noqa: E402
import numpy as np  # noqa: E402
import benchmarks.mac_soft_disc_lid as R  # noqa: E402
import mac_soft_disc_np as NP  # noqa: E402
from oracle import oracle as ORA, mac_oracle as MORA  # noqa: E402

SOLVES = []     # (iterations, ratios) of every cg the reference ran


def _cg_recorded(orig):
    def cg(Aop, b, x0=None, *, rtol=1e-5, atol=0.0, maxiter=None, M=None, callback=None):
        at = rtol * np.linalg.norm(b)
        ratios = [np.linalg.norm(b - Aop.matvec(x0)) / at]

        def cb(xk):
            ratios.append(np.linalg.norm(b - Aop.matvec(xk)) / at)
            if callback is not None:
                callback(xk)
        r = orig(Aop, b, x0=x0, rtol=rtol, atol=atol, maxiter=maxiter, M=M, callback=cb)
        SOLVES.append((len(ratios) - 1, ratios))
        return r
    return cg


def _pcg_counted(orig, counts):
    def pcg(*a, **kw):
        kw["count"] = counts
        return orig(*a, **kw)
    return pcg


class Tap:
    """Wraps the driver module's operators; one dict per step."""

    PRED = ("momentum_predictor", "momentum_predictor_lid_imex", "momentum_predictor_lid_semilag")
    NAMES = PRED + ("rebuild_phi_from_reference_map", "extrapolate_reference_map",
                    "solid_cauchy_stress", "project")

    def __init__(self, counts):
        self.steps, self.cur, self.counts = [], None, counts
        self.orig = {k: getattr(R, k) for k in self.NAMES}

    def __enter__(self):
        for k in self.NAMES:
            setattr(R, k, self.w_pred(k) if k in self.PRED else getattr(self, "w_" + k))
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(R, k, f)

    def w_rebuild_phi_from_reference_map(self, X1, X2, f):
        out = self.orig["rebuild_phi_from_reference_map"](X1, X2, f)
        if self.cur is None or "u_new" in self.cur:
            self.cur = dict(X1=X1.copy(), X2=X2.copy(), phis=[])
            self.steps.append(self.cur)
        self.cur["phis"].append(out.copy())
        return out

    def w_extrapolate_reference_map(self, *a):
        out = self.orig["extrapolate_reference_map"](*a)
        if self.cur is not None:
            self.cur["X1_new"], self.cur["X2_new"] = out[0].copy(), out[1].copy()
        return out

    def w_solid_cauchy_stress(self, *a, **kw):
        out = self.orig["solid_cauchy_stress"](*a, **kw)
        self.cur["J"] = out[3].copy()
        return out

    def w_pred(self, name):
        def pred(u, v, nu, dx, dy, dt, U_lid, **kw):
            cfl = dt * max(np.max(np.abs(u)) / dx, np.max(np.abs(v)) / dy)
            self.cur.update(u=u.copy(), v=v.copy(), dt=dt, fu=kw["fu"].copy(), fv=kw["fv"].copy(),
                            cfl=cfl, pred=name, cs2=kw.get("cs2", 0.0),
                            sl=name.endswith("semilag") and cfl > NP.CFL_SWITCH)
            n0 = len(self.counts)
            out = self.orig[name](u, v, nu, dx, dy, dt, U_lid, **kw)
            self.cur["its"] = list(self.counts[n0:]) or [0, 0]
            return out
        return pred

    def w_project(self, *a):
        out = self.orig["project"](*a)
        self.cur.update(u_new=out[0].copy(), v_new=out[1].copy())
        return out


def margins_ok(it, ratios):
    ran = ratios[:it]
    return (not ran or min(ran) >= 1.05) and ratios[it] <= 1.0 / 1.05


def gen_trace(name, out):
    kw, nsteps, keep = NP.TRACES[name]
    counts, n0 = [], len(SOLVES)
    pcg = M._pcg_helmholtz
    M._pcg_helmholtz = _pcg_counted(pcg, counts)
    try:
        with Tap(counts) as tap, contextlib.redirect_stdout(io.StringIO()) as buf:
            traj = R.run(N=NP.N, t_end=NP.t_end_of(name), write=False,
                         out_root=tempfile.mkdtemp(prefix="rmt_soft_"), **kw)
    finally:
        M._pcg_helmholtz = pcg
    S = tap.steps
    assert "DIVERGED" not in buf.getvalue(), name
    assert traj.shape == (nsteps, 5) and len(S) == nsteps, (name, traj.shape, len(S))
    assert all("u_new" in s for s in S)
    use_sl, use_imex, use_el = NP.resolve(kw["integrator"])
    for s in S:
        assert len(s["phis"]) == (1 if use_el else 2)
        assert min(np.abs(p).min() for p in s["phis"]) >= 1e-9, name
        assert len(s["its"]) == 2 and (use_imex or s["its"] == [0, 0])
        assert (s["cs2"] > 0.0) == use_el
    solves = SOLVES[n0:]
    assert len(solves) == (2 * nsteps if use_imex else 0), (name, len(solves))
    for it, ratios in solves:
        assert margins_ok(it, ratios), (name, it, ratios[-2:])
    sl = np.array([s["sl"] for s in S])
    cfl = np.array([s["cfl"] for s in S])
    its = np.array([s["its"] for s in S])
    assert [a for s in S for a in s["its"]] == (counts if use_imex else [0, 0] * nsteps)
    if use_sl:
        assert sl.any() and not sl.all(), name
        assert np.abs(cfl - NP.CFL_SWITCH).min() >= 1e-6
    else:
        assert not sl.any()
    np.testing.assert_array_equal(traj[:, 0], np.cumsum(np.full(nsteps, kw["dt"])))
    print(f"  {name}: {nsteps} steps, SL branch on {int(sl.sum())}, CFL {cfl.min():.3f}..{cfl.max():.3f} "
          f"(closest to the switch {np.abs(cfl - NP.CFL_SWITCH).min():.3f}), PCG counts "
          f"{its.min()}..{its.max()}, min |phi| {min(np.abs(p).min() for s in S for p in s['phis']):.2e}")
    out.update({f"{name}_record": traj, f"{name}_sl": sl, f"{name}_cfl": cfl, f"{name}_its": its,
                f"{name}_keep": np.array(keep), f"{name}_dt": kw["dt"],
                f"{name}_t_end": NP.t_end_of(name)})
    for k in keep:
        s = S[k - 1]
        for f in ("u", "v", "X1", "X2"):
            out[f"{name}_before{k}_{f}"] = s[f]
        out.update({f"{name}_after{k}_u": s["u_new"], f"{name}_after{k}_v": s["v_new"],
                    f"{name}_after{k}_X1": s["X1_new"], f"{name}_after{k}_X2": s["X2_new"],
                    f"{name}_after{k}_J": s["J"]})
        if name == "explicit":
            out[f"{name}_after{k}_phi"] = s["phis"][-1]
        st = {f: s[f] for f in ("u", "v", "X1", "X2")}
        base, wv, wm = NP.map_noise(ORA, MORA, st, kw["integrator"], kw["dt"], kw.get("mu_s", 0.1),
                                    kw.get("scheme", "semilagrangian"), seed=k)
        for f in ("u", "v", "X1", "X2"):      # the restatement is the captured step
            assert np.abs(base[f] - out[f"{name}_after{k}_{f}"]).max() <= 0.1 * NP.STEP_BAR, (name, k, f)
        print(f"    step {k}: one-ulp response of u, v {wv:.1e}, of the maps {wm:.1e}")
        assert max(wv, wm) <= 0.1 * NP.STEP_BAR, (name, k, wv, wm)
        out[f"{name}_noise{k}"] = np.array([wv, wm])
    last = S[-1]
    out.update({f"{name}_final_u": last["u_new"], f"{name}_final_v": last["v_new"],
                f"{name}_final_X1": last["X1_new"], f"{name}_final_X2": last["X2_new"]})
    # the force stage of the last kept step of the explicit trace, for the fused kernel
    if name == "explicit":
        s = S[keep[-1] - 1]
        fu, fv, J, S = NP.solid_force(F, s["X1_new"], s["X2_new"], s["phis"][-1], NP.DX, NP.DX,
                                      2.0 * NP.DX, 0.1)
        np.testing.assert_array_equal(fu, s["fu"])      # the restated stage is run()'s
        np.testing.assert_array_equal(fv, s["fv"])
        np.testing.assert_array_equal(J, s["J"])
        out.update(explicit_fu=fu, explicit_fv=fv,
                   explicit_fbar=NP.force_bar(S, s["phis"][-1], 2.0 * NP.DX, NP.DX, NP.DX)[1])


def gen_ops(out):
    for shape in NP.SHAPES:
        g, k = NP.op_inputs(shape), NP.key(shape)
        assert g["dx"] != g["dy"] and (g["phi"] <= 0)[1:-1, 1:-1].any()
        big = shape[0] * shape[1] >= 3000
        um = 0.5 * (g["u0"] + g["u1"]); vm = 0.5 * (g["v0"] + g["v1"])     # :133-134
        out[f"{k}_umc"] = 0.5 * (um[:, :-1] + um[:, 1:]); out[f"{k}_vmc"] = 0.5 * (vm[:-1, :] + vm[1:, :])
        cfl = g["dt"] * max(np.abs(g["u0"]).max() / g["dx"], np.abs(g["v0"]).max() / g["dy"])
        assert abs(cfl - 0.5) < 1e-12
        assert (g["phi"] <= g["w_cut"]).any() and (g["phi"] > g["w_cut"]).any()
        for w, tag in ((g["w_cut"], "adv"),) + (() if big else ((0.0, "adv0"),)):
            a = M.advect_xi_conservative(g["X1"], g["u0"], g["v0"], g["dx"], g["dy"], g["dt"],
                                         g["phi"], w)
            assert np.isfinite(a).all() and not np.array_equal(a, g["X1"])
            out[f"{k}_{tag}"] = a
        for iso, clamp in NP.stored_variants(shape):
            fu, fv, J, S = NP.solid_force(F, g["X1"], g["X2"], g["phi"], g["dx"], g["dy"], g["w_t"],
                                          NP.MU_S, NP.KAPPA, clamp, iso)
            sbar, _ = NP.force_bar(S, g["phi"], g["w_t"], g["dx"], g["dy"])
            # the bar on S (device sin against glibc's: |dH| <= 4e-16) must be reachable
            assert sbar == 0.0 or 4e-16 * (sbar / 1e-14) <= 0.5 * sbar
            v = NP.vkey(iso, clamp)
            out.update({f"{k}_{v}_fu": fu, f"{k}_{v}_fv": fv, f"{k}_{v}_J": J,
                        f"{k}_{v}_bars": np.array(NP.force_bar(S, g["phi"], g["w_t"], g["dx"], g["dy"]))})
            if not big or (iso, clamp) == NP.FORCE_VARIANTS[0]:
                out[f"{k}_{v}_S"] = np.stack(S)
            if clamp:
                assert shape[0] < 9 or (J == 5.0).any()     # the detG clamp fires
        J = out[f"{k}_{NP.vkey(False, 0.0)}_J"]
        out[f"{k}_diag"] = NP.soft_diag(g["phi"], J, g["u0"], g["v0"], g["dx"], g["dy"])
        m = g["phi"] <= 0
        Xc, Yc = np.meshgrid((np.arange(shape[1]) + 0.5) * g["dx"], (np.arange(shape[0]) + 0.5) * g["dy"])
        out[f"{k}_centroid"] = np.array([Xc[m].mean(), Yc[m].mean()])


if __name__ == "__main__":
    t0 = time.time()
    M.cg = _cg_recorded(M.cg)
    out, ops = {}, {}
    for name in NP.TRACES:
        gen_trace(name, out)
    gen_ops(ops)
    save("mac_soft_disc", N=NP.N, dt_ref=NP.DT_REF, **out)
    save("mac_soft_disc_ops", **ops)
    for f in ("mac_soft_disc.npz", "mac_soft_disc_ops.npz"):
        size = os.path.getsize(os.path.join(OUT, f))
        assert size <= 900 * 1024, (f, size)
    print(f"done in {time.time() - t0:.0f}s")
