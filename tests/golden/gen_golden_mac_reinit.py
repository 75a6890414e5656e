"""Golden-vector generator for reference-map reinitialisation with stored deformation
(benchmarks/mac_reinit_test.py, Rycroft 2018): runs the pyRMT reference in pure-Python mode
(imported exactly as gen_golden.py does) and writes

    tests/golden/mac_reinit_trace32.npz   run(N=32, t_end=60.5 dt, reinit_J=1.02): 61 steps (the
                                          last one clipped to dt / 2), the per-step record and the
                                          full state before and after steps 26, 40, 53 and 60
    tests/golden/mac_reinit_ops.npz       the stage outputs of step 40 of that run, and the
                                          operators on tests/mac_reinit_np.py's off-square inputs

The driver's loop is not restated: its own run() is called, and state is captured by wrapping
the names the driver module looks up per call (advect_reference_map: the six planes a step
starts from; bilinear_interpolate: phiref and both level sets; momentum_predictor: u, v, the
face forces and the step's dt; _F_current, _matmul: J_ep and Ftot; project: the new velocity;
extrapolate_reference_map: five calls in a step that reinitialises, three otherwise).  So the
capture is run()'s own arithmetic by construction; the numbers run() prints on its last step
are parsed and checked against the captured ones all the same.

The generator asserts that the run reinitialises at steps [26, 53] exactly and that no step's
distortion comes closer than 1e-6 to reinit_J (device rounding, ~1e-14, cannot flip a decision).

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_golden_mac_reinit.py
"""
import contextlib
import io
import os
import re
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import F, M, save  # noqa: E402
import numpy as np  # noqa: E402
import benchmarks.mac_reinit_test as R  # noqa: E402
import mac_reinit_np as NP  # noqa: E402

N, REINIT_J, NSTEPS, KEEP, STAGE = 32, 1.02, 61, (26, 40, 53, 60), 40
MU_S, MU_F, RHO, U_LID = 0.3, 0.01, 1.0, 1.0


class Tap:
    """Wraps the driver module's operators; one dict per step."""

    NAMES = ("advect_reference_map", "extrapolate_reference_map", "bilinear_interpolate",
             "momentum_predictor", "project", "_F_current", "_matmul")

    def __init__(self):
        self.steps, self.cur, self.orig = [], None, {k: getattr(R, k) for k in self.NAMES}
        self.started = False   # (the initial extrapolation comes before the first step)

    def __enter__(self):
        for k in self.NAMES:
            setattr(R, k, getattr(self, "w_" + k.lstrip("_")))
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(R, k, f)

    def w_bilinear_interpolate(self, phiref, *a):
        out = self.orig["bilinear_interpolate"](phiref, *a)
        if self.cur is None or "u_new" in self.cur:
            self.cur = dict(phiref=phiref.copy(), phi_pre=out.copy(), q=[], n_extrap=0, matmul=[])
            self.steps.append(self.cur)
            self.started = True
        else:
            self.cur["phi"] = out.copy()
        return out

    def w_advect_reference_map(self, q, *a):
        self.cur["q"].append(q.copy())
        return self.orig["advect_reference_map"](q, *a)

    def w_extrapolate_reference_map(self, *a):
        out = self.orig["extrapolate_reference_map"](*a)
        if self.started:
            self.cur["n_extrap"] += 1
            if self.cur["n_extrap"] == 1:
                self.cur["X1e"], self.cur["X2e"] = out[0].copy(), out[1].copy()
            elif self.cur["n_extrap"] in (2, 3):
                self.cur.setdefault("Fse", []).extend([out[0].copy(), out[1].copy()])
        return out

    def w_F_current(self, *a):
        out = self.orig["_F_current"](*a)
        self.cur["Fc"] = [p.copy() for p in out]
        return out

    def w_matmul(self, A, B):
        out = self.orig["_matmul"](A, B)
        self.cur["matmul"].append([p.copy() for p in out])
        return out

    def w_momentum_predictor(self, u, v, nu, dx, dy, dt, U_lid, fu=None, fv=None, rho=1.0):
        self.cur.update(u=u.copy(), v=v.copy(), dt=dt, fu=fu.copy(), fv=fv.copy())
        return self.orig["momentum_predictor"](u, v, nu, dx, dy, dt, U_lid, fu=fu, fv=fv, rho=rho)

    def w_project(self, *a):
        out = self.orig["project"](*a)
        self.cur.update(u_new=out[0].copy(), v_new=out[1].copy())
        return out


def distortion(J_ep, phi):
    sm = phi <= 0
    if not sm.any():
        return np.inf, np.nan, np.nan, 0
    jin = J_ep[sm]
    return max(jin.max(), 1.0 / max(jin.min(), 1e-6)), jin.min(), jin.max(), int(sm.sum())


def state_before(s):
    return dict(X1=s["q"][0], X2=s["q"][1], Fs=np.stack(s["q"][2:6]), phiref=s["phiref"],
                u=s["u"], v=s["v"])


def gen_trace():
    dx, _ = M.mac_grid(N, N)
    dt = min(0.3 * dx / U_LID, 0.2 * dx * dx / (MU_F / RHO), 0.3 * dx / (np.sqrt(MU_S / RHO) + 1e-9))
    t_end = (NSTEPS - 0.5) * dt
    buf = io.StringIO()
    with Tap() as tap, contextlib.redirect_stdout(buf):
        t_ret = R.run(N=N, t_end=t_end, reinit=True, U_lid=U_LID, mu_s=MU_S, mu_f=MU_F, rho=RHO,
                      reinit_J=REINIT_J)
    S = tap.steps
    assert len(S) == NSTEPS and all("u_new" in s for s in S), len(S)
    rec, t, n_reinit, reinit_steps = [], 0.0, 0, []
    for k, s in enumerate(S, 1):
        t += s["dt"]
        dist, jmin, jmax, cnt = distortion(s["Fc"][4], s["phi"])
        assert s["n_extrap"] in (3, 5)
        if s["n_extrap"] == 5:
            n_reinit += 1
            reinit_steps.append(k)
            assert dist > REINIT_J
        else:
            assert not dist > REINIT_J
        rec.append((t, dist, jmin, jmax, n_reinit, np.abs(s["u_new"]).max(), cnt))
    rec = np.array(rec)
    margin = np.abs(rec[:, 1] - REINIT_J).min()
    print(f"  reinitialisations at steps {reinit_steps}, smallest |dist - reinit_J| = {margin:.3e} "
          f"at step {1 + int(np.abs(rec[:, 1] - REINIT_J).argmin())}")
    assert reinit_steps == [26, 53], reinit_steps
    assert margin >= 1e-6, margin
    assert S[-1]["dt"] < 0.75 * dt and t_ret == t == rec[-1, 0]
    # run()'s own last-step line against the capture
    last = [ln for ln in buf.getvalue().splitlines() if ln.strip().startswith("step")][-1]
    mm = re.search(r"step\s+(\d+) t=\s*([\d.]+) epochJ\[([-\d.]+),([-\d.]+)\].*reinits=(\d+) "
                   r"max\|u\|=([\d.]+)", last)
    assert mm, last
    assert int(mm.group(1)) == NSTEPS and int(mm.group(5)) == n_reinit == 2
    assert mm.group(2) == f"{t:.3f}" and mm.group(3) == f"{rec[-1, 2]:.2f}"
    assert mm.group(4) == f"{rec[-1, 3]:.2f}" and mm.group(6) == f"{rec[-1, 5]:.2f}"
    out = dict(N=N, reinit_J=REINIT_J, mu_s=MU_S, mu_f=MU_F, rho=RHO, U_lid=U_LID, dt=dt,
               t_end=t_end, record=rec, reinit_steps=np.array(reinit_steps), margin=margin,
               keep=np.array(KEEP))
    for k in KEEP:
        for name, a in state_before(S[k - 1]).items():
            out[f"before{k}_{name}"] = a
        for name, a in state_before(S[k]).items():
            out[f"after{k}_{name}"] = a
        out[f"after{k}_phi"] = S[k - 1]["phi"]
        if S[k - 1]["n_extrap"] == 5:   # Ftot of the step, before the fold's extrapolation
            out[f"ftot{k}"] = np.stack(S[k - 1]["matmul"][1])
    save("mac_reinit_trace32", **out)
    return S, dx, dt


def stage_outputs(X1, X2, Fs, phi, dx, dy, w_t, mu_s):
    """The :74-85 stage on given planes, through the driver's own _F_current / _matmul and the
    reference's operators ((ny, nx) need not be square)."""
    ny, nx = phi.shape
    Fc = R._F_current(X1, X2, dx, dy)
    Ft = R._matmul(Fc[:4], Fs)
    b11 = Ft[0]**2 + Ft[1]**2
    b12 = Ft[0]*Ft[2] + Ft[1]*Ft[3]
    b22 = Ft[2]**2 + Ft[3]**2
    H = F.smoothed_heaviside(phi, w_t)
    Sxx = (1 - H) * mu_s * b11; Sxy = (1 - H) * mu_s * b12; Syy = (1 - H) * mu_s * b22
    divx = R.grad_central_x_2nd(Sxx, dx) + R.grad_central_y_2nd(Sxy, dy)
    divy = R.grad_central_x_2nd(Sxy, dx) + R.grad_central_y_2nd(Syy, dy)
    fu = np.zeros((ny, nx + 1)); fu[:, 1:-1] = 0.5 * (divx[:, 1:] + divx[:, :-1])
    fv = np.zeros((ny + 1, nx)); fv[1:-1, :] = 0.5 * (divy[1:, :] + divy[:-1, :])
    # the bar on S (1e-14, device sin against glibc's: |dH| <= 4e-16) must be reachable
    band = np.abs(phi) <= w_t
    amp = max(np.abs(mu_s * b[band]).max() for b in (b11, b12, b22))
    assert 4e-16 * amp <= 5e-15, amp
    return dict(J=Fc[4], Ftot=np.stack(Ft), S=np.stack([Sxx, Sxy, Syy]), fu=fu, fv=fv)


def gen_ops(S, dx, dt):
    out = {}
    s = S[STAGE - 1]
    st = stage_outputs(s["X1e"], s["X2e"], s["Fse"], s["phi"], dx, dx, 2.0 * dx, MU_S)
    np.testing.assert_array_equal(st["fu"], s["fu"])     # the restated stage is run()'s
    np.testing.assert_array_equal(st["fv"], s["fv"])
    np.testing.assert_array_equal(st["J"], s["Fc"][4])
    assert not np.array_equal(s["Fse"][0], np.ones((N, N)))   # second epoch: Fs != I
    out.update(s40_X1=s["X1e"], s40_X2=s["X2e"], s40_Fs=np.stack(s["Fse"]), s40_phi=s["phi"],
               s40_dx=dx, **{f"s40_{k}": v for k, v in st.items()})
    d = distortion(s["Fc"][4], s["phi"])
    out["s40_dist"] = np.array([d[2], d[1], d[3]], dtype=np.float64)   # max J, min J, count
    for shape in NP.SHAPES:
        g = NP.op_inputs(shape)
        k = NP.key(shape)
        st = stage_outputs(g["X1"], g["X2"], g["Fs"], g["phi"], g["dx"], g["dy"], g["w_t"], NP.MU_S)
        assert (st["J"] == 1.0 / 1e-9).any()     # the detG clamp fires
        out.update({f"{k}_{n}": v for n, v in st.items()})
        d = distortion(st["J"], g["phi"])
        out[f"{k}_dist"] = np.array([d[2], d[1], d[3]], dtype=np.float64)
        m = (g["phi"] <= 0).astype(float)
        adv = [F.advect_reference_map(q, g["a"], g["b"], g["Xg"], g["Yg"], NP.ADV_DT, g["dx"],
                                      g["dy"], g["phi"], 'semilagrangian', 0.0) for q in g["q"]]
        # masked: all eight planes (zero outside the disc, so they pack well); unmasked: all
        # eight on the two small shapes, planes 0 and 3 (the NaN one) on the two large ones
        out[f"{k}_advm"] = np.stack([p * m for p in adv])
        keep = range(8) if shape[0] * shape[1] < 3000 else (0, 3)
        out[f"{k}_adv_planes"] = np.array(list(keep))
        out[f"{k}_adv"] = np.stack([adv[i] for i in keep])
        assert np.signbit(out[f"{k}_advm"]).any() and np.isnan(out[f"{k}_advm"]).any()
    save("mac_reinit_ops", **out)


if __name__ == "__main__":
    S, dx, dt = gen_trace()
    gen_ops(S, dx, dt)
