"""NumPy restatement of the four-roll-mill viscoelastic driver (pyrmt_amd.mac:
ve_centre_kinematics, ve_face_force, momentum_predictor_periodic_imex_elastic, ve_lock,
ve_record and the loop MacViscoelasticExtension), the inputs its tests share and the bars they
hold the device to.

Every operator is written with the same NumPy calls in the same order as
benchmarks/mac_viscoelastic_extension.py and pyRMT/mac.py:560-584 evaluate them, so the
arithmetic ones give the reference's bits; tests/golden/mac_ve_extension_ops.npz and
mac_ve_extension_runs.npz (written from the reference itself) pin that.  Extrapolation and
advection go through the oracle, as in tests/viscoelastic_np.py.  `Ext(m, solve)` takes the
namespace its exp / sin (and, through viscoelastic_np.Ops, log / cos / arctan2) come from and
the function every FFT solve goes through: tools/mac_ve_ext_floor.py passes perturbing ones,
which is how the floors the bars stand on were measured.
"""
import json
import os

import numpy as np

import viscoelastic_np as V

INF = np.inf
same_bits = V.same_bits


def fft_solve(rhs, denom, pin=False):
    """Every FFT solve of the tier: ifft2(fft2(rhs) / denom), the (0, 0) mode zeroed for the
    Poisson solve (mac.py:471-473, 517-518, 582-583)."""
    h = np.fft.fft2(rhs) / denom
    if pin:
        h[0, 0] = 0.0
    return np.real(np.fft.ifft2(h))


def gx(f, dx):
    """utils.py:5-14 (not wrapping; the one-sided three-point rule at the two ends)."""
    o = np.zeros_like(f)
    o[:, 1:-1] = (f[:, 2:] - f[:, 0:-2]) / (2 * dx)
    o[:, 0] = (-3*f[:, 0] + 4*f[:, 1] - f[:, 2]) / (2*dx)
    o[:, -1] = (3*f[:, -1] - 4*f[:, -2] + f[:, -3]) / (2*dx)
    return o


def gy(f, dy):
    o = np.zeros_like(f)
    o[1:-1, :] = (f[2:, :] - f[0:-2, :]) / (2 * dy)
    o[0, :] = (-3*f[0, :] + 4*f[1, :] - f[2, :]) / (2*dy)
    o[-1, :] = (3*f[-1, :] - 4*f[-2, :] + f[-3, :]) / (2*dy)
    return o


def poisson_eigs(Nx, Ny, dx, dy):
    e = lap_eigs(Nx, Ny, dx, dy).copy()
    e[0, 0] = 1.0
    return e


def lap_eigs(Nx, Ny, dx, dy):
    lx = -4.0 * np.sin(np.pi * np.arange(Nx) / Nx) ** 2 / dx**2
    ly = -4.0 * np.sin(np.pi * np.arange(Ny) / Ny) ** 2 / dy**2
    return lx[np.newaxis, :] + ly[:, np.newaxis]


def _v_at_u(v):
    return 0.25 * (v + np.roll(v, 1, 1) + np.roll(v, -1, 0) + np.roll(np.roll(v, -1, 0), 1, 1))


def _u_at_v(u):
    return 0.25 * (u + np.roll(u, -1, 1) + np.roll(u, 1, 0) + np.roll(np.roll(u, 1, 0), -1, 1))


def _lap(q, dx, dy):
    return ((np.roll(q, -1, 1) - 2 * q + np.roll(q, 1, 1)) / dx**2
            + (np.roll(q, -1, 0) - 2 * q + np.roll(q, 1, 0)) / dy**2)


def _adv(u, v, dx, dy):
    dudx = (np.roll(u, -1, 1) - np.roll(u, 1, 1)) / (2 * dx)
    dudy = (np.roll(u, -1, 0) - np.roll(u, 1, 0)) / (2 * dy)
    dvdx = (np.roll(v, -1, 1) - np.roll(v, 1, 1)) / (2 * dx)
    dvdy = (np.roll(v, -1, 0) - np.roll(v, 1, 0)) / (2 * dy)
    return u * dudx + _v_at_u(v) * dudy, _u_at_v(u) * dvdx + v * dvdy


class Ext:
    """The operators; m: the namespace of exp and sin, solve: fft_solve or a stand-in."""

    def __init__(self, m=np, solve=fft_solve):
        self.m, self.solve, self.ve = m, solve, V.Ops(m)

    # ---- :106, :119-120
    @staticmethod
    def centre_kinematics(u, v, dx, dy):
        u_c = 0.5 * (u + np.roll(u, -1, 1)); v_c = 0.5 * (v + np.roll(v, -1, 0))
        return u_c, v_c, gx(u_c, dx), gy(u_c, dy), gx(v_c, dx), gy(v_c, dy)

    def heaviside(self, x, w_t):
        inv_wt = 1.0 / w_t; inv_pi = 1.0 / np.pi
        H = 0.5 * (1.0 + x * inv_wt + inv_pi * self.m.sin(np.pi * x * inv_wt))
        H = np.where(x > w_t, 1.0, H)
        return np.where(x < -w_t, 0.0, H)

    # ---- :125-131
    def face_force(self, be11, be12, be22, phi, G, w_t, dx, dy):
        H = self.heaviside(phi, w_t)
        Sxx = (1 - H) * G * be11; Sxy = (1 - H) * G * be12; Syy = (1 - H) * G * be22
        divx = gx(Sxx, dx) + gy(Sxy, dy)
        divy = gx(Sxy, dx) + gy(Syy, dy)
        return (0.5 * (divx + np.roll(divx, 1, 1)), 0.5 * (divy + np.roll(divy, 1, 0)),
                0.5 * (H + np.roll(H, 1, 1)), 0.5 * (H + np.roll(H, 1, 0)), 1.0 - H)

    # ---- mac.py:560-584
    @staticmethod
    def imex_elastic_rhs(u, v, dx, dy, dt, cs2, chi_c, fu, fv, rho=1.0):
        adv_u, adv_v = _adv(u, v, dx, dy)
        c_el = dt * dt * cs2
        chi_u = 0.5 * (chi_c + np.roll(chi_c, 1, 1))
        chi_v = 0.5 * (chi_c + np.roll(chi_c, 1, 0))
        return (u - dt * adv_u + dt * fu / rho + c_el * (1.0 - chi_u) * _lap(u, dx, dy),
                v - dt * adv_v + dt * fv / rho + c_el * (1.0 - chi_v) * _lap(v, dx, dy))

    def predictor_imex_elastic(self, u, v, nu, dx, dy, dt, lap_eig, cs2, chi_c, fu, fv, rho=1.0):
        ru, rv = self.imex_elastic_rhs(u, v, dx, dy, dt, cs2, chi_c, fu, fv, rho)
        denom = 1.0 - (dt * nu + dt * dt * cs2) * lap_eig
        return self.solve(ru, denom), self.solve(rv, denom)

    def predictor_imex(self, u, v, nu, dx, dy, dt, lap_eig):                 # mac.py:521-540
        adv_u, adv_v = _adv(u, v, dx, dy)
        denom = 1.0 - (dt * nu) * lap_eig
        return self.solve(u - dt * adv_u, denom), self.solve(v - dt * adv_v, denom)

    @staticmethod
    def predictor_explicit(u, v, nu, dx, dy, dt):                            # mac.py:636-650
        adv_u, adv_v = _adv(u, v, dx, dy)
        ru = -adv_u + nu * _lap(u, dx, dy)
        rv = -adv_v + nu * _lap(v, dx, dy)
        return u + dt * ru, v + dt * rv

    def project(self, us, vs, dx, dy, dt, rho, eig):                         # mac.py:476-480
        div = (np.roll(us, -1, 1) - us) / dx + (np.roll(vs, -1, 0) - vs) / dy
        phi = self.solve((rho / dt) * div, eig, True)
        return (us - (dt / rho) * ((phi - np.roll(phi, 1, 1)) / dx),
                vs - (dt / rho) * ((phi - np.roll(phi, 1, 0)) / dy), phi)

    # ---- :139-155; one face plane at a time
    def lock(self, star, u, f_s, Hf, mill, dt, beta, rho, mode):
        if mode == "explicit":
            fu = f_s + Hf * beta * (mill - u)
            return star + dt * fu / rho
        if mode == "imex":
            star = star + dt * f_s / rho
        ep = self.m.exp(-dt * beta * Hf / rho)
        return mill + (star - mill) * ep

    # ---- :159-171
    @staticmethod
    def record(be11, be12, be22, phi, u, at):
        sm = phi <= 0
        with np.errstate(invalid="ignore", over="ignore"):
            lam = float(V.lam_max_plane(be11, be12, be22)[sm].max()) if sm.any() else -INF
            return np.array([lam, float(sm.sum()), float(be11.ravel()[at]),
                             float(np.max(np.abs(u))), float(np.all(np.isfinite(u)))])


NP = Ext()

# ------------------------------------------------------------------ shared inputs --
SHAPES = ((3, 3), (5, 7), (33, 70), (64, 64))
ARITH_ONLY = (33, 70)          # the fixture keeps only the bit-exact results of this shape
DX, DY = 0.03125, 0.046875
W_T, G, NU, DT, CS2, RHO, BETA = 2.0 * DX, 0.3, 0.05, 0.01, 0.3, 1.25, 150.0
key = V.key


def op_inputs(shape):
    """Unit-normal planes (seeded by the shape) and a tilted-plane phi: the solid phi <= 0
    touches the west and the south edge and the corner between them, and both clamps of H and
    its sine branch occur on every shape (at (3, 3): -1.53, 0.2 and 1.93 w_t)."""
    ny, nx = shape
    rng = np.random.default_rng(1000 * ny + nx)
    names = ("u", "v", "be11", "be12", "be22", "fu", "fv", "us", "vs", "um", "vm")
    g = {k: rng.standard_normal(shape) for k in names}
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    g["phi"] = W_T * (3.0 * (i + 0.5) / nx + 2.2 * (j + 0.5) / ny - 2.4)
    return g


def op_results(E, g, arith_only=False):
    """Every operator of `E` on the inputs g, by fixture name."""
    r = {}
    r["kin"] = np.stack(E.centre_kinematics(g["u"], g["v"], DX, DY))
    ff = E.face_force(g["be11"], g["be12"], g["be22"], g["phi"], G, W_T, DX, DY)
    chi = ff[4]
    r["rhs"] = np.stack(E.imex_elastic_rhs(g["u"], g["v"], DX, DY, DT, CS2, chi, g["fu"], g["fv"],
                                           RHO))
    r["lock_explicit"] = np.stack([
        E.lock(g["us"], g["u"], g["fu"], ff[2], g["um"], DT, BETA, RHO, "explicit"),
        E.lock(g["vs"], g["v"], g["fv"], ff[3], g["vm"], DT, BETA, RHO, "explicit")])
    r["record"] = E.record(g["be11"], g["be12"], g["be22"], g["phi"], g["u"],
                           (g["phi"].shape[0] // 2) * g["phi"].shape[1] + g["phi"].shape[1] // 2)
    if arith_only:
        return r
    r["force"] = np.stack(ff)
    ny, nx = g["phi"].shape
    le = lap_eigs(nx, ny, DX, DY)
    r["pred"] = np.stack(E.predictor_imex_elastic(g["u"], g["v"], NU, DX, DY, DT, le, CS2, chi,
                                                  g["fu"], g["fv"], RHO))
    for mode in ("imex", "imex-elastic"):
        r["lock_" + mode] = np.stack([
            E.lock(g["us"], g["u"], g["fu"], ff[2], g["um"], DT, BETA, RHO, mode),
            E.lock(g["vs"], g["v"], g["fv"], ff[3], g["vm"], DT, BETA, RHO, mode)])
    return r


# ------------------------------------------------------------------------ the loop --
def resolve(integrator=None, imex=False, elastic_imex=False):
    name = integrator or ("imex-elastic" if elastic_imex else "imex" if imex else "explicit")
    return name, name in ("imex", "imex-elastic"), name == "imex-elastic"


class Loop:
    """benchmarks/mac_viscoelastic_extension.run (:41-189) without frames and files: the same
    sequence as pyrmt_amd.mac.MacViscoelasticExtension, a plane at a time."""

    BETA, LAYERS = 150.0, 3

    def __init__(self, O, E, N=128, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.05, rho=1.0, R=0.13,
                 integrator=None, imex=False, elastic_imex=False, dt=None):
        self.O, self.E, self.N, self.R, self.G, self.rho = O, E, N, R, G, rho
        dx, dy = 1.0 / N, 1.0 / N
        self.dx, self.dy = dx, dy
        xc = (np.arange(N) + 0.5) * dx; xf = np.arange(N) * dx
        Xc, Yc = np.meshgrid(xc, xc)
        Xu, Yu = np.meshgrid(xf, xc); Xv, Yv = np.meshgrid(xc, xf)
        self.Xg, self.Yg = np.meshgrid(xf, xf)
        self.w_t = 2.0 * dx; self.nu = mu_f / rho
        k = 2.0 * np.pi; U0 = eps_rate / k
        self.u_mill = U0 * np.sin(k * Xu) * np.cos(k * Yu)
        self.v_mill = -U0 * np.cos(k * Xv) * np.sin(k * Yv)
        phi = np.sqrt((Xc - 0.5)**2 + (Yc - 0.5)**2) - R; m = (phi <= 0).astype(float)
        self.X1, self.X2 = O.extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, self.LAYERS)
        self.psi = [np.zeros((N, N)) for _ in range(3)]
        self.name, self.imex, self.elastic = resolve(integrator, imex, elastic_imex)
        self.u = np.zeros((N, N)); self.v = np.zeros((N, N))
        self.eig = poisson_eigs(N, N, dx, dy)
        self.lap_eig = lap_eigs(N, N, dx, dy) if self.imex else None
        cs = np.sqrt(G / rho)
        dt_adv = 0.25 * dx / max(U0, 0.1)
        dt_visc = 0.2 * dx * dx / self.nu
        dt_elastic = 0.3 * dx / (cs + 1e-9)
        if dt is None:
            dt = dt_adv if self.elastic else (min(dt_adv, dt_elastic) if self.imex
                                              else min(dt_adv, dt_visc, dt_elastic))
        self.dt = dt
        self.tau = INF if tau <= 0 else tau
        self.Wi = eps_rate * self.tau
        self.bxx_analytic = (INF if (self.tau == INF or self.Wi >= 0.5)
                             else 1.0 / (1.0 - 2.0 * self.Wi))
        self.t, self.nsteps, self.stopped, self.clause = 0.0, 0, False, None
        self.record, self.dts, self.cells, self.min_abs_phi = [], [], [], INF
        self.phi = self.be = None

    def step(self, nsteps=1, t_end=INF):
        O, E, N, dx, dy, rho = self.O, self.E, self.N, self.dx, self.dy, self.rho
        dt = self.dt
        for _ in range(nsteps):
            if self.stopped or not self.t < t_end:
                break
            if self.t + dt > t_end:
                dt = t_end - self.t
            u, v = self.u, self.v
            u_c, v_c, L11, L12, L21, L22 = E.centre_kinematics(u, v, dx, dy)
            phi = O.rebuild_phi_disc(self.X1, self.X2, 0.5, 0.5, self.R)
            m = (phi <= 0).astype(float)
            adv = lambda q: O.advect_reference_map(q, u_c, v_c, self.Xg, self.Yg, dt, dx, dy, phi,
                                                   'semilagrangian', 0.0) * m
            X1, X2 = adv(self.X1), adv(self.X2)
            self.X1, self.X2 = O.extrapolate_reference_map(X1, X2, phi, dx, dy, self.LAYERS)
            p11, p12, p22 = (adv(p) for p in self.psi)
            p11, p12 = O.extrapolate_reference_map(p11, p12, phi, dx, dy, self.LAYERS)
            p22, _ = O.extrapolate_reference_map(p22, np.zeros((N, N)), phi, dx, dy, self.LAYERS)
            self.psi = list(E.ve.stepper(self.imex)(p11, p12, p22, L11, L12, L21, L22, self.tau,
                                                   dt))
            be = E.ve.sym_exp(*self.psi)
            f_su, f_sv, Hu, Hv, chi = E.face_force(*be, phi, self.G, self.w_t, dx, dy)
            if self.elastic:
                us, vs = E.predictor_imex_elastic(u, v, self.nu, dx, dy, dt, self.lap_eig,
                                                  self.G / rho, chi, f_su, f_sv, rho)
            elif self.imex:
                us, vs = E.predictor_imex(u, v, self.nu, dx, dy, dt, self.lap_eig)
            else:
                us, vs = E.predictor_explicit(u, v, self.nu, dx, dy, dt)
            us = E.lock(us, u, f_su, Hu, self.u_mill, dt, self.BETA, rho, self.name)
            vs = E.lock(vs, v, f_sv, Hv, self.v_mill, dt, self.BETA, rho, self.name)
            self.u, self.v, self.p = E.project(us, vs, dx, dy, dt, rho, self.eig)
            self.t += dt
            self.nsteps += 1
            ci = N // 2
            lam, count, bxx_c, umax, finite = E.record(*be, phi, self.u, ci * N + ci)
            if count == 0:
                lam = np.nan
            self.phi, self.be = phi, be
            self.min_abs_phi = min(self.min_abs_phi, float(np.abs(phi).min()))
            self.record.append((self.t, lam, bxx_c, umax))
            self.dts.append(dt); self.cells.append(int(count))
            if not finite or count == 0 or lam > 1e4:                           # :170
                self.stopped = True
                self.clause = "non-finite u" if not finite else "no solid cell" if count == 0 \
                    else "lam_max > 1e4"
        return self

    def history(self, t_end=INF):
        return [r for k, r in enumerate(self.record, 1) if k % 100 == 0 or r[0] >= t_end]

    def state(self):
        return dict(u=self.u, v=self.v, X1=self.X1, X2=self.X2, phi=self.phi,
                    psi=np.stack(self.psi), be=np.stack(self.be))


def run(O, E, N, t_end, **kw):
    """(t, hist, the Loop) of run(N, t_end, ...)."""
    with np.errstate(over="ignore", invalid="ignore"):
        sim = Loop(O, E, N=N, **kw).step(2**31 - 1, t_end)
    return sim.t, sim.history(t_end), sim


# ---- the short runs: 12 steps, the last clipped, at the explicit viscous step of mu_f = 0.05
INTEGRATORS = ("explicit", "imex", "imex-elastic")
SHORT_N, SHORT_TAUS, SHORT_STEPS, MU_F = (24, 32), (0.5, 0.0), 12, 0.05
STATE = ("u", "v", "X1", "X2", "phi", "psi", "be")


def short_dt(N):
    dx = 1.0 / N
    return 0.2 * dx * dx / MU_F


def short_cases():
    return [(N, name, tau) for N in SHORT_N for name in INTEGRATORS for tau in SHORT_TAUS]


def short_key(N, name, tau):
    return f"n{N}_{name}_tau{tau:g}"


def short_kwargs(N, name, tau):
    return dict(N=N, t_end=(SHORT_STEPS - 0.5) * short_dt(N), tau=tau, dt=short_dt(N), mu_f=MU_F,
                integrator=name)


MIN_ABS_PHI = 1e-4     # no cell changes side under rounding: min |phi| over a run's steps
# the driver's own dt (dt_adv, 20 x short_dt): over 12 steps the solid-cell count changes at
# step 5 (52 -> 56) and min |phi| falls to 8.7e-5 there, so the fixture keeps the longest
# prefix on which the condition holds, 4 steps (the 4th clipped)
LARGE = dict(N=32, name="imex-elastic", tau=0.5, key="large32", steps=4)


def large_dt():
    return 0.25 * (1.0 / LARGE["N"]) / max(0.5 / (2.0 * np.pi), 0.1)


def large_kwargs(steps=LARGE["steps"]):
    return dict(N=LARGE["N"], t_end=(steps - 0.5) * large_dt(), tau=LARGE["tau"], mu_f=MU_F,
                integrator=LARGE["name"])


# ---- the eight N = 40 runs of the reference's test_ve_imex_fsi.py and test_elastic_imex.py
_DTV = 0.2 * (1.0 / 40) * (1.0 / 40) / 0.05
_DTE = 0.3 * (1.0 / 40) / np.sqrt(0.3)
LONG = {
    "fsi_explicit": dict(imex=False, dt=_DTV, t_end=1.0),
    "fsi_imex": dict(imex=True, dt=_DTV, t_end=1.0),
    "fsi_explicit_3x": dict(imex=False, dt=3.0 * _DTV, t_end=1.0),
    "fsi_imex_3x": dict(imex=True, dt=3.0 * _DTV, t_end=1.0),
    "el_explicit": dict(imex=False, t_end=0.6),
    "el_elastic_small": dict(elastic_imex=True, dt=0.2 * _DTE, t_end=0.6),
    "el_imex_8x": dict(imex=True, dt=8.0 * _DTE, t_end=0.8),
    "el_elastic_8x": dict(elastic_imex=True, dt=8.0 * _DTE, t_end=0.8),
}
LONG_CFG = dict(N=40, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.05)
# the two runs that blow up, and the clause of :170 that ends each in the restatement on the
# CPU (at the reference's step: 12 and 6)
DIVERGING = {"fsi_explicit_3x": "non-finite u", "el_imex_8x": "lam_max > 1e4"}


# ---- saturation at N = 32, tau = 0.5 (Wi = 0.25, b_xx -> 2).  With the driver's defaults (the
# explicit integrator at its own dt) the reference's run stops at step 129, t = 0.504, on
# `u not all finite`, long before it saturates, so the check runs under "imex" at its own dt
# to t_end = 4; both records are in the fixture.
SAT_CFG = dict(N=32, tau=0.5)
SAT = {"sat_explicit": dict(t_end=4.0), "sat_imex": dict(t_end=4.0, integrator="imex")}


def reached(hist, t_end):
    return bool(hist) and hist[-1][0] >= t_end - 1e-9


# ----------------------------------------------------------------------------- bars --
BAR_FACTOR = V.BAR_FACTOR
FLOOR_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                          "profiles", "ve_extension", "floor.json")
FFT_REL = 1e-12       # the project's bar for the rocFFT / pocketfft pair, of max-abs


def floors():
    with open(FLOOR_JSON) as f:
        return json.load(f)["floors"]


FLOORS = floors() if os.path.exists(FLOOR_JSON) else {}


def bar(case):
    return BAR_FACTOR * FLOORS[case]


def assert_close(got, ref, case, what=""):
    """Finite values within bar(case), the non-finite pattern equal; printed, then asserted."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what or case, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(ref), err_msg=f"{what} finite")
    ok = np.isfinite(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print(f"{what or case}: max err {err:.3e}, bar {bar(case):.3e}")
    assert err <= bar(case), (what or case, err, bar(case))
