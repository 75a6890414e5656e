"""NumPy restatement of the viscoelastic constitutive layer (pyrmt_amd/viscoelastic.py), the
inputs its tests share, and the bars they hold the device to.

The restatement is written from the formulas (upper-convected Maxwell; log-conformation after
Fattal & Kupferman 2004 in closed form for 2 x 2) with the same NumPy calls in the same order as
the reference evaluates them, so the arithmetic operators give its bits; tests/golden/
viscoelastic_ops.npz (written from the reference itself) pins that.  `Ops(m)` takes the
namespace its exp, log, sin, cos and arctan2 come from: tools/ve_floor.py passes one that moves
every result by up to an ulp, which is how the noise floors below were measured.

Inputs are built from +, * and sqrt on index grids (correctly rounded everywhere), so the
fixture generator, the CPU tests and the GPU tests hold the same bits without storing them.
"""
import json
import os

import numpy as np

INF = np.inf


class Ops:
    def __init__(self, m=np):
        self.m = m

    # ---- UCM
    @staticmethod
    def ucm_local_rhs(b11, b12, b22, L11, L12, L21, L22, tau):
        D11 = 2.0 * (L11 * b11 + L12 * b12)
        D12 = (L11 * b12 + L12 * b22) + (L21 * b11 + L22 * b12)
        D22 = 2.0 * (L21 * b12 + L22 * b22)
        it = 0.0 if tau == INF else 1.0 / tau
        return D11 - it * (b11 - 1.0), D12 - it * b12, D22 - it * (b22 - 1.0)

    def ucm_local_step(self, b11, b12, b22, L11, L12, L21, L22, tau, dt, nsteps=1):
        for _ in range(nsteps):
            k1 = self.ucm_local_rhs(b11, b12, b22, L11, L12, L21, L22, tau)
            k2 = self.ucm_local_rhs(b11 + dt * k1[0], b12 + dt * k1[1], b22 + dt * k1[2],
                                    L11, L12, L21, L22, tau)
            b11 = b11 + 0.5 * dt * (k1[0] + k2[0])
            b12 = b12 + 0.5 * dt * (k1[1] + k2[1])
            b22 = b22 + 0.5 * dt * (k1[2] + k2[2])
        return b11, b12, b22

    @staticmethod
    def viscoelastic_stress(b11, b12, b22, G, b_ref=None, G_inf=0.0):
        s = [G * b11, G * b12, G * b22]
        if b_ref is not None and G_inf != 0.0:
            s = [s[k] + G_inf * b_ref[k] for k in range(3)]
        return tuple(s)

    # ---- log-conformation
    def eig2(self, a, b, c):
        """(l1 >= l2, angle of l1's eigenvector) of [[a, b], [b, c]]."""
        tr = 0.5 * (a + c)
        d = np.sqrt(np.maximum(0.25 * (a - c)**2 + b * b, 0.0))
        return tr + d, tr - d, 0.5 * self.m.arctan2(2.0 * b, a - c)

    def _spectral(self, a, b, c, fn):
        l1, l2, th = self.eig2(a, b, c)
        f1 = fn(l1); f2 = fn(l2)
        cs, sn = self.m.cos(th), self.m.sin(th)
        return cs*cs*f1 + sn*sn*f2, cs*sn*(f1 - f2), sn*sn*f1 + cs*cs*f2

    def sym_log(self, a, b, c):
        return self._spectral(a, b, c, lambda l: self.m.log(np.maximum(l, 1e-300)))

    def sym_exp(self, a, b, c):
        return self._spectral(a, b, c, self.m.exp)

    def logconf_local_rhs(self, p11, p12, p22, L11, L12, L21, L22, tau):
        m = self.m
        l1, l2, th = self.eig2(p11, p12, p22)
        cs, sn = m.cos(th), m.sin(th)
        a11 = cs*L11 + sn*L21; a12 = cs*L12 + sn*L22           # R^T L
        a21 = -sn*L11 + cs*L21; a22 = -sn*L12 + cs*L22
        M11 = a11*cs + a12*sn; M12 = -a11*sn + a12*cs          # R^T L R
        M21 = a21*cs + a22*sn; M22 = -a21*sn + a22*cs
        lam1 = m.exp(l1); lam2 = m.exp(l2)
        denom = lam2 - lam1
        deg = np.abs(denom) < 1e-10
        ratio = np.where(deg, m.exp(-l1), (l2 - l1) / np.where(deg, 1.0, denom))
        it = 0.0 if tau == INF else 1.0/tau
        E11 = 2.0*M11 + it*(m.exp(-l1) - 1.0)
        E22 = 2.0*M22 + it*(m.exp(-l2) - 1.0)
        E12 = ratio * (lam2*M12 + lam1*M21)
        return (cs*cs*E11 - 2.0*cs*sn*E12 + sn*sn*E22,
                cs*sn*(E11 - E22) + (cs*cs - sn*sn)*E12,
                sn*sn*E11 + 2.0*cs*sn*E12 + cs*cs*E22)

    def lam_gap(self, p11, p12, p22):
        """|lam2 - lam1| as logconf_local_rhs forms it (the `deg` test's operand)."""
        l1, l2, _ = self.eig2(p11, p12, p22)
        return np.abs(self.m.exp(l2) - self.m.exp(l1))

    def logconf_local_step(self, p11, p12, p22, L11, L12, L21, L22, tau, dt, nsteps=1):
        for _ in range(nsteps):
            k1 = self.logconf_local_rhs(p11, p12, p22, L11, L12, L21, L22, tau)
            k2 = self.logconf_local_rhs(p11 + dt*k1[0], p12 + dt*k1[1], p22 + dt*k1[2],
                                        L11, L12, L21, L22, tau)
            p11, p12, p22 = (p11 + 0.5*dt*(k1[0]+k2[0]), p12 + 0.5*dt*(k1[1]+k2[1]),
                             p22 + 0.5*dt*(k1[2]+k2[2]))
        return p11, p12, p22

    def relax_exact(self, p11, p12, p22, tau, dt):
        if tau == INF or dt == 0.0:
            return p11, p12, p22
        b11, b12, b22 = self.sym_exp(p11, p12, p22)
        e = self.m.exp(-dt / tau)
        return self.sym_log(1.0 + (b11 - 1.0) * e, b12 * e, 1.0 + (b22 - 1.0) * e)

    def logconf_local_step_strang(self, p11, p12, p22, L11, L12, L21, L22, tau, dt, nsteps=1):
        p = (p11, p12, p22)
        for _ in range(nsteps):
            p = self.relax_exact(*p, tau, 0.5 * dt)
            p = self.logconf_local_step(*p, L11, L12, L21, L22, INF, dt)
            p = self.relax_exact(*p, tau, 0.5 * dt)
        return p

    def stepper(self, strang):
        return self.logconf_local_step_strang if strang else self.logconf_local_step


NP = Ops()


def lam_max_plane(b11, b12, b22):
    tr = 0.5 * (b11 + b22)
    return tr + np.sqrt(np.maximum(0.25 * (b11 - b22)**2 + b12**2, 0.0))


def min_eig(ops, p):
    b11, b12, b22 = ops.sym_exp(*p)
    tr = 0.5 * (b11 + b22)
    return np.min(tr - np.sqrt(np.maximum(0.25 * (b11 - b22)**2 + b12 * b12, 0.0)))


# ------------------------------------------------------------------ shared inputs --
SHAPES = ((1,), (63,), (64,), (65,), (33, 70), (9, 9))
TAU, DT, G, G_INF = 0.5, 0.01, 0.3, 0.125
# the elementwise launch (viscoelastic.hip VE_MAXB x VE_T, read back through
# rmt_ve_launch_shape by the GPU test): the last of LONG_N cells is the first of a second trip
VE_MAXB, VE_T = 2048, 256
LONG_N = VE_MAXB * VE_T + 1


def key(shape):
    return "x".join(str(s) for s in shape)


def op_inputs(shape):
    """psi (|entries| <= 1.4: eigenvalue gaps are 0 or >= 0.03), a velocity gradient that is
    neither symmetric nor traceless, an SPD b = F F^T and a reference branch, of any shape."""
    n = int(np.prod(shape))
    i = np.arange(n).reshape(shape)
    a = ((i * 7) % 23) * 0.125 - 1.375
    b = ((i * 5) % 19) * 0.0625 - 0.5625
    c = ((i * 3) % 29) * 0.09375 - 1.3125
    L = (((i * 11) % 13) * 0.125 - 0.75, ((i * 2) % 7) * 0.25 - 0.75,
         ((i * 13) % 11) * 0.1875 - 0.9375, ((i * 17) % 5) * 0.25 - 0.5)
    f11, f12, f21, f22 = 1.0 + 0.25 * a, b, 0.25 * c, 1.0 + 0.125 * b
    bb = (f11 * f11 + f12 * f12, f11 * f21 + f12 * f22, f21 * f21 + f22 * f22)
    bref = (1.0 + 0.5 * b * b, 0.25 * a, 1.0 + 0.125 * c * c)
    return dict(psi=(a, b, c), L=L, b=bb, bref=bref)


def special_inputs():
    """One step's special values, a cell each: psi = 0 (exact `deg`, arctan2(0, 0)); diagonal
    psi with a < c and b = +0.0 / -0.0 (theta = +-pi/2); a NaN and an inf cell; l1 = 800 (certain
    overflow of exp); and for sym_log a tensor with a negative eigenvalue (the 1e-300 clamp)."""
    a = np.array([0.0, -0.5, -0.5, np.nan, 0.25, 800.0, 0.0, 0.5])
    b = np.array([0.0, 0.0, -0.0, 0.125, np.inf, 0.0, 0.0, 0.25])
    c = np.array([0.0, 0.75, 0.75, 0.5, 0.5, 1.0, 0.0, -1.0])
    L = (np.full(8, 0.25), np.full(8, -0.5), np.full(8, 0.375), np.full(8, -0.25))
    neg = (np.array([1.0, -2.0, 0.5, 1.0]), np.array([2.0, 0.0, 0.0, 0.0]),
           np.array([1.0, 3.0, 0.5, 1.0]))
    return dict(psi=(a, b, c), L=L, neg=neg)


GAPS = (1e-6, 1e-8, 3e-10, 3e-11, 1e-13)
# e^{-l0} of the ladder's l0, rounded to 5 digits
_L0 = ((0.0, 1.0), (0.5, 0.60653), (-0.75, 2.117), (1.25, 0.2865))
_ROT = ((1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-0.6, 0.8), (0.28, -0.96), (-1.0, 0.0), (0.8, 0.6),
        (-0.8, -0.6))


def gap_inputs(gap):
    """32 cells whose eigenvalues of exp(psi) lie `gap` apart, to a few percent: psi =
    R(theta) diag(l0 + d, l0 - d) R(theta)^T with d = (gap / 2) e^{-l0} s over four l0 and eight
    angles (cos 2 theta, sin 2 theta from Pythagorean pairs).  s = 1.05 on the rungs of the
    quotient branch (gap >= 3e-10) and 0.9 on those of the `deg` branch (gap <= 3e-11), so every
    cell lies on its rung's side of it, by construction."""
    s = 1.05 if gap >= 3e-10 else 0.9
    l0 = np.repeat([v[0] for v in _L0], len(_ROT))
    d = (0.5 * gap * s) * np.repeat([v[1] for v in _L0], len(_ROT))
    c2 = np.tile([r[0] for r in _ROT], len(_L0))
    s2 = np.tile([r[1] for r in _ROT], len(_L0))
    psi = (l0 + d * c2, d * s2, l0 + (-d) * c2)
    n = l0.size
    i = np.arange(n)
    L = (((i * 3) % 7) * 0.25 - 0.75, ((i * 5) % 9) * 0.125 - 0.5, ((i * 2) % 5) * 0.25 - 0.375,
         ((i * 7) % 11) * 0.125 - 0.625)
    return dict(psi=psi, L=L)


def tg_velocity_gradient(N):
    xc = (np.arange(N) + 0.5) * (2 * np.pi / N)
    X, Y = np.meshgrid(xc, xc)
    return (np.sin(X) * np.sin(Y), -np.cos(X) * np.cos(Y), np.cos(X) * np.cos(Y),
            -np.sin(X) * np.sin(Y))


TG_N, TG_STEPS = (16, 33), 50
TG_CASES = ((0.5, 5e-3), (0.5, 0.1), (INF, 0.02))
TG_COMPARE = (16, 0.5, 5e-3, 0.25)


def tg_key(N, tau, dt, strang):
    return f"tg{N}_tau{tau:g}_dt{dt:g}_{'strang' if strang else 'explicit'}"


def tg_run(ops, N, tau, dt, strang, nsteps=TG_STEPS, gaps=None):
    """psi after nsteps from 0 under the frozen Taylor-Green gradient; gaps: a list that gets
    every |lam2 - lam1| plane the right-hand sides of the run see (the states they start from
    and the RK2 predictors)."""
    Lc = tg_velocity_gradient(N)
    p = (np.zeros((N, N)),) * 3
    step = ops.stepper(strang)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(nsteps):
            if gaps is not None:
                q = ops.relax_exact(*p, tau, 0.5 * dt) if strang else p
                t = INF if strang else tau
                k1 = ops.logconf_local_rhs(*q, *Lc, t)
                gaps.append(ops.lam_gap(*q))
                gaps.append(ops.lam_gap(*(q[k] + dt * k1[k] for k in range(3))))
            p = step(*p, *Lc, tau, dt)
    return p


def tg_compare(ops, N, tau, dt, T):
    n = int(round(T / dt))
    pe = tg_run(ops, N, tau, dt, False, n)
    ps = tg_run(ops, N, tau, dt, True, n)
    diff = max(np.nanmax(np.abs(pe[i] - ps[i])) for i in range(3))
    return diff, min_eig(ops, pe), min_eig(ops, ps)


def relaxation_setups():
    """(b0, L, tau) of the three 0-D checks (step strain, steady shear, elastic limit)."""
    return (((1.0 + 0.5**2, 0.5, 1.0), (0.0, 0.0, 0.0, 0.0), 2.0),
            ((1.0, 0.0, 1.0), (0.0, 0.3, 0.0, 0.0), 2.0),
            ((1.0, 0.0, 1.0), (0.0, 0.4, 0.0, 0.0), INF))


# ------------------------------------------------------------------ uniform extension --
UNI_N, UNI_STEPS, UNI_TAUS = 32, 12, (0.5, INF)


class UniformLoop:
    """The uniform-extension loop composed from the oracle's operators and `ops`: the same
    sequence as pyrmt_amd.viscoelastic.UniformExtension, a plane at a time."""

    def __init__(self, O, ops, N=UNI_N, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.02, rho=1.0, R=0.13):
        self.O, self.ops, self.N, self.R = O, ops, N, R
        dx = dy = 1.0 / N
        self.dx, self.dy = dx, dy
        xc = (np.arange(N) + 0.5) * dx
        Xc, Yc = np.meshgrid(xc, xc)
        self.Xg, self.Yg = np.meshgrid(np.arange(N) * dx, np.arange(N) * dy)
        e = eps_rate
        self.u_c = e * (Xc - 0.5); self.v_c = -e * (Yc - 0.5)
        phi = np.sqrt((Xc - 0.5)**2 + (Yc - 0.5)**2) - R
        m = (phi <= 0).astype(float)
        self.X1, self.X2 = O.extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, 3)
        self.psi = [np.zeros((N, N)) for _ in range(3)]
        nu, cs = mu_f / rho, np.sqrt(G / rho)
        self.dt = min(0.25 * dx / max(0.5 * e, 0.1), 0.2 * dx * dx / nu, 0.3 * dx / (cs + 1e-9))
        self.tau = INF if tau <= 0 else tau
        self.t, self.record, self.dts, self.min_abs_phi, self.stopped = 0.0, [], [], INF, False
        self.phi = self.be = None

    def step(self, nsteps=1, t_end=INF):
        O, ops, dx, dy, N = self.O, self.ops, self.dx, self.dy, self.N
        dt = self.dt
        for _ in range(nsteps):
            if self.stopped or not self.t < t_end:
                break
            if self.t + dt > t_end:
                dt = t_end - self.t
            u_c, v_c = self.u_c, self.v_c
            phi = O.rebuild_phi_disc(self.X1, self.X2, 0.5, 0.5, self.R)
            m = (phi <= 0).astype(float)
            adv = lambda q: O.advect_reference_map(q, u_c, v_c, self.Xg, self.Yg, dt, dx, dy, phi,
                                                   'semilagrangian', 0.0) * m
            X1, X2 = adv(self.X1), adv(self.X2)
            self.X1, self.X2 = O.extrapolate_reference_map(X1, X2, phi, dx, dy, 3)
            p11, p12, p22 = (adv(p) for p in self.psi)
            p11, p12 = O.extrapolate_reference_map(p11, p12, phi, dx, dy, 3)
            p22, _ = O.extrapolate_reference_map(p22, np.zeros((N, N)), phi, dx, dy, 3)
            Lc = (O.grad_central_x_2nd(u_c, dx), O.grad_central_y_2nd(u_c, dy),
                  O.grad_central_x_2nd(v_c, dx), O.grad_central_y_2nd(v_c, dy))
            self.psi = list(ops.logconf_local_step(p11, p12, p22, *Lc, self.tau, dt))
            self.be = ops.sym_exp(*self.psi)
            self.t += dt
            sm = phi <= 0
            lam = float(lam_max_plane(*self.be)[sm].max()) if sm.any() else np.nan
            self.phi = phi
            self.min_abs_phi = min(self.min_abs_phi, float(np.abs(phi).min()))
            self.record.append((self.t, lam, float(self.be[0][N // 2, N // 2]), int(sm.sum())))
            self.dts.append(dt)
            if not sm.any() or lam > 1e3:
                self.stopped = True
        return self


# ----------------------------------------------------------------------------- bars --
# Every transcendental case is held to BAR_FACTOR times its measured floor: the largest
# difference, over 20 repeats, between the restatement and itself with every exp, log, sin, cos
# and arctan2 result moved by -1, 0 or +1 ulp at random (tools/ve_floor.py writes
# profiles/viscoelastic/floor.json).  4: the device library's documented fp64 bounds reach 2 ulp
# where the nudge is 1, and a random nudge understates the worst case.
BAR_FACTOR = 4.0
FLOOR_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                          "profiles", "viscoelastic", "floor.json")


def floors():
    with open(FLOOR_JSON) as f:
        return json.load(f)["floors"]


def bar(case):
    """The bar of a case of floor.json."""
    return BAR_FACTOR * FLOORS[case]


FLOORS = floors() if os.path.exists(FLOOR_JSON) else {}


def assert_close(got, ref, case, what=""):
    """The NaN and the inf pattern (with signs) equal, the finite values within bar(case); the
    figure is printed before it is asserted."""
    got, ref = np.stack([np.asarray(p) for p in got]), np.asarray(ref)
    assert got.shape == ref.shape, (what or case, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what} NaN pattern")
    inf = np.isinf(ref)
    np.testing.assert_array_equal(np.isinf(got), inf, err_msg=f"{what} inf pattern")
    np.testing.assert_array_equal(got[inf], ref[inf])
    ok = np.isfinite(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print(f"{what or case}: max err {err:.3e}, bar {bar(case):.3e}")
    assert err <= bar(case), (what or case, err, bar(case))


def same_bits(a, b):
    """== on the bit patterns (tells -0.0 from +0.0, and compares NaNs)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# the reduction's launch (viscoelastic.hip VL_RB x VL_T): a constant shape, so a cell at a flat
# index >= LAM_TRIP is read on a workgroup's second trip whatever n is
LAM_TRIP = 256 * 256
