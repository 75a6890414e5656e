"""The viscoelastic constitutive layer (pyRMT/viscoelastic.py) on the device: the
upper-convected Maxwell update of the elastic Finger tensor b_e, its log-conformation form
psi = log(b_e) with the explicit RK2 and the Strang (exact relaxation) steppers, the matrix
log / exp of a symmetric 2 x 2 field and the stress -- the reference's names, signatures and
return shapes over viscoelastic.hip -- and the three drivers that need nothing but this layer:

    relaxation_tests      benchmarks/viscoelastic_relaxation_test.py   (0-D)
    tg_run_compare        benchmarks/viscoelastic_taylor_green.py      (frozen L, every cell)
    UniformExtension      benchmarks/mac_viscoelastic_uniform.py       (imposed extension)

Inputs are NumPy arrays, device tensors or scalars; the arrays of a call share one shape (any
shape: the kernels are elementwise), scalars are broadcast to full planes here.  Results come
back in the caller's array type; a call whose inputs are all scalars returns Python floats.
The steppers take `nsteps`: that many steps in one launch, the state in registers in between,
with the bits of `nsteps` single calls.  ucm_* and viscoelastic_stress give the reference's
bits; the others differ from it through exp, log, sin, cos and atan2 alone (DESIGN.md
section 18).  The coupled four-roll-mill driver (mac_viscoelastic_extension, elastic IMEX)
stands on this layer in pyrmt_amd.mac (MacViscoelasticExtension); the lid
cavity's mac_viscoelastic_disc is not built."""
import ctypes
import math

import numpy as np

from . import _lib as L
from .functions import (_IO, _p, _plane_ptrs, _torch, _advect_sl_rk4_multi, ctx_for,
                        extrapolate_reference_map, grad_central_x_2nd, grad_central_y_2nd)

__all__ = ["ucm_local_rhs", "ucm_local_step", "sym_log", "sym_exp", "logconf_local_rhs",
           "logconf_local_step", "logconf_local_step_strang", "relax_exact",
           "viscoelastic_stress", "lam_max", "relaxation_tests", "tg_velocity_gradient",
           "tg_run_compare", "UniformExtension", "ve_uniform_run"]

MAX_FUSED = 100000   # steps per launch of a driver (one cell's steps run one after another)


def _ctx():
    """The elementwise entries take n themselves: one small context carries their stream."""
    return ctx_for(5, 5)


def _is_scalar(v):
    return np.ndim(v) == 0 if not hasattr(v, "dim") else v.dim() == 0


class _Planes:
    """The planes of one call: their common shape (ValueError on a mismatch), scalars broadcast
    to it, results back in the caller's type (floats when every input was a scalar)."""

    def __init__(self, what, *vals):
        arrays = [v for v in vals if v is not None and not _is_scalar(v)]
        shapes = {tuple(v.shape) for v in arrays}
        if len(shapes) > 1:
            raise ValueError(f"{what}: arrays of one shape, got {sorted(shapes)}")
        self.shape = shapes.pop() if shapes else ()
        self.n = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        if self.n < 1:
            raise ValueError(f"{what}: empty arrays")
        self.io = _IO(*arrays)
        self.floats = not arrays
        self.keep = []

    def dev(self, v):
        if _is_scalar(v):
            t = self.io.torch.full(self.shape or (1,), float(v), dtype=self.io.torch.float64,
                                   device="cuda")
        else:
            t = self.io.dev(v)
        self.keep.append(t)
        return t

    def ptrs(self, vals):
        return _plane_ptrs([self.dev(v) for v in vals])

    def out3(self):
        o = self.io.empty((3,) + (self.shape or (1,)))
        return o, _plane_ptrs([o[0], o[1], o[2]])

    def result(self, o):
        if self.floats:
            return tuple(o[:, 0].tolist())
        return tuple(self.io.out(o[k]) for k in range(3))


def _rhs(entry, what, s, Lc, tau):
    P = _Planes(what, *s, *Lc)
    o, op = P.out3()
    L.check(getattr(L.lib(), entry)(_ctx().bind(), P.n, P.ptrs(s), P.ptrs(Lc), float(tau), op),
            what)
    return P.result(o)


def _nsteps(what, nsteps):
    if int(nsteps) != nsteps or nsteps < 1:
        raise ValueError(f"{what}: nsteps is a whole number >= 1")
    return int(nsteps)


# ------------------------------------------------------------------------------ UCM --
def ucm_local_rhs(b11, b12, b22, L11, L12, L21, L22, tau):
    """viscoelastic.py:27-42: L b + b L^T - (1 / tau)(b - I) per component (an entry of its own,
    rmt_ve_ucm_rhs; the reference's bits)."""
    return _rhs("rmt_ve_ucm_rhs", "ucm_local_rhs", (b11, b12, b22), (L11, L12, L21, L22), tau)


def ucm_local_step(b11, b12, b22, L11, L12, L21, L22, tau, dt, nsteps=1):
    """viscoelastic.py:45-54: one explicit RK2 (Heun) step of the homogeneous UCM evolution, or
    `nsteps` of them in one launch; the reference's bits."""
    k = _nsteps("ucm_local_step", nsteps)
    P = _Planes("ucm_local_step", b11, b12, b22, L11, L12, L21, L22)
    o, op = P.out3()
    L.check(L.lib().rmt_ve_ucm_steps(_ctx().bind(), P.n, P.ptrs((b11, b12, b22)),
                                     P.ptrs((L11, L12, L21, L22)), float(tau), float(dt), k,
                                     None, op, None), "ucm_local_step")
    return P.result(o)


def viscoelastic_stress(b11, b12, b22, G, b_ref=None, G_inf=0.0):
    """viscoelastic.py:167-179: G b_e, plus G_inf b_ref (a triple) for the standard linear
    solid; the reference's bits, its `b_ref is not None and G_inf != 0.0` branch included."""
    if b_ref is not None and len(b_ref) != 3:
        raise ValueError("viscoelastic_stress: b_ref is (bxx, bxy, byy)")
    P = _Planes("viscoelastic_stress", b11, b12, b22, *(b_ref or ()))
    o, op = P.out3()
    rp = P.ptrs(b_ref) if b_ref is not None else None
    L.check(L.lib().rmt_ve_stress(_ctx().bind(), P.n, P.ptrs((b11, b12, b22)), float(G), rp,
                                  float(G_inf), op), "viscoelastic_stress")
    return P.result(o)


# ----------------------------------------------------------------- log-conformation --
def _sym_fn(entry, what, a, b, c):
    P = _Planes(what, a, b, c)
    o, op = P.out3()
    L.check(getattr(L.lib(), entry)(_ctx().bind(), P.n, P.ptrs((a, b, c)), op), what)
    return P.result(o)


def sym_log(a, b, c):
    """viscoelastic.py:71-76: the matrix log of the symmetric field [[a, b], [b, c]]
    (eigenvalues clamped at 1e-300)."""
    return _sym_fn("rmt_ve_sym_log", "sym_log", a, b, c)


def sym_exp(a, b, c):
    """viscoelastic.py:79-84: the matrix exp of the symmetric field [[a, b], [b, c]]."""
    return _sym_fn("rmt_ve_sym_exp", "sym_exp", a, b, c)


def logconf_local_rhs(p11, p12, p22, L11, L12, L21, L22, tau):
    """viscoelastic.py:87-116: the right-hand side of the homogeneous log-conformation
    evolution in the eigenframe of psi (Fattal-Kupferman)."""
    return _rhs("rmt_ve_logconf_rhs", "logconf_local_rhs", (p11, p12, p22),
                (L11, L12, L21, L22), tau)


def _logconf_steps(what, strang, p11, p12, p22, L11, L12, L21, L22, tau, dt, nsteps):
    k = _nsteps(what, nsteps)
    P = _Planes(what, p11, p12, p22, L11, L12, L21, L22)
    o, op = P.out3()
    L.check(L.lib().rmt_ve_logconf_steps(_ctx().bind(), P.n, P.ptrs((p11, p12, p22)),
                                         P.ptrs((L11, L12, L21, L22)), float(tau), float(dt), k,
                                         strang, op), what)
    return P.result(o)


def logconf_local_step(p11, p12, p22, L11, L12, L21, L22, tau, dt, nsteps=1):
    """viscoelastic.py:119-125: one explicit RK2 step of psi = log(b_e), or `nsteps` in one
    launch (the bits of `nsteps` single calls)."""
    return _logconf_steps("logconf_local_step", 0, p11, p12, p22, L11, L12, L21, L22, tau, dt,
                          nsteps)


def logconf_local_step_strang(p11, p12, p22, L11, L12, L21, L22, tau, dt, nsteps=1):
    """viscoelastic.py:150-164: relax(dt / 2), stretch(dt), relax(dt / 2) with the relaxation
    integrated exactly, or `nsteps` such steps in one launch; with tau = inf the bits of
    logconf_local_step at tau = inf."""
    return _logconf_steps("logconf_local_step_strang", 1, p11, p12, p22, L11, L12, L21, L22, tau,
                          dt, nsteps)


def relax_exact(p11, p12, p22, tau, dt):
    """viscoelastic.py:133-147: psi after the exact relaxation b_e <- I + (b_e - I) exp(-dt / tau);
    tau = inf or dt == 0.0 returns the input's bits (no exp / log round trip)."""
    P = _Planes("relax_exact", p11, p12, p22)
    o, op = P.out3()
    L.check(L.lib().rmt_ve_relax_exact(_ctx().bind(), P.n, P.ptrs((p11, p12, p22)), float(tau),
                                       float(dt), op), "relax_exact")
    return P.result(o)


def lam_max(b11, b12, b22, phi, at=0, out=None):
    """benchmarks/mac_viscoelastic_uniform.py:30-32, :90-92 as one reduction: three doubles,
    the largest eigenvalue of b over phi <= 0 (NaN propagates; -inf without such a cell), the
    number of those cells and b11 at the flat index `at` (a device tensor for device inputs,
    written into `out` when given)."""
    P = _Planes("lam_max", b11, b12, b22, phi)
    o = P.io.empty((3,)) if out is None else out
    L.check(L.lib().rmt_ve_lam_max(_ctx().bind(), P.n, P.ptrs((b11, b12, b22)), _p(P.dev(phi)),
                                   int(at), _p(o)), "lam_max")
    return P.io.out(o)


# -------------------------------------------------------------------------- drivers --
def _ucm_run(b, Lc, tau, dt, nsteps, track=None):
    """`nsteps` UCM steps of one cell in launches of at most MAX_FUSED; with `track` (three
    entries, each None or nsteps host values) also the largest |component - track| met."""
    torch = _torch()
    dev = lambda a: torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)), device="cuda")
    s, Ld = [dev(v) for v in b], [dev(v) for v in Lc]   # (kept: the pointer arrays own nothing)
    Lp = _plane_ptrs(Ld)
    tr = [None if t is None else dev(t) for t in (track or ())]
    err, worst = (torch.zeros(1, dtype=torch.float64, device="cuda"), 0.0) if track else (None, 0.0)
    c = _ctx()
    for k0 in range(0, nsteps, MAX_FUSED):
        k = min(MAX_FUSED, nsteps - k0)
        tp = None
        if track:
            tp = (ctypes.c_void_p * 3)(*[None if t is None else t[k0:].data_ptr() for t in tr])
        sp = _plane_ptrs(s)
        L.check(L.lib().rmt_ve_ucm_steps(c.bind(), 1, sp, Lp, float(tau), float(dt), k, tp, sp,
                                         _p(err)), "ucm steps")
        if track:
            worst = max(worst, err.item())
    return [t.item() for t in s], worst


def relaxation_tests(dt=2e-4):
    """The three checks of benchmarks/viscoelastic_relaxation_test.py (:27-83) as (e1, e2, e3):
    stress relaxation after a step strain, steady simple shear, and the elastic limit
    tau = inf against F F^T.  Each is a few fused launches on a one-cell state.  The running
    maxima of the first and third need every intermediate state: the kernel carries them
    (rmt_ve_ucm_steps' track / out_err), compared with the exact values of every step, which
    the host computes beforehand (the decay exp(-t / tau); F under the same RK2)."""
    tau, gamma, gdot2, gdot3 = 2.0, 0.5, 0.3, 0.4
    n1, n2, n3 = (int(round(T / dt)) for T in (10.0, 80.0, 2.0))
    exact = gamma * np.exp(-(np.arange(1, n1 + 1) * dt) / tau)                        # :34-35
    _, e1 = _ucm_run((1.0 + gamma**2, gamma, 1.0), (0.0,) * 4, tau, dt, n1, (None, exact, None))
    b, _ = _ucm_run((1.0, 0.0, 1.0), (0.0, gdot2, 0.0, 0.0), tau, dt, n2)             # :43-53
    e2 = max(abs(b[1] - tau * gdot2), abs(b[0] - (1.0 + 2.0 * tau**2 * gdot2**2)),
             abs(b[2] - 1.0))
    L11, L12, L21, L22 = 0.0, gdot3, 0.0, 0.0                                         # :64-80
    F11, F12, F21, F22 = 1.0, 0.0, 0.0, 1.0
    fr = lambda a11, a12, a21, a22: (L11*a11 + L12*a21, L11*a12 + L12*a22,
                                     L21*a11 + L22*a21, L21*a12 + L22*a22)
    bb = np.empty((3, n3))
    for k in range(n3):
        k1 = fr(F11, F12, F21, F22)
        k2 = fr(F11 + dt*k1[0], F12 + dt*k1[1], F21 + dt*k1[2], F22 + dt*k1[3])
        F11 += 0.5*dt*(k1[0] + k2[0]); F12 += 0.5*dt*(k1[1] + k2[1])
        F21 += 0.5*dt*(k1[2] + k2[2]); F22 += 0.5*dt*(k1[3] + k2[3])
        bb[:, k] = (F11*F11 + F12*F12, F11*F21 + F12*F22, F21*F21 + F22*F22)
    _, e3 = _ucm_run((1.0, 0.0, 1.0), (L11, L12, L21, L22), math.inf, dt, n3, tuple(bb))
    return e1, e2, e3


def tg_velocity_gradient(N):
    """viscoelastic_taylor_green.py:39-47: the Taylor-Green velocity gradient at the cell
    centres of [0, 2 pi]^2 (host, set-up)."""
    xc = (np.arange(N) + 0.5) * (2 * np.pi / N)
    X, Y = np.meshgrid(xc, xc)
    return (np.sin(X) * np.sin(Y), -np.cos(X) * np.cos(Y), np.cos(X) * np.cos(Y),
            -np.sin(X) * np.sin(Y))


def _min_eig(torch, p):
    b11, b12, b22 = sym_exp(*p)                                                       # :50-55
    tr = 0.5 * (b11 + b22)
    d = torch.sqrt(torch.clamp(0.25 * (b11 - b22) ** 2 + b12 * b12, min=0.0))
    return (tr - d).min().item()


def tg_run_compare(N=64, tau=0.5, dt=1e-3, T=2.0):
    """viscoelastic_taylor_green.run_compare (:58-76) on device tensors: psi from 0 under the
    frozen Taylor-Green gradient with both steppers, int(round(T / dt)) steps each in fused
    launches; (max |psi_explicit - psi_strang| with nanmax's rule, min eigenvalue of b_e
    explicit, the same for Strang)."""
    torch = _torch()
    Lc = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tg_velocity_gradient(N)]
    nsteps = int(round(T / dt))
    runs = []
    for step in (logconf_local_step, logconf_local_step_strang):
        p = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for _ in range(3)]
        for k0 in range(0, nsteps, MAX_FUSED):
            p = step(*p, *Lc, tau, dt, nsteps=min(MAX_FUSED, nsteps - k0))
        runs.append(p)
    pe, ps = runs
    diffs = []
    for a, b in zip(pe, ps):
        d = (a - b).abs()
        d = d[~torch.isnan(d)]
        diffs.append(d.max().item() if d.numel() else math.nan)
    return max(diffs), _min_eig(torch, pe), _min_eig(torch, ps)


class UniformExtension:
    """The loop body of benchmarks/mac_viscoelastic_uniform.py:70-99 on device tensors,
    composed from operators: a soft blob (radius R at the centre) in the imposed planar
    extension u = (eps (x - 1/2), -eps (y - 1/2)), which is never advanced.  A step: phi
    rebuilt from the map, the five planes X1, X2, p11, p12, p22 advected on one backtrace and
    masked, three extrapolations (p22 with a zero partner), logconf_local_step, sym_exp and the
    rmt_ve_lam_max reduction, whose three doubles are the step's one host read.  tau <= 0 means
    inf.  The velocity and its gradient are the same every step and are formed once.

    `record`: one (t, lam_max, b_xx(centre)) per step (lam_max NaN without a solid cell);
    `dts`: the step sizes; history() is the reference's every-50th-step view.  The loop stops
    (`stopped`) without a solid cell or with lam_max > 1e3 (:95)."""

    LAYERS = 3

    def __init__(self, N=96, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.02, rho=1.0, R=0.13):
        torch = _torch()
        self.torch, self.N, self.R, self.eps = torch, int(N), float(R), eps_rate
        N, e = self.N, eps_rate
        dx, dy = 1.0 / N, 1.0 / N
        self.dx, self.dy = dx, dy
        xc = (np.arange(N) + 0.5) * dx
        Xc, Yc = np.meshgrid(xc, xc)
        Xg, Yg = np.meshgrid(np.arange(N) * dx, np.arange(N) * dy)
        dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).cuda()
        u_c = e * (Xc - 0.5); v_c = -e * (Yc - 0.5)                                   # :74
        self.umax = float(np.max(np.abs(u_c)))
        phi = np.sqrt((Xc - 0.5)**2 + (Yc - 0.5)**2) - R                              # :53-55
        m = (phi <= 0).astype(float)
        X1, X2 = extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, self.LAYERS)
        self.Xg, self.Yg, self.u_c, self.v_c, self.X1, self.X2 = map(dev, (Xg, Yg, u_c, v_c,
                                                                            X1, X2))
        self.psi = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for _ in range(3)]
        self.zero = torch.zeros((N, N), dtype=torch.float64, device="cuda")
        self.Lc = [grad_central_x_2nd(self.u_c, dx), grad_central_y_2nd(self.u_c, dy),  # :84-85
                   grad_central_x_2nd(self.v_c, dx), grad_central_y_2nd(self.v_c, dy)]
        nu, cs = mu_f / rho, np.sqrt(G / rho)
        self.dt = float(min(0.25 * dx / max(0.5 * e, 0.1), 0.2 * dx * dx / nu,
                            0.3 * dx / (cs + 1e-9)))                                    # :60
        self.tau = math.inf if tau <= 0 else float(tau)                                # :61-62
        self.Wi = e * self.tau
        self.bxx_analytic = (math.inf if (self.tau == math.inf or self.Wi >= 0.5)
                             else 1.0 / (1.0 - 2.0 * self.Wi))
        self.ctx = ctx_for(N, N)
        self.be = torch.empty((3, N, N), dtype=torch.float64, device="cuda")
        self.stats = torch.empty(3, dtype=torch.float64, device="cuda")
        self.phi = None
        self.t, self.nsteps, self.stopped, self.record, self.dts = 0.0, 0, False, [], []

    def step(self, nsteps=1, t_end=None):
        torch, lib, N, dx, dy = self.torch, L.lib(), self.N, self.dx, self.dy
        t_end = math.inf if t_end is None else t_end
        dt, n, at = self.dt, N * N, (N // 2) * N + N // 2
        for _ in range(int(nsteps)):
            if self.stopped or not self.t < t_end:
                break
            if self.t + dt > t_end:
                dt = t_end - self.t                                                # :72-73
            phi = torch.empty_like(self.X1)
            L.check(lib.rmt_rebuild_phi_disc(self.ctx.bind(), _p(self.X1), _p(self.X2), 0.5, 0.5,
                                             self.R, _p(phi)), "rebuild_phi")          # :75
            qs = [self.X1, self.X2] + self.psi
            outs = [torch.empty_like(q) for q in qs]
            _advect_sl_rk4_multi(self.ctx, qs, self.u_c, self.v_c, self.Xg, self.Yg, dt, dx, dy,
                                 phi, outs)                                        # :76-81
            self.X1, self.X2 = extrapolate_reference_map(outs[0], outs[1], phi, dx, dy,
                                                         self.LAYERS)
            p11, p12 = extrapolate_reference_map(outs[2], outs[3], phi, dx, dy, self.LAYERS)
            p22, _ = extrapolate_reference_map(outs[4], self.zero, phi, dx, dy, self.LAYERS)
            self.psi = [p11, p12, p22]
            pp, bp = _plane_ptrs(self.psi), _plane_ptrs([self.be[0], self.be[1], self.be[2]])
            L.check(lib.rmt_ve_logconf_steps(self.ctx.bind(), n, pp, _plane_ptrs(self.Lc),
                                             self.tau, dt, 1, 0, pp), "logconf_local_step")
            L.check(lib.rmt_ve_sym_exp(self.ctx.bind(), n, pp, bp), "sym_exp")         # :86-87
            L.check(lib.rmt_ve_lam_max(self.ctx.bind(), n, bp, _p(phi), at, _p(self.stats)),
                    "lam_max")
            self.t += dt
            self.nsteps += 1
            lam, count, bxx_c = self.stats.tolist()              # the step's one host read
            solid = count > 0
            if not solid:
                lam = math.nan                                                     # :91
            self.phi = phi
            self.record.append((self.t, lam, bxx_c))
            self.dts.append(dt)
            if not solid or lam > 1e3:                                                 # :95
                self.stopped = True
        return self

    def history(self, t_end=math.inf):
        """The reference's `hist` (:93-94): every 50th step and those at t >= t_end, each
        (t, lam_max, b_xx(centre), max|u_c|)."""
        return [r + (self.umax,) for k, r in enumerate(self.record, 1)
                if k % 50 == 0 or r[0] >= t_end]

    def get(self, name):
        """Host copy of X1, X2, phi, p11, p12, p22 or be11, be12, be22."""
        planes = dict(X1=self.X1, X2=self.X2, phi=self.phi, p11=self.psi[0], p12=self.psi[1],
                      p22=self.psi[2], be11=self.be[0], be12=self.be[1], be22=self.be[2])
        return planes[name].cpu().numpy()


def ve_uniform_run(N=96, t_end=8.0, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.02, rho=1.0, R=0.13,
                   return_sim=False):
    """mac_viscoelastic_uniform.run (:35-108): integrate to t_end or to the stop; returns
    (t, hist) as the reference does (return_sim: (t, hist, the UniformExtension))."""
    if not math.isfinite(t_end):
        raise ValueError("ve_uniform_run: a finite t_end")
    sim = UniformExtension(N, tau, eps_rate, G, mu_f, rho, R).step(2**31 - 1, t_end)
    hist = sim.history(t_end)
    return (sim.t, hist, sim) if return_sim else (sim.t, hist)
