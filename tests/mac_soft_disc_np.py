"""Shared pieces of the soft-disc integrator-ladder tests (benchmarks/mac_soft_disc_lid.py;
tests/golden/gen_mac_soft_disc.py writes the fixture, tests/test_mac_soft_disc_cpu.py and
tests/test_gpu_mac_soft_disc.py read it): the traces' parameters, the operator inputs (built
from +, * and sqrt on index grids alone, correctly rounded everywhere, so the generator and the
tests hold the same bits without storing them), and a NumPy restatement of the four new
operators and of one loop step per rung (the expensive operators through the oracle)."""
import numpy as np

from mac_faces_np import faces_of_stress

# ---------------------------------------------------------------- traces ----
N = 32
DX = 1.0 / N
DT_REF = min(0.3 * DX, 0.2 * DX * DX / 0.01)          # 0.009375
# name -> (run() keywords, steps, the steps whose state before and after is kept).
# A kept step is a one-step case of the tests, held to 1e-12 on u, v and the maps.  That is a
# fair demand only where the reference's own step does not move by more than a tenth of it when
# one face-force value moves by one ulp (map_noise below, measured on the CPU by the generator).
# In the elastic rungs the maps are advanced with the new velocity, whose last bits depend on
# the rounding of the force and the CG; a map value inside the solid that flips its last bit
# moves the third extrapolated layer by up to 2e-12 (three chained least-squares fits, ~1e4 x),
# and a step in which some cell's interpolant lies that close to a rounding boundary answers
# most nudges so.  Measured with 24 nudges a step (velocity / maps): explicit, imex, imex-sl and
# weno5 maps 0 everywhere (their maps never see the new velocity); imex-elastic 0 but for steps
# 14 (8e-13) and 25 (2e-16); the stiff disc 0 at step 16 only, else 9e-13..2e-12;
# imex-elastic-sl 0 at step 7 and 2e-16 at step 11, else 6e-13..2e-12, its three central-branch
# steps included (1e-12, 1e-12, 2e-12): both kept steps of that rung take the semi-Lagrangian
# branch, and the central branch of the switch has its one-step case in imex-sl, step 2, its
# elastic predictor in imex-elastic.
TRACES = {
    "explicit": (dict(integrator="explicit", dt=DT_REF), 30, (12, 30)),
    "imex": (dict(integrator="imex", dt=DT_REF), 30, (30,)),
    "elastic": (dict(integrator="imex-elastic", dt=DT_REF), 30, (12, 30)),
    "stiff": (dict(integrator="imex-elastic", mu_s=8.0, dt=0.3 * DX), 20, (16,)),
    "imex_sl": (dict(integrator="imex-sl", dt=5 * DT_REF), 18, (2, 18)),
    "elastic_sl": (dict(integrator="imex-elastic-sl", dt=5 * DT_REF), 18, (7, 11)),
    "weno5": (dict(integrator="explicit", dt=DT_REF, scheme="weno5"), 10, (10,)),
}
T_END_SL = 0.8
STEP_BAR, NOISE_NUDGES = 1e-12, 24
CFL_SWITCH = 0.9
X0, Y0, R = 0.6, 0.5, 0.2
MU_F, RHO, U_LID, KAPPA, NL = 0.01, 1.0, 1.0, 0.0, 3


def t_end_of(name):
    """The t_end that gives the trace its step count (dt is not clipped to it)."""
    kw, steps, _ = TRACES[name]
    return T_END_SL if name.endswith("_sl") else (steps - 0.5) * kw["dt"]


# ---------------------------------------------------------------- operator inputs ----
SHAPES = ((5, 5), (6, 6), (33, 70), (65, 64), (97, 97))
BOX = (1.0, 1.25)
MU_S, W_CUT_FAC = 0.1, 0.5
FORCE_VARIANTS = ((False, 0.0), (True, 0.0), (False, 5.0), (True, 5.0))   # (isochoric, detg_clamp)


def stored_variants(shape):
    """The variants whose reference outputs the fixture holds: all four below 3000 cells, the
    two opposite ones above (the fused kernel is held to its own unfused composition in all four
    at every size, which needs no fixture)."""
    return FORCE_VARIANTS if shape[0] * shape[1] < 3000 else (FORCE_VARIANTS[0], FORCE_VARIANTS[3])


def key(shape):
    return f"{shape[0]}x{shape[1]}"


def vkey(iso, clamp):
    return f"{'iso' if iso else 'dev'}{int(clamp)}"


def op_inputs(shape):
    """A (ny, nx) cell grid on [0, 1] x [0, 1.25] (dx != dy): a disc of radius 0.3 (solid cells
    already at 5 x 5), maps whose detG falls below 1 / 5 at the disc's lower edge (the clamp at 5
    fires there), two swirls on the faces (wall faces not zeroed) whose first
    reaches a face CFL of 0.5 at `dt`, and w_cut = dx / 2 with phi on both sides of it."""
    ny, nx = shape
    dx, dy = BOX[0] / nx, BOX[1] / ny
    xc, yc = (np.arange(nx) + 0.5) * dx, (np.arange(ny) + 0.5) * dy
    xf, yf = np.arange(nx + 1) * dx, np.arange(ny + 1) * dy
    Xc, Yc = np.meshgrid(xc, yc)
    Xu, Yu = np.meshgrid(xf, yc)
    Xv, Yv = np.meshgrid(xc, yf)
    phi = np.sqrt((Xc - 0.45) ** 2 + (Yc - 0.6) ** 2) - 0.3
    X1 = Xc * (0.0625 + Yc * Yc) + 0.0625 * Yc
    X2 = Yc + 0.09375 * Xc * Xc + 0.0625 * Xc * Yc
    u0 = -1.5 * (Yu - 0.6) + 0.25 * Xu * Yu
    v0 = 1.5 * (Xv - 0.45) - 0.125 * Yv * Yv
    u1 = 0.75 * u0 + 0.125 * Xu * Xu
    v1 = 0.875 * v0 - 0.0625 * Xv * Yv
    dt = 0.5 / max(np.abs(u0).max() / dx, np.abs(v0).max() / dy)
    return dict(dx=dx, dy=dy, w_t=2.0 * dx, w_cut=W_CUT_FAC * dx, dt=dt, phi=phi, X1=X1, X2=X2,
                u0=u0, v0=v0, u1=u1, v1=v1)


# ---------------------------------------------------------------- the new operators ----
def midpoint_centres(u0, v0, u1, v1):
    """mac_soft_disc_lid.py:133-134."""
    um = 0.5 * (u0 + u1); vm = 0.5 * (v0 + v1)
    return 0.5 * (um[:, :-1] + um[:, 1:]), 0.5 * (vm[:-1, :] + vm[1:, :])


def _xi_flux_div_faces(xi, u, v, dx, dy):
    ny, nx = xi.shape
    xu = np.empty((ny, nx + 1))
    xu[:, 1:-1] = 0.5 * (xi[:, :-1] + xi[:, 1:])
    xu[:, 0] = xi[:, 0]; xu[:, -1] = xi[:, -1]
    fx = u * xu
    xv = np.empty((ny + 1, nx))
    xv[1:-1, :] = 0.5 * (xi[:-1, :] + xi[1:, :])
    xv[0, :] = xi[0, :]; xv[-1, :] = xi[-1, :]
    fy = v * xv
    return (fx[:, 1:] - fx[:, :-1]) / dx + (fy[1:, :] - fy[:-1, :]) / dy


def advect_xi_conservative(xi, u, v, dx, dy, dt, phi, w_cut=0.0):
    """mac.py:713-721."""
    H = (phi <= w_cut).astype(float)
    rhs = lambda q: -H * _xi_flux_div_faces(q, u, v, dx, dy)
    q1 = xi + dt * rhs(xi)
    q2 = 0.75 * xi + 0.25 * (q1 + dt * rhs(q1))
    return (1.0 / 3.0) * xi + (2.0 / 3.0) * (q2 + dt * rhs(q2))


def solid_force(O, X1, X2, phi, dx, dy, w_t, mu_s, kappa=0.0, detg_clamp=0.0, isochoric=False):
    """mac_soft_disc_lid.py:103-110 on the operators of O (the oracle, or the reference's
    functions module): (fu, fv, J, the three blended stresses)."""
    sxx, sxy, syy, J = O.solid_cauchy_stress(X1, X2, dx, dy, mu_s, kappa, phi,
                                             detg_clamp=detg_clamp, isochoric=isochoric)
    H = O.smoothed_heaviside(phi, w_t)
    Sxx = (1 - H) * sxx; Sxy = (1 - H) * sxy; Syy = (1 - H) * syy
    fu, fv = faces_of_stress(O, Sxx, Sxy, Syy, dx, dy)
    return fu, fv, J, (Sxx, Sxy, Syy)


def soft_diag(phi, J, u, v, dx, dy):
    """What mac_soft_disc_lid.py:139-150 reads: (count, sum Xc, sum Yc, min J, max J, max|u|,
    max|v|, non-finite flag) with the driver's own cell centres."""
    ny, nx = phi.shape
    Xc, Yc = np.meshgrid((np.arange(nx) + 0.5) * dx, (np.arange(ny) + 0.5) * dy)
    m = phi <= 0
    bad = not (np.all(np.isfinite(u)) and np.all(np.isfinite(v)))
    return np.array([m.sum(), Xc[m].sum(), Yc[m].sum(), J.min(), J.max(), np.abs(u).max(),
                     np.abs(v).max(), float(bad)])


def force_bar(S, phi, w_t, dx, dy):
    """The bars of the fused force against the reference: the blended stress behind the device
    sine to 1e-14 of its amplitude in the band where H is a sine; a one-sided difference sums
    (3 + 4 + 1) S over 2 h, a divergence two of them, a face the mean of two divergences."""
    band = np.abs(phi) <= w_t
    amp = max(float(np.abs(s[band]).max()) for s in S) if band.any() else 0.0
    return 1e-14 * amp, 1e-14 * amp * 8.0 / min(dx, dy)


# ---------------------------------------------------------------- one loop step ----
def resolve(integrator):
    """:57-62 for the canonical names the traces use: (use_semilag, use_imex, use_elastic)."""
    sl = integrator.endswith("-sl")
    base = integrator[:-3] if sl else integrator
    return sl, sl or base in ("imex", "imex-elastic"), base == "imex-elastic"


def step(O, MO, s, integrator, dt, mu_s=0.1, scheme="semilagrangian", n=N, nudge=None):
    """One pass of mac_soft_disc_lid.py:79-150 from the state s (u, v, X1, X2) on the oracle's
    operators (O: oracle.oracle, MO: oracle.mac_oracle).  Returns the new state, with J, phi
    (the one the stop test reads) and sl (the semi-Lagrangian branch was taken).
    nudge = (trial, rng): map_noise's probe, one non-zero face force moved by one ulp."""
    dx = dy = 1.0 / n
    Xg, Yg = np.meshgrid(np.arange(n) * dx, np.arange(n) * dy)
    use_sl, use_imex, use_el = resolve(integrator)
    nu, w_t, cs = MU_F / RHO, 2.0 * dx, np.sqrt(mu_s / RHO)
    wc = (4.0 if scheme in ("central2", "weno5") else 0.0) * dx
    u, v, X1, X2 = s["u"], s["v"], s["X1"], s["X2"]
    adv = lambda q, a, b, phi: O.advect_reference_map(q, a, b, Xg, Yg, dt, dx, dy, phi, scheme, wc)
    u_c, v_c = midpoint_centres(u, v, u, v)
    phi = O.rebuild_phi_disc(X1, X2, X0, Y0, R)
    sm = (phi <= 0).astype(float)
    if not use_el:
        X1, X2 = O.extrapolate_reference_map(adv(X1, u_c, v_c, phi) * sm, adv(X2, u_c, v_c, phi) * sm,
                                             phi, dx, dy, NL)
        phi = O.rebuild_phi_disc(X1, X2, X0, Y0, R)
    fu, fv, J, _ = solid_force(O, X1, X2, phi, dx, dy, w_t, mu_s, KAPPA)
    if nudge is not None:
        trial, rng = nudge
        f = (fu, fv)[trial % 2]
        k = rng.choice(np.flatnonzero(f))
        f.flat[k] = np.nextafter(f.flat[k], (-1) ** (trial // 2) * np.inf)
    cs2 = cs * cs if use_el else 0.0
    sl = False
    if use_sl:
        sl = dt * max(np.abs(u).max() / dx, np.abs(v).max() / dy) > CFL_SWITCH
        us, vs = MO.momentum_predictor_lid_semilag(u, v, nu, dx, dy, dt, U_LID, fu=fu, fv=fv,
                                                   rho=RHO, cs2=cs2)
    elif use_imex:
        us, vs = MO.momentum_predictor_lid_imex(u, v, nu, dx, dy, dt, U_LID, fu=fu, fv=fv,
                                                rho=RHO, cs2=cs2)
    else:
        us, vs = MO.momentum_predictor(u, v, nu, dx, dy, dt, U_LID, fu=fu, fv=fv, rho=RHO)
    un, vn, _ = MO.project(us, vs, dx, dy, dt, RHO, MO.poisson_eigs_neumann(n, n, dx, dy))
    if use_el:
        umc, vmc = midpoint_centres(u, v, un, vn)
        X1, X2 = O.extrapolate_reference_map(adv(X1, umc, vmc, phi) * sm, adv(X2, umc, vmc, phi) * sm,
                                             phi, dx, dy, NL)
    return dict(u=un, v=vn, X1=X1, X2=X2, J=J, phi=phi, sl=sl)


def map_noise(O, MO, s, integrator, dt, mu_s=0.1, scheme="semilagrangian", seed=0):
    """The reference step's own response to a one-ulp change of one face-force value (what the
    rounding of another implementation's force or CG amounts to; the step's inputs themselves
    are not touched, so at rest, u = v = 0, the probe still acts): the largest change of
    (u or v, X1 or X2) over NOISE_NUDGES nudges (alternating fu and fv, up and down, at seeded
    non-zero faces)."""
    base = step(O, MO, s, integrator, dt, mu_s, scheme)
    rng = np.random.default_rng(7000 + seed)
    wv = wm = 0.0
    for trial in range(NOISE_NUDGES):
        out = step(O, MO, s, integrator, dt, mu_s, scheme, nudge=(trial, rng))
        wv = max(wv, np.abs(out["u"] - base["u"]).max(), np.abs(out["v"] - base["v"]).max())
        wm = max(wm, np.abs(out["X1"] - base["X1"]).max(), np.abs(out["X2"] - base["X2"]).max())
    return base, wv, wm
