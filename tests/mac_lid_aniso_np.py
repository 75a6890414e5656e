"""Shared pieces of the dx != dy tests of the lid-tier MAC operators and the IMEX tier
(tests/test_mac_lid_aniso_cpu.py pins the oracle, tests/test_gpu_mac_lid_aniso.py the kernels):
the grids, the seeded inputs, the case tables with their bars, the one-ulp nudge that measures a
reference's own noise floor, and a residual-recording copy of the oracle's CG.

The grids are square in cells (the lid-tier kernels are square-only) on a non-square box:
dx, dy = mac_grid(N, N, Lx, Ly) with Lx != Ly.

Bars.  What is not bit-exact is held to 1e-12 of the solution's scale against the reference's
fixture and to 1e-11 against the oracle at other sizes.  A bar holds only where the reference's
own response to a one-ulp change of one input value (its noise floor) is at most a tenth of it;
where that response is larger, the case's bar is ten times the floor measured on the CPU and is
written next to the case below (NOISY).  No bar comes from a GPU result.
"""
import numpy as np

BOXES = {"tall": (1.0, 1.25), "wide": (2.0, 1.0)}    # (Lx, Ly): dx / dy = 0.8 and 2
FIXTURE_GRIDS = ((5, "tall"), (6, "wide"), (33, "tall"))
ORACLE_N = (64, 97)
# the projection's oracle sizes: the DCT-II solve takes N that factor into radices <= 23 and
# refuses the prime 97 (NotImplementedError, tests/test_gpu_dct2.py test_rejected_shapes), so
# the odd, non-power-of-two size of the projection is 99 = 9 * 11
PROJ_N = (64, 99)
NU, DT, RHO, GAMMA, U_LID, CS2 = 0.01, 2e-3, 1.3, 0.07, 1.0, 4.0
ETA, GSUM = 2.0, 0.6
COEFS = (2e-5, 0.5e-3, 0.05)
BAR_FIXTURE, BAR_ORACLE = 1e-12, 1e-11
BAR_PROJECT = 1e-12    # the projection, at every size (tests/test_gpu_mac.py test_mac_projection)


def spacing(N, box):
    Lx, Ly = BOXES[box]
    return Lx / N, Ly / N


def fixture(golden, N):
    """The arrays of one grid of tests/golden/mac_lid_aniso.npz, scalars as Python floats."""
    g = golden("mac_lid_aniso")
    d = {k[len(f"n{N}_"):]: g[k] for k in g.files if k.startswith(f"n{N}_")}
    return {k: (a.item() if a.ndim == 0 else a) for k, a in d.items()}


def discs(N, dx, dy):
    """Two overlapping discs that reach the bottom row and the left column (cell centres)."""
    Xc, Yc = np.meshgrid((np.arange(N) + 0.5) * dx, (np.arange(N) + 0.5) * dy)
    L = min(N * dx, N * dy)
    pa = np.sqrt((Xc - 0.30 * L) ** 2 + (Yc - 0.30 * L) ** 2) - 0.32 * L
    pb = np.sqrt((Xc - 0.36 * L) ** 2 + (Yc - 0.34 * L) ** 2) - 0.33 * L
    return pa, pb


def op_inputs(N, seed):
    """Seeded standard_normal fields of every staggering (the wall faces are not zeroed: the
    outputs' zeroing is under test)."""
    rng = np.random.default_rng(seed)
    u, fu = rng.standard_normal((2, N, N + 1))
    v, fv = rng.standard_normal((2, N + 1, N))
    kappa, H, p = rng.standard_normal((3, N, N))
    rhs_u = rng.standard_normal((N, N - 1))
    rhs_v = rng.standard_normal((N - 1, N))
    return dict(u=u, v=v, fu=fu, fv=fv, kappa=kappa, H=H, p=p, rhs_u=rhs_u, rhs_v=rhs_v)


def op_seed(N, box):
    """The seed of op_inputs at an oracle size."""
    return 5000 + 10 * N + list(BOXES).index(box)


def project_inputs(MO, N, box):
    """(u*, v*) for the projection at an oracle size: the oracle's explicit lid predictor of the
    seeded fields with forces (wall-normal faces 0, as the projection expects), at the box's
    own (dx, dy)."""
    dx, dy = spacing(N, box)
    d = op_inputs(N, op_seed(N, box))
    return MO.momentum_predictor(d["u"], d["v"], NU, dx, dy, DT, U_LID, fu=d["fu"], fv=d["fv"],
                                 rho=RHO)


def semilag_dt(u, v, dx, dy, cfl):
    """The dt at which the advective CFL of mac.py:387 is `cfl`."""
    return cfl / max(np.max(np.abs(u)) / dx, np.max(np.abs(v)) / dy)


def nudge(a, sign=1.0):
    """a with one interior element moved by one ulp."""
    b = np.array(a, dtype=np.float64, copy=True)
    j, i = b.shape[0] // 2, b.shape[1] // 2
    b[j, i] = np.nextafter(b[j, i], sign * np.inf)
    return b


def rel(a, b):
    """max|a - b| / max|b|."""
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def with_noise(fn, args, pos, kw=None):
    """fn(*args, **kw) as a tuple of arrays, and its response to a one-ulp change of args[pos]:
    max over the outputs of max|a - b| / max|a|."""
    kw = kw or {}
    a = fn(*args, **kw)
    b = fn(*(args[:pos] + (nudge(args[pos]),) + args[pos + 1:]), **kw)
    if isinstance(a, np.ndarray):
        a, b = (a,), (b,)
    a = tuple(x for x in a if isinstance(x, np.ndarray))
    b = tuple(x for x in b if isinstance(x, np.ndarray))
    return a, max(rel(y, x) for x, y in zip(a, b))


def cg_x0_rec(matvec, b, psolve, rtol, maxiter):
    """oracle.mac_oracle.cg_x0 with the stopping test's ||r|| / atol of every trip recorded:
    returns (x, iterations, ratios); ratios[k] is the value tested at the head of trip k, and
    the last entry is the one that stopped the loop (or, at maxiter, the residual left)."""
    x = b.copy()
    bnrm2 = np.linalg.norm(b)
    if bnrm2 == 0:
        return b.copy(), 0, []
    atol = rtol * bnrm2
    r = b - matvec(x) if x.any() else b.copy()
    rho_prev, p = None, None
    ratios = []
    for it in range(maxiter):
        ratios.append(np.linalg.norm(r) / atol)
        if np.linalg.norm(r) < atol:
            return x, it, ratios
        z = psolve(r)
        rho_cur = np.dot(r, z)
        if it > 0:
            beta = rho_cur / rho_prev
            p *= beta
            p += z
        else:
            p = np.empty_like(r)
            p[:] = z[:]
        q = matvec(p)
        alpha = rho_cur / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho_cur
    ratios.append(np.linalg.norm(r) / atol)
    return x, maxiter, ratios


def margin_ok(ratios, it, maxiter):
    """An equal iteration count is a fair demand only where rounding does not decide the
    stopping test: ||r|| / atol >= 1.05 on every trip that runs (the last one decides) and
    <= 0.95 where the loop stops.  A loop that ends at maxiter has no stopping value."""
    ran = ratios[:it]
    if ran and min(ran) < 1.05:
        return False
    return it == maxiter or ratios[it] <= 0.95


class Recorded:
    """Context manager: the oracle's cg_x0 replaced by cg_x0_rec, every solve's
    (iterations, ratios, maxiter) kept in .solves."""

    def __init__(self, MO):
        self.MO, self.solves = MO, []

    def __enter__(self):
        self.orig = self.MO.cg_x0

        def rec(matvec, b, psolve, rtol, maxiter):
            x, it, ratios = cg_x0_rec(matvec, b, psolve, rtol, maxiter)
            self.solves.append((it, ratios, maxiter))
            return x, it
        self.MO.cg_x0 = rec
        return self

    def __exit__(self, *a):
        self.MO.cg_x0 = self.orig

    def all_ok(self):
        return all(margin_ok(r, it, mx) for it, r, mx in self.solves)


# ---------------------------------------------------------------- Helmholtz cases ----
# (N, box, coef, kind, precond) -> seed of the right-hand side.  CG runs at the reference's
# default rtol 1e-10, PCG at 1e-8 (mac.py:263, 287).  A seed whose oracle residual history
# violates margin_ok is replaced (SEED_OVERRIDE), the case stays.
HELM_N = (5, 6, 33, 64, 97)
RTOL = {0: 1e-10, 1: 1e-8}     # by precond


def helm_cases():
    out = []
    for N in HELM_N:
        for box in BOXES:
            for coef in COEFS:
                for kind in (0, 1):
                    for precond in (0, 1):
                        out.append((N, box, coef, kind, precond))
    return out


HELM_BIG = [(516, "tall", 0.5e-3, kind, 1) for kind in (0, 1)]
# (the formula's seed: its ||r|| / atol on the last trip that ran and where it stopped)
SEED_OVERRIDE = {
    (33, "tall", 0.05, 0, 1): 3302008,     # 3302001: 1.050, 0.122
    (33, "wide", 0.05, 0, 0): 3302107,     # 3302100: 1.006, 0.697
    (64, "tall", 0.0005, 1, 1): 6401025,   # 6401011: 1.004, 0.072
    (64, "tall", 0.05, 1, 0): 6402031,     # 6402010: 1.078, 0.980
    (64, "wide", 0.05, 0, 0): 6402121,     # 6402100: 1.002, 0.847
    (97, "tall", 0.05, 0, 0): 9702189,     # 9702000: 1.000, 0.948
    (97, "tall", 0.05, 1, 0): 9702073,     # 9702010: 1.079, 0.998
    (97, "wide", 0.0005, 0, 0): 9701114,   # 9701100: 1.050, 0.688
    (97, "wide", 0.0005, 1, 0): 9701152,   # 9701110: 1.025, 0.676
    (97, "wide", 0.05, 0, 0): 9702107,     # 9702100: 1.077, 0.985
    (97, "wide", 0.05, 1, 0): 9702460,     # 9702110: 1.007, 0.938
}
# bars above BAR_ORACLE: ten times the oracle's one-ulp response measured on the CPU (none: the
# largest response of the cases below is 6.7e-14, N = 97, tall, coef 0.05, v, CG; 6.2e-14 at
# N = 516)
NOISY = {}


def helm_seed(case):
    N, box, coef, kind, precond = case
    base = 100000 * N + 1000 * COEFS.index(coef) + 100 * list(BOXES).index(box) + 10 * kind + precond
    return SEED_OVERRIDE.get(case, base)


def helm_rhs(case):
    N, _, _, kind, _ = case
    shp = (N, N - 1) if kind == 0 else (N - 1, N)
    return np.random.default_rng(helm_seed(case)).standard_normal(shp)


def helm_bar(case):
    return NOISY.get(case, BAR_ORACLE)


def helm_id(case):
    N, box, coef, kind, precond = case
    return f"N{N}-{box}-coef{coef:g}-{'uv'[kind]}-{'pcg' if precond else 'cg'}"


# ---------------------------------------------------------------- predictor cases ----
# (N, box, variant) at the oracle sizes; variant: plain, forces (fu, fv, rho, cs2), fu, fv
PRED_VARIANTS = ("plain", "forces", "fu", "fv")
PRED_SEED_OVERRIDE = {}
PRED_NOISY = {}


def pred_cases():
    return [(N, box, var) for N in ORACLE_N for box in BOXES for var in PRED_VARIANTS]


def pred_inputs(case, which):
    """(u, v, kwargs) of one predictor case; which: 'imex' or 'semilag' (seeds differ)."""
    N, box, var = case
    base = 7000 + 10 * N + 3 * list(BOXES).index(box) + PRED_VARIANTS.index(var) + \
        (500 if which == "semilag" else 0)
    rng = np.random.default_rng(PRED_SEED_OVERRIDE.get((which,) + case, base))
    u, fu = rng.standard_normal((2, N, N + 1))
    v, fv = rng.standard_normal((2, N + 1, N))
    kw = {"plain": {}, "forces": dict(fu=fu, fv=fv, rho=RHO, cs2=CS2),
          "fu": dict(fu=fu, rho=RHO), "fv": dict(fv=fv, rho=RHO)}[var]
    return u, v, kw


def pred_bar(which, case):
    return PRED_NOISY.get((which,) + case, BAR_ORACLE)


def pred_id(case):
    return f"N{case[0]}-{case[1]}-{case[2]}"


def semilag_cases():
    """(N, box, variant, cfl): the semi-Lagrangian branch at CFL 4 in every variant, and the
    branch below cfl_switch (CFL 0.5: the IMEX predictor, bit for bit) plain and forced."""
    return [(N, box, var, cfl) for N in ORACLE_N for box in BOXES
            for var, cfl in (("plain", 4.0), ("forces", 4.0), ("fu", 4.0), ("fv", 4.0),
                             ("plain", 0.5), ("forces", 0.5))]


def semilag_inputs(case):
    """(args, kwargs) of momentum_predictor_lid_semilag for one case."""
    N, box, var, cfl = case
    dx, dy = spacing(N, box)
    u, v, kw = pred_inputs((N, box, var), "semilag")
    return (u, v, NU, dx, dy, semilag_dt(u, v, dx, dy, cfl), U_LID), kw


def imex_inputs(case):
    N, box, _ = case
    dx, dy = spacing(N, box)
    u, v, kw = pred_inputs(case, "imex")
    return (u, v, NU, dx, dy, DT, U_LID), kw


# ---------------------------------------------------------------- plan cache, early exits ----
CACHE_COEF_A, CACHE_COEF_B = 0.5e-3, 0.05


def cache_sequence(kind):
    """The calls that walk imex_plan's paths: (N, dx, dy, coef, rhs, same_bits_as) with
    same_bits_as the index of an earlier step whose result must come back bit for bit, or None.
    The plans live on the context of their N, so the N = 33 steps share one plan and N = 34
    builds its own in between."""
    dx, dy = spacing(33, "wide")
    dx34, dy34 = spacing(34, "wide")
    rng = np.random.default_rng(4100 + kind)
    r33 = rng.standard_normal((33, 32) if kind == 0 else (32, 33))
    r34 = rng.standard_normal((34, 33) if kind == 0 else (33, 34))
    a, b = CACHE_COEF_A, CACHE_COEF_B
    return [(33, dx, dy, a, r33, None),      # cold
            (33, dx, dy, a, r33, 0),         # exact hit
            (33, dx, dy, b, r33, None),      # keep: same shape, new coef
            (33, dy, dx, b, r33, None),      # keep: the spacings exchanged
            (34, dx34, dy34, b, r34, None),  # another shape: a plan built from nothing
            (33, dx, dy, a, r33, 0)]         # back to step 0's (dx, dy, coef): keep once more


EXIT_N, EXIT_BOX, EXIT_COEF = 33, "wide", 0.05


def exit_rhs(kind):
    shp = (EXIT_N, EXIT_N - 1) if kind == 0 else (EXIT_N - 1, EXIT_N)
    return np.random.default_rng(4200 + kind).standard_normal(shp)
