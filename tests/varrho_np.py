"""Case builders of the variable-density projection tests off the square
(tests/test_gpu_varrho_offsquare.py, tests/test_varrho_rect_cpu.py) and of their fixture's
generator (tests/golden/gen_varrho_rect.py): the grids, a density that varies along the walls,
the velocity and pressure planes, the key names of tests/golden/varrho_rect.npz, and the
recorded residual history of the oracle's CG.

Plain NumPy, no GPU.
"""
import functools

import numpy as np

from offsquare_np import sid, spacing  # noqa: F401  (re-exported)

# (ny, nx), spacing kind: the grids whose results the reference itself wrote into the fixture
FIXTURE_GRIDS = [((20, 47), "aniso"), ((131, 5), "aniso"), ((5, 131), "iso")]
# operator and divergence: the fixture's shapes, the stage-tile shapes and a transposed one
OP_SHAPES = [(20, 47), (131, 5), (5, 131), (37, 133), (133, 37), (69, 256), (36, 132)]
PROJ_SHAPES = [(37, 133), (133, 37), (69, 256)]
# the 263263 cells of this grid are one row and 118 cells more than the 262144 threads of
# k_vr_apply's grid (CG_BLOCKS * CG_T): the second grid-stride trip
STRIDE_SHAPE = (263, 1001)
CG_THREADS = 262144

# name -> (bc_kind of the C ABI, lid speed); the identity is passed as lambda u, v: (u, v)
BCS = {"freeslip": (2, 0.0), "lid": (1, 1.0), "identity": (0, 0.0)}
# (maxiter, previous pressure given): p_prev = None changes the rhs only, one cap is enough
RUNS = [(1, True), (2, True), (5, True), (2, False)]
MAXITERS = (1, 2, 5)
DT = 1e-3
RATIO = 4.0
BAR = 1e-10     # atol = BAR * max(|ref|.max(), 1): the bar of tests/test_gpu_varrho.py


def heaviside(x, w):
    """functions.py:660-671."""
    H = 0.5 * (1.0 + x * (1.0 / w) + (1.0 / np.pi) * np.sin(np.pi * x * (1.0 / w)))
    H = np.where(x > w, 1.0, H)
    return np.where(x < -w, 0.0, H)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Inputs of one grid, from default_rng(ny * 11 + nx): rho = the smoothed-Heaviside
    mixture (ratio 4) of a disc centred at (0.1 Lx, 0.85 Ly) with radius 0.3 min(Lx, Ly) and
    w = 2 max(dx, dy) -- it crosses the west wall and the lid -- times uniform(0.9, 1.1) per
    cell, so no two cells and no two faces share a coefficient; a*, b* = a Taylor-Green pair
    + 0.1 N(0, 1); p = N(0, 1) for the operator; p_prev = 0.1 N(0, 1).  Shared: never written."""
    ny, nx = shape
    dx, dy = spacing(shape, kind)
    rng = np.random.default_rng(ny * 11 + nx)
    X, Y = np.meshgrid(np.arange(nx) * dx, np.arange(ny) * dy)
    Lx, Ly = (nx - 1) * dx, (ny - 1) * dy
    phi = np.sqrt((X - 0.1 * Lx) ** 2 + (Y - 0.85 * Ly) ** 2) - 0.3 * min(Lx, Ly)
    H = heaviside(phi, 2.0 * max(dx, dy))
    rho = ((1 - H) * RATIO + H * 1.0) * rng.uniform(0.9, 1.1, (ny, nx))
    k = 2 * np.pi
    c = dict(dx=dx, dy=dy, dt=DT, rho=rho, p=rng.standard_normal((ny, nx)))
    c["a"] = 0.5 * np.sin(k * X) * np.cos(k * Y) + 0.1 * rng.standard_normal((ny, nx))
    c["b"] = -0.5 * np.cos(k * X) * np.sin(k * Y) + 0.1 * rng.standard_normal((ny, nx))
    c["p_prev"] = 0.1 * rng.standard_normal((ny, nx))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def check_density(rho, kind):
    """What the cases rest on: the density differs between every wall cell and its inward
    neighbour (the BC source cells of the free-slip box) and no two neighbouring faces carry
    the same coefficient; in the 1 x 0.7 box (aniso) the disc crosses the west wall and the
    lid, so the density varies along them by more than the rough factor's 0.2 * 4 could (with
    dx == dy a 5-wide grid is a sliver that the disc cannot span)."""
    assert (rho[0] != rho[1]).all() and (rho[-1] != rho[-2]).all()
    assert (rho[:, 0] != rho[:, 1]).all() and (rho[:, -1] != rho[:, -2]).all()
    if kind == "aniso":
        assert np.ptp(rho[:, 0]) > 1.0 and np.ptp(rho[-1]) > 1.0
    ir = 1.0 / rho
    fx, fy = 0.5 * (ir[:, :-1] + ir[:, 1:]), 0.5 * (ir[:-1] + ir[1:])
    assert (fx[:, :-1] != fx[:, 1:]).all() and (fy[:-1] != fy[1:]).all()


# ── keys of tests/golden/varrho_rect.npz ──────────────────────────────────────────
INPUTS = ("rho", "p", "a", "b", "p_prev")


def key(shape, name):
    return "g%s_%s" % (sid(shape), name)


def run_key(shape, maxiter, with_prev, name):
    """an / bn / pn: the three BCs stacked in the order of BCS; it: the callback count."""
    return key(shape, "m%d%s_%s" % (maxiter, "" if with_prev else "n", name))


def fixture_case(g, shape):
    """The fixture's inputs of one grid as a dict like case()'s, with eig, Ap and divU."""
    c = {k: g[key(shape, k)] for k in INPUTS + ("eig", "Ap", "divU")}
    c.update({k: float(g[key(shape, k)]) for k in ("dx", "dy", "dt")})
    return c


# ── the oracle's CG, watched ──────────────────────────────────────────────────────
def oracle_residuals(O, c, with_prev, n):
    """||r|| / ||b|| as the oracle's CG tests it at the top of iterations 0 .. n - 1 (rtol = 0:
    the test never passes, and the iterates do not depend on rtol)."""
    ny, nx = c["a"].shape
    eig = O._precompute_poisson_eigenvalues(nx, ny, c["dx"], c["dy"])
    seen = []
    solve = O._solve_poisson_dct

    def watched(r, e):
        seen.append(np.linalg.norm(r))
        return solve(r, e)
    O._solve_poisson_dct = watched
    try:
        O.pressure_projection_variable(c["a"], c["b"], c["dx"], c["dy"], c["dt"], c["rho"], 2,
                                       0.0, c["p_prev"] if with_prev else None, eig, rtol=0.0,
                                       maxiter=n)
    finally:
        O._solve_poisson_dct = solve
    return [s / seen[0] for s in seen]


def worst(got, ref, bar=BAR):
    """max |got - ref| over the bar's atol, the worst of the given (got, ref) pairs."""
    return max(float(np.abs(g - r).max()) / (bar * max(float(np.abs(r).max()), 1.0))
               for g, r in zip(got, ref))
