"""Position sets, exact-arithmetic inputs and NumPy references of the reduction tests
(test_gpu_reductions.py on the device, test_reductions_cpu.py for this file itself).

A reduction over n items on B workgroups of T threads gives item k to thread k mod (T * B) on
trip k div (T * B).  `positions` lists the items at which that mapping can go wrong: both ends,
the wave and workgroup edges, the last item of the first trip and the first of the second, the
ends of the plane's rows and a seeded handful in between.  A test changes one item at each of
them and compares the result with the reference's for that field.

The sums are made exact, so that `==` holds whatever the fold order: every term is a small
integer times a power of two (velocities integer / 4, dx and dy powers of two, densities and
viscosities powers of two), every partial sum is exact in binary64, and the expected value comes
from Python integers through `fractions.Fraction`.  Such a test fails on a dropped, doubled or
misplaced item and on nothing else.
"""
from fractions import Fraction

import numpy as np

# first-pass launch shapes (threads T, workgroups B) of the reductions under test
RED = (256, 1024)        # k_reduce_p1 / p2 (compute_timestep, two_solid_diag), k_all_finite2
EPOCH = (256, 256)       # k_mac_epoch_p1
SOFT = (256, 128)        # k_mac_soft_diag_p1
CFL = (256, 512)         # k_macpsl_absmax (at most SLR_BLOCKS workgroups)
NPSUM = (128, 64)        # k_np_pairwise: leaves of 128 items, 64 of them an 8192-item chunk
LAUNCHES = dict(RED=RED, EPOCH=EPOCH, SOFT=SOFT, CFL=CFL, NPSUM=NPSUM)

DX, DY = 2.0 ** -7, 2.0 ** -6


def positions(shape, T, B, seed=0):
    """K(n, T, B) of a (rows, cols) plane flattened in C order, clipped to [0, n), sorted."""
    rows, cols = shape
    n = rows * cols
    K = {0, 1, 63, 64, T - 1, T, T * B - 1, T * B, T * B + 1, n - 2, n - 1,
         (rows - 1) * cols, n - 1, cols - 1}
    rng = np.random.default_rng([seed, rows, cols, T, B])
    K |= {int(k) for k in rng.integers(0, n, 16)}
    return sorted(k for k in K if 0 <= k < n)


def last_column(shape):
    rows, cols = shape
    return [j * cols + cols - 1 for j in range(rows)]


def last_row(shape):
    rows, cols = shape
    return [(rows - 1) * cols + i for i in range(cols)]


def exact_float(q):
    """The binary64 that is exactly the Fraction q (asserted)."""
    x = float(q)
    assert Fraction(x) == q, q
    return x


# ── velocities on the quarter lattice ────────────────────────────────────────────
def quarter_ints(shape, seed, lim=8):
    """Two integer planes in -lim .. lim; the velocities are these / 4."""
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    return rng.integers(-lim, lim + 1, shape), rng.integers(-lim, lim + 1, shape)


def quarter_field(shape, seed, lim=8):
    a4, b4 = quarter_ints(shape, seed, lim)
    return a4 / 4.0, b4 / 4.0


# ── energies (output.py:6-39, :136-193) with phi = 1 everywhere, so H = 1 ─────────
KE_RHO_F, KE_RHO_S = 2.0, 8.0
ED_MU_F, ED_ETA_S = 0.5, 4.0
ENERGY_W_T = 0.25     # phi = 1 > w_t: the smoothed Heaviside is exactly 1
ENERGY_SHAPES = ((5, 5), (8, 16), (64, 128), (7, 1171), (82, 100), (128, 128), (130, 129))


def _dot(x, y):
    """sum(x * y) of two small-integer planes as a Python integer (int64 holds it exactly)."""
    return int(np.sum(np.asarray(x, dtype=np.int64) * np.asarray(y, dtype=np.int64)))


def ke_exact(a4, b4, rho_f=KE_RHO_F, dx=DX, dy=DY):
    """sum(0.5 rho_f (a^2 + b^2)) dx dy for a = a4 / 4, b = b4 / 4 in exact arithmetic."""
    s = _dot(a4, a4) + _dot(b4, b4)
    return exact_float(Fraction(s, 16) * Fraction(rho_f) / 2 * Fraction(dx) * Fraction(dy))


def _grad_int(f, axis):
    """2 h times utils.py's second-order gradient of an integer plane: central in the
    interior, -3 f0 + 4 f1 - f2 (and its mirror) at the two edges."""
    f = np.moveaxis(np.asarray(f, dtype=np.int64), axis, -1)
    g = np.empty_like(f)
    g[..., 1:-1] = f[..., 2:] - f[..., :-2]
    g[..., 0] = -3 * f[..., 0] + 4 * f[..., 1] - f[..., 2]
    g[..., -1] = 3 * f[..., -1] - 4 * f[..., -2] + f[..., -3]
    return np.moveaxis(g, -1, axis)


def dissipation_exact(a4, b4, mu_f=ED_MU_F, dx=DX, dy=DY):
    """sum(2 mu_f (D_xx^2 + D_yy^2 + 2 D_xy^2)) dx dy for a = a4 / 4, b = b4 / 4."""
    hx, hy = Fraction(1, 8) / Fraction(dx), Fraction(1, 8) / Fraction(dy)   # (1/4) / (2 h)
    ax, ay, bx, by = _grad_int(a4, 1), _grad_int(a4, 0), _grad_int(b4, 1), _grad_int(b4, 0)
    s = _dot(ax, ax) * hx * hx + _dot(by, by) * hy * hy
    # D_xy = (ay hy + bx hx) / 2
    p, q = hy / 2, hx / 2
    s += 2 * (p * p * _dot(ay, ay) + q * q * _dot(bx, bx) + 2 * p * q * _dot(ay, bx))
    return exact_float(2 * Fraction(mu_f) * s * Fraction(dx) * Fraction(dy))


def disc_energy_inputs(shape):
    """Smooth fields and a disc on a (ny, nx) node grid, for the bars of test_energy_exports:
    the strain energy bit for bit, KE and dissipation through the smoothed Heaviside."""
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    X, Y = np.meshgrid(np.arange(nx) * dx, np.arange(ny) * dy)
    phi = np.sqrt((X - 0.45) ** 2 + (Y - 0.55) ** 2) - 0.3
    X1 = X + 0.03 * np.sin(3 * Y); X2 = Y - 0.02 * np.cos(2 * X)
    a = np.sin(2 * np.pi * X) * np.cos(np.pi * Y); b = -np.cos(np.pi * X) * np.sin(2 * np.pi * Y)
    return dict(dx=dx, dy=dy, phi=phi, X1=X1, X2=X2, a=a, b=b, w_t=2 * dx)


# ── compute_timestep (functions.py:165-192) ──────────────────────────────────────
TS_SHAPES = ((5, 7), (512, 512), (513, 513))
TS_SPIKE = 5.0
# c_s = 2: the solid bound 0.1 dx lies between the fluid bound of the base field (|u| <= 0.71:
# above 0.28 dx) and that of the spiked field (0.04 dx); no surface tension, no viscosity, so
# the other bounds are 1.0
TS_PAR = dict(dx=DX, dy=DY, CFL=0.2, dt_min_cap=1.0, mu_s=3.0, rho_s=1.0, gamma=0.0, rho_f=1.0,
              mu_f=0.0, eta_s=0.0, kappa=0.0)
# c_s = 0.1: the fluid bound binds on the base field itself, so a result that carries a fluid
# bound from the finite speeds differs from one without it
TS_PAR_SLOW = dict(TS_PAR, mu_s=0.0075)


def ts_base(shape):
    """|a|, |b| <= 1/2."""
    return quarter_field(shape, 11, lim=2)


# ── epoch distortion (mac_reinit_test.py:91-94) ──────────────────────────────────
EPOCH_SHAPES = ((9, 12), (256, 256), (257, 257))


def epoch_distortion(J, phi):
    m = phi <= 0
    if not m.any():
        return np.array([-np.inf, np.inf, 0.0])
    return np.array([J[m].max(), J[m].min(), float(m.sum())])


# ── soft-disc diagnostics (mac_soft_disc_lid.py:139-150) ─────────────────────────
SOFT_SHAPES = ((9, 12), (128, 256), (182, 185))


def centre_sums(cells, nx, dx=DX, dy=DY):
    """(count, sum Xc, sum Yc) over the flat cell indices `cells`, exact."""
    sx = sum(Fraction(2 * (k % nx) + 1, 2) for k in cells) * Fraction(dx)
    sy = sum(Fraction(2 * (k // nx) + 1, 2) for k in cells) * Fraction(dy)
    return float(len(cells)), exact_float(sx), exact_float(sy)


# ── the periodic CFL switch (mac.py:625-626) ─────────────────────────────────────
CFL_SHAPES = ((5, 7), (256, 512), (256, 513))
CFL_DX, CFL_DY = 2.0 ** -7, 2.0 ** -5
CFL_DT, CFL_SWITCH = 2.0 ** -4, 0.9
CFL_BASE = 2.0 ** -12          # |u|, |v| of the base field: CFL = dt * base / dx = 2^-9
# dy = 4 dx, so the divisors tell apart.  A u face of 2 dx / dt = 0.25 is CFL 2 through dx and
# would be CFL 0.5 (no switch) through dy.  A v face of 2 dy / dt = 1.0 is CFL 2 through dy;
# and a v face of 0.5 dy / dt = 0.25 is CFL 0.5 through dy (no switch) and would be CFL 2
# through dx.  Only the correct divisor gives each expected branch.
CFL_U_SPIKE, CFL_V_SPIKE, CFL_V_BELOW = 0.25, 1.0, 0.25


def cfl_took_sl(u, v, dx=CFL_DX, dy=CFL_DY, dt=CFL_DT, switch=CFL_SWITCH):
    """mac.py:625-626 as written: Python's max keeps its first operand unless the second
    compares greater, so a NaN in u makes cfl NaN (`cfl <= switch` is False: the SL branch)
    and a NaN in v is dropped."""
    with np.errstate(invalid="ignore"):
        cfl = dt * max(np.max(np.abs(u)) / dx, np.max(np.abs(v)) / dy)
        return not cfl <= switch


# ── two-solid record (two_disc_contact.py:98-104, common.py:110-115) ─────────────
TWO_SHAPES = ((9, 12), (513, 513))


def two_solid_diag(phi_a, phi_b, X, Y, Jmin):
    def centroid(phi):
        m = phi <= 0.0
        return (X[m].mean(), Y[m].mean()) if np.any(m) else (np.nan, np.nan)
    (xa, ya), (xb, yb) = centroid(phi_a), centroid(phi_b)
    return np.array([xa, ya, xb, yb, Jmin.min()])
