"""Every item reaches the result of every standalone reduction, and a NaN does what it does in
the reference.

The per-cell operators are pinned at tile edges and odd sizes; this file does the same for the
reductions.  Each one is run on three shapes -- tiny, n = T * B exactly (every first-pass thread
one item) and the smallest convenient n > T * B (the grid-stride loop's second trip) -- and a
single item is changed at each position of reductions_np.positions: the ends, the wave and
workgroup edges, T * B - 1, T * B, T * B + 1, the row ends and a seeded handful.  The planes
stay on the device and one element is rewritten per call.

Comparisons are `==` (isnan where the reference gives NaN).  Maxima and minima are exact in any
fold order; the sums are built from small integers times powers of two, so every partial sum is
exact and the expected value comes from Python integers (reductions_np.py, checked against the
oracle by test_reductions_cpu.py).  The only tolerances are test_energy_exports' own: the
strain energy bit for bit against the oracle, and 1e-14 relative on the kinetic energy and the
dissipation where the smoothed Heaviside (device sin against glibc's) is in the density.

Covered: rmt_compute_timestep (k_reduce_p1<3> / k_reduce_p2<3>), the fused step's first dt
(reduce_maxsq2_nan on the product path), rmt_all_finite2 through advect_reference_map, np_sum's
size classes through the three energies, rmt_mac_epoch_distortion, rmt_mac_soft_diag (cell and
face planes), the CFL switch of the periodic semi-Lagrangian predictor and rmt_two_solid_diag.

Out of scope here: the CG dots (their iteration counts are pinned against the oracle), the row
tree of the pressure mean (held at 1e-13 by the DCT solve tests at many ny), the fused loops'
own diagnostics (k_diag_p1 / p2, k_mac_diag) and the slab paths.
"""
import ctypes

import numpy as np
import pytest

import mac_soft_disc_np as SNP
import reductions_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(gpu):
    from pyrmt_amd import functions
    return functions


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


class Poke:
    """One element of a device plane (and of its host copy) changed inside a `with`."""

    def __init__(self, t, h, k, value):
        self.t, self.h, self.k, self.value = t.view(-1), h.reshape(-1), k, value

    def __enter__(self):
        self.old = self.h[self.k]
        self.h[self.k] = self.value
        self.t[self.k] = self.value

    def __exit__(self, *exc):
        self.h[self.k] = self.old
        self.t[self.k] = float(self.old)


def same(got, want, what):
    """== for finite values, isnan where the reference gives NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=str(what))   # (NaN matches NaN only)


# ── 1. compute_timestep ───────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def ts_fields():
    out = {}
    for shape in R.TS_SHAPES:
        a, b = R.ts_base(shape)
        out[shape] = (a, b, dev(a), dev(b))
    return out


@pytest.mark.parametrize("shape", R.TS_SHAPES)
def test_compute_timestep_single_spike(F, oracle, ts_fields, shape):
    a, b, ad, bd = ts_fields[shape]
    base = oracle.compute_timestep(a, b, **R.TS_PAR)
    assert F.compute_timestep(ad, bd, **R.TS_PAR) == base
    for h, t in ((a, ad), (b, bd)):
        for k in R.positions(shape, *R.RED):
            for spike in (R.TS_SPIKE, -R.TS_SPIKE):
                with Poke(t, h, k, spike):
                    want = oracle.compute_timestep(a, b, **R.TS_PAR)
                    assert want < base                       # the fluid bound binds
                    got = F.compute_timestep(ad, bd, **R.TS_PAR)
                assert got == want, (shape, k, spike, got, want)


@pytest.mark.parametrize("shape", R.TS_SHAPES)
def test_compute_timestep_nonfinite(F, oracle, ts_fields, shape):
    """functions.py:172 takes np.max of the speeds, which is NaN when one of them is; Python's
    min then skips that bound (a NaN never compares smaller), so the result is the smallest of
    the other bounds, not a fluid bound from the finite speeds.  An infinite speed gives 0."""
    a, b, ad, bd = ts_fields[shape]
    zero = np.zeros(shape)
    slow = oracle.compute_timestep(a, b, **R.TS_PAR_SLOW)
    others = oracle.compute_timestep(zero, zero, **R.TS_PAR_SLOW)
    assert slow < others                                     # the fluid bound binds when finite
    assert F.compute_timestep(ad, bd, **R.TS_PAR_SLOW) == slow
    for h, t in ((a, ad), (b, bd)):
        for k in R.positions(shape, *R.RED):
            with Poke(t, h, k, np.nan):
                with np.errstate(invalid="ignore"):
                    want = oracle.compute_timestep(a, b, **R.TS_PAR_SLOW)
                assert want == others
                got = F.compute_timestep(ad, bd, **R.TS_PAR_SLOW)
            assert got == want, (shape, k, "nan", got, want)
            for inf in (np.inf, -np.inf):
                with Poke(t, h, k, inf):
                    assert oracle.compute_timestep(a, b, **R.TS_PAR_SLOW) == 0.0
                    got = F.compute_timestep(ad, bd, **R.TS_PAR_SLOW)
                assert got == 0.0, (shape, k, inf, got)
    # a NaN and, elsewhere, a faster finite cell: still no fluid bound
    n = a.size
    with Poke(ad, a, n - 1, np.nan), Poke(bd, b, 0, R.TS_SPIKE):
        assert F.compute_timestep(ad, bd, **R.TS_PAR_SLOW) == others


@pytest.mark.parametrize("shape", R.TS_SHAPES)
def test_compute_timestep_negative_zero(F, oracle, shape):
    z = -0.0 * np.ones(shape)
    assert np.signbit(z).all()
    for par in (R.TS_PAR, R.TS_PAR_SLOW):
        assert F.compute_timestep(dev(z), dev(z), **par) == oracle.compute_timestep(z, z, **par)


# ── 2. the fused loop's first-step dt ─────────────────────────────────────────────
def test_fused_step_first_dt(gpu, oracle):
    """reduce_maxsq2_nan on the product path: Simulation.step after set_field computes dt from
    the fields as they are.  A face speed of 64 makes the fluid bound bind at N = 513 (the
    viscous bound, 0.2 dx^2 / 0.04, is the smallest of the others)."""
    from pyrmt_amd.simulation import soft_disc_in_lid_driven
    N = 513
    sim = soft_disc_in_lid_driven(N)
    P = sim.params
    par = dict(dx=sim.dx, dy=sim.dy, CFL=P.cfl, dt_min_cap=P.dt_cap, mu_s=P.mu_s, rho_s=P.rho_s,
               gamma=0.0, rho_f=P.rho_f, mu_f=P.mu_f, eta_s=P.eta_s, kappa=P.kappa)
    zero = np.zeros((N, N))
    others = oracle.compute_timestep(zero, zero, **par)
    T, B = R.RED
    n = N * N
    for step, k in enumerate((0, T - 1, T * B - 1, T * B, T * B + 1, n - 1)):
        u = zero.copy(); u.ravel()[k] = 64.0
        want = oracle.compute_timestep(u, zero, **par)
        assert want < others and want == P.cfl * sim.dx / (64.0 + 1e-6)
        sim.set_field("u", u); sim.set_field("v", zero)
        sim.step(1)
        dt = sim.diagnostics()["dt"]
        assert len(dt) == step + 1
        assert dt[step] == want, (k, dt[step], want)


# ── 3. all_finite2 through advect_reference_map ───────────────────────────────────
@pytest.mark.parametrize("shape", [(5, 7), (513, 513)])
def test_advect_reference_map_guard(F, ts_fields, shape):
    ny, nx = shape
    a, b, ad, bd = ts_fields[shape]
    X, Y, dx, dy = F.create_grid(nx, ny, 1.0, 1.0)
    Xd, Yd = dev(X), dev(Y)
    phi = dev(np.ones(shape))
    args = (Xd, ad, bd, Xd, Yd, 1e-3, dx, dy, phi)
    out = F.advect_reference_map(*args)                      # the finite field: no error
    assert out.shape == Xd.shape and bool(out.isfinite().all())
    for h, t in ((a, ad), (b, bd)):
        for k in R.positions(shape, *R.RED):
            for bad in (np.nan, np.inf, -np.inf):
                with Poke(t, h, k, bad):
                    with pytest.raises(FloatingPointError):
                        F.advect_reference_map(*args)
    F.advect_reference_map(*args)                            # restored: no error again


# ── 4. the energies: np_sum's size classes ────────────────────────────────────────
@pytest.mark.parametrize("shape", R.ENERGY_SHAPES)
def test_energies_exact(F, shape):
    """n = 25 and 128 (one leaf of np_pairwise_serial, with and without a tail), 8192 (one full
    chunk on the wave), 8197 and 8200 (a partial chunk of 5: the n < 8 branch; of 8: the
    unrolled branch with neither loop nor tail), 16384 (two full chunks, no partial one) and
    16770 (a partial chunk of 386: the recursion)."""
    a4, b4 = R.quarter_ints(shape, 3)
    ad, bd, phi = dev(a4 / 4.0), dev(b4 / 4.0), dev(np.ones(shape))
    ke = F.compute_kinetic_energy(ad, bd, R.KE_RHO_F, R.KE_RHO_S, phi, R.ENERGY_W_T, R.DX, R.DY)
    assert ke == R.ke_exact(a4, b4), (shape, ke, R.ke_exact(a4, b4))
    ed = F.compute_viscous_dissipation(ad, bd, R.ED_MU_F, phi, R.ENERGY_W_T, R.DX, R.DY, R.ED_ETA_S)
    assert ed == R.dissipation_exact(a4, b4), (shape, ed, R.dissipation_exact(a4, b4))


@pytest.mark.parametrize("shape", [(7, 1171), (82, 100), (130, 129)])
def test_kinetic_energy_single_spike(F, shape):
    """(7, 1171) as well: its positions 8192, n - 2 and n - 1 lie in the five-item chunk."""
    a4, b4 = R.quarter_ints(shape, 3)
    a = a4 / 4.0
    ad, bd, phi = dev(a), dev(b4 / 4.0), dev(np.ones(shape))
    for k in R.positions(shape, *R.NPSUM):
        old = a4.ravel()[k]
        a4.ravel()[k] = 31                                   # 7.75, outside the base range
        with Poke(ad, a, k, 7.75):
            ke = F.compute_kinetic_energy(ad, bd, R.KE_RHO_F, R.KE_RHO_S, phi, R.ENERGY_W_T,
                                          R.DX, R.DY)
        want = R.ke_exact(a4, b4)
        a4.ravel()[k] = old
        assert ke == want, (shape, k, ke, want)


@pytest.mark.parametrize("shape", R.ENERGY_SHAPES)
def test_energies_vs_oracle_with_a_disc(F, oracle, shape):
    g = R.disc_energy_inputs(shape)
    dx, dy, w_t = g["dx"], g["dy"], g["w_t"]
    assert (g["phi"] <= 0).any() and (g["phi"] > 0).any()
    se = F.compute_strain_energy(g["X1"], g["X2"], g["phi"], 0.3, dx, dy, 0.1)
    want = oracle.compute_strain_energy(g["X1"], g["X2"], g["phi"], 0.3, dx, dy, kappa=0.1)
    print(f"{shape}: strain energy {se!r} (oracle {want!r})")
    assert se == want and se != 0
    ke = F.compute_kinetic_energy(g["a"], g["b"], 1.0, 2.0, g["phi"], w_t, dx, dy)
    ed = F.compute_viscous_dissipation(g["a"], g["b"], 0.01, g["phi"], w_t, dx, dy, 0.05)
    kw = oracle.compute_kinetic_energy(g["a"], g["b"], 1.0, 2.0, g["phi"], w_t, dx, dy)
    ew = oracle.compute_viscous_dissipation(g["a"], g["b"], 0.01, g["phi"], w_t, dx, dy, 0.05)
    print(f"{shape}: KE rel {abs(ke - kw) / kw:.3g}, dissipation rel {abs(ed - ew) / ew:.3g} "
          "(bar 1e-14)")
    np.testing.assert_allclose(ke, kw, rtol=1e-14)
    np.testing.assert_allclose(ed, ew, rtol=1e-14)


# ── 5. epoch_distortion ───────────────────────────────────────────────────────────
@pytest.mark.parametrize("shape", R.EPOCH_SHAPES)
def test_epoch_distortion_single_cell(M, shape):
    J = np.full(shape, 2.0); phi = np.ones(shape)
    Jd, pd = dev(J), dev(phi)
    same(M.epoch_distortion(Jd, pd).cpu(), [-np.inf, np.inf, 0.0], shape)
    n = J.size
    for k in R.positions(shape, *R.EPOCH):
        with Poke(pd, phi, k, -1.0), Poke(Jd, J, k, 7.0):
            one = M.epoch_distortion(Jd, pd)
            with Poke(pd, phi, 0, 0.0):                      # and cell 0, whose J is 2 (or 7)
                two = M.epoch_distortion(Jd, pd)
                want2 = R.epoch_distortion(J, phi)
        same(one.cpu(), [7.0, 7.0, 1.0], (shape, k))
        same(two.cpu(), want2, (shape, k))
        assert tuple(want2) == ((7.0, 7.0, 1.0) if k == 0 else (7.0, 2.0, 2.0))
        # a NaN in a solid cell reaches both extremes and leaves the count; elsewhere it is ignored
        other = 0 if k else n - 1
        with Poke(pd, phi, other, 0.0):
            with Poke(pd, phi, k, -1.0), Poke(Jd, J, k, np.nan):
                solid = M.epoch_distortion(Jd, pd)
            with Poke(Jd, J, k, np.nan):
                fluid = M.epoch_distortion(Jd, pd)
        same(solid.cpu(), [np.nan, np.nan, 2.0], (shape, k, "NaN in a solid cell"))
        same(fluid.cpu(), [2.0, 2.0, 1.0], (shape, k, "NaN in a fluid cell"))


# ── 6. soft_diag ──────────────────────────────────────────────────────────────────
class SoftPlanes:
    def __init__(self, shape):
        ny, nx = shape
        self.shape = shape
        self.phi = np.ones(shape); self.J = np.ones(shape)
        self.u = np.zeros((ny, nx + 1)); self.v = np.zeros((ny + 1, nx))
        self.d = [dev(x) for x in (self.phi, self.J, self.u, self.v)]

    def run(self, M):
        return M.soft_diag(*self.d, R.DX, R.DY)

    def want(self):
        with np.errstate(invalid="ignore"):
            return SNP.soft_diag(self.phi, self.J, self.u, self.v, R.DX, R.DY)


@pytest.mark.parametrize("shape", R.SOFT_SHAPES)
def test_soft_diag_cells(M, shape):
    ny, nx = shape
    S = SoftPlanes(shape)
    pd, Jd = S.d[0], S.d[1]
    same(S.run(M).cpu(), [0, 0, 0, 1, 1, 0, 0, 0], shape)
    K = R.positions(shape, *R.SOFT)
    for k in K:
        with Poke(pd, S.phi, k, -1.0):
            got = S.run(M)
        i, j = k % nx, k // nx
        want = [1.0, (i + 0.5) * R.DX, (j + 0.5) * R.DY, 1, 1, 0, 0, 0]
        assert want[:3] == list(R.centre_sums([k], nx))
        same(got.cpu(), want, (shape, k))
        # the extremes of J are over all cells, not only the solid ones (there is none here)
        with Poke(Jd, S.J, k, 0.25):
            lo = S.run(M)
        with Poke(Jd, S.J, k, 7.0):
            hi = S.run(M)
        with Poke(Jd, S.J, k, np.nan):
            nan = S.run(M)
        same(lo.cpu(), [0, 0, 0, 0.25, 1, 0, 0, 0], (shape, k))
        same(hi.cpu(), [0, 0, 0, 1, 7, 0, 0, 0], (shape, k))
        same(nan.cpu(), [0, 0, 0, np.nan, np.nan, 0, 0, 0], (shape, k))
    # many solid cells at once: the positions and a block across the middle rows
    cells = set(K)
    for j in range(ny // 2 - 2, ny // 2 + 2):
        cells |= {j * nx + i for i in range(1, nx - 1)}
    cells = sorted(cells)
    S.phi.ravel()[cells] = -0.5
    S.d[0] = dev(S.phi)
    want = list(R.centre_sums(cells, nx)) + [1, 1, 0, 0, 0]
    same(S.run(M).cpu(), want, (shape, "block"))
    same(S.want(), want, (shape, "block, the NumPy restatement"))


@pytest.mark.parametrize("shape", R.SOFT_SHAPES)
def test_soft_diag_faces(M, shape):
    """The face planes have more items than there are cells: ny (nx + 1) and (ny + 1) nx, each
    with its own positions, and the last face column / row swept whole."""
    ny, nx = shape
    S = SoftPlanes(shape)
    for name, h, t, slot, extra in (("u", S.u, S.d[2], 5, R.last_column(S.u.shape)),
                                    ("v", S.v, S.d[3], 6, R.last_row(S.v.shape))):
        assert h.size > ny * nx
        K = sorted(set(R.positions(h.shape, *R.SOFT)) | set(extra))
        assert K[-1] == h.size - 1
        for k in K:
            with Poke(t, h, k, -3.0):
                got = S.run(M)
            want = [0, 0, 0, 1, 1, 0, 0, 0]; want[slot] = 3.0
            same(got.cpu(), want, (shape, name, k))
        for k in R.positions(h.shape, *R.SOFT):
            for bad in (np.nan, np.inf, -np.inf):
                with Poke(t, h, k, bad):
                    got = S.run(M)
                    want = S.want()
                assert want[7] == 1.0 and (np.isnan(want[slot]) or want[slot] == np.inf)
                same(got.cpu(), want, (shape, name, k, bad))


# ── 7. the periodic CFL switch ────────────────────────────────────────────────────
@pytest.mark.parametrize("shape", R.CFL_SHAPES)
def test_periodic_cfl_switch(M, shape):
    """mac.py:625-626: cfl = dt * max(max|u| / dx, max|v| / dy) with Python's max, then
    `if cfl <= cfl_switch` takes the central branch.  max keeps its first operand unless the
    second compares greater: a NaN in u makes cfl NaN, the comparison False, and the SL branch
    runs; a NaN in v never compares greater and is dropped (the central branch while u is
    small)."""
    ny, nx = shape
    dx, dy, dt = R.CFL_DX, R.CFL_DY, R.CFL_DT
    lap = M.lap_eigs_periodic(nx, ny, dx, dy)
    rng = np.random.default_rng(7)
    u = R.CFL_BASE * rng.choice([-1.0, 1.0], shape); v = R.CFL_BASE * rng.choice([-1.0, 1.0], shape)
    ud, vd = dev(u), dev(v)

    def took():
        return M._predictor_semilag(ud, vd, 0.01, dx, dy, dt, lap, R.CFL_SWITCH)[2]

    assert took() is False and R.cfl_took_sl(u, v) is False
    for k in R.positions(shape, *R.CFL):
        for h, t, spike, want in ((u, ud, R.CFL_U_SPIKE, True), (u, ud, -R.CFL_U_SPIKE, True),
                                  (v, vd, -R.CFL_V_SPIKE, True), (v, vd, R.CFL_V_BELOW, False),
                                  (u, ud, np.nan, True), (v, vd, np.nan, False)):
            with Poke(t, h, k, spike):
                assert R.cfl_took_sl(u, v) is want
                got = took()
            assert got is want, (shape, k, spike, got, want)
    assert took() is False


# ── 8. rmt_two_solid_diag ─────────────────────────────────────────────────────────
@pytest.mark.parametrize("shape", R.TWO_SHAPES)
def test_two_solid_diag(F, shape):
    from pyrmt_amd import _lib as L
    ny, nx = shape
    n = ny * nx
    X, Y, _, _ = F.create_grid(nx, ny, 1.0, 1.0)
    pa = np.ones(shape); pb = np.ones(shape); J = np.ones(shape)
    Xd, Yd, pad, pbd, Jd = map(dev, (X, Y, pa, pb, J))
    ctx = F.ctx_for(ny, nx)

    def run():
        out = (ctypes.c_double * 5)()
        L.check(L.lib().rmt_two_solid_diag(ctx.bind(), F._p(pad), F._p(pbd), F._p(Xd), F._p(Yd),
                                           F._p(Jd), out), "rmt_two_solid_diag")
        return np.array(out[:])

    same(run(), [np.nan] * 4 + [1.0], (shape, "no solid cell"))
    for k in R.positions(shape, *R.RED):
        m = n - 1 - k
        with Poke(pad, pa, k, -1.0), Poke(pbd, pb, m, 0.0), Poke(Jd, J, k, 0.25):
            got = run()
            want = R.two_solid_diag(pa, pb, X, Y, J)
            # two_disc_contact.py:104 records Jmin.min(): NaN when any cell's is, whatever
            # the other cells hold; the centroids stay
            with Poke(Jd, J, k, np.nan), Poke(Jd, J, m if m != k else 0, 0.25):
                got_nan = run()
                want_nan = R.two_solid_diag(pa, pb, X, Y, J)
        assert tuple(want) == (X.ravel()[k], Y.ravel()[k], X.ravel()[m], Y.ravel()[m], 0.25)
        same(got, want, (shape, k))
        assert np.isnan(want_nan[4]) and tuple(want_nan[:4]) == tuple(want[:4])
        same(got_nan, want_nan, (shape, k, "NaN in Jmin"))
