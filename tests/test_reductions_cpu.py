"""The helper of the reduction tests (reductions_np.py) checked on the CPU: the position sets
hold the items the launch shapes single out, the exact-arithmetic expectations equal the
oracle's floating-point results with `==`, the parameter sets put the bounds where the GPU
tests need them, and every NumPy reference agrees with the oracle (or with the restatements
the other tiers already use) wherever one exists."""
import numpy as np
import pytest

import mac_soft_disc_np as SNP
import reductions_np as R


@pytest.mark.parametrize("name,shapes", [
    ("RED", R.TS_SHAPES + R.TWO_SHAPES), ("EPOCH", R.EPOCH_SHAPES), ("SOFT", R.SOFT_SHAPES),
    ("CFL", R.CFL_SHAPES), ("NPSUM", ((82, 100), (130, 129)))])
def test_position_sets(name, shapes):
    T, B = R.LAUNCHES[name]
    second_trip = False
    for shape in shapes:
        rows, cols = shape
        n = rows * cols
        K = R.positions(shape, T, B)
        assert K == sorted(set(K)) and K[0] == 0 and K[-1] == n - 1
        assert all(0 <= k < n for k in K)
        want = {0, 1, 63, 64, T - 1, T, T * B - 1, T * B, T * B + 1, n - 2, n - 1,
                (rows - 1) * cols, cols - 1}
        assert {k for k in want if k < n} <= set(K)
        assert len(K) > len({k for k in want if k < n}) or n < 64   # and the seeded ones
        assert K == R.positions(shape, T, B)          # seeded: the same set every time
        if n > T * B:
            second_trip = True
            assert {T * B - 1, T * B, n - 1} <= set(K)
    assert second_trip, "no shape of this reduction reaches the grid-stride loop's second trip"


def test_exact_shape_fills_the_first_trip():
    """One shape per reduction has n = T * B exactly where a grid allows it."""
    assert 512 * 512 == R.RED[0] * R.RED[1]
    assert 256 * 256 == R.EPOCH[0] * R.EPOCH[1]
    assert 128 * 256 == R.SOFT[0] * R.SOFT[1]
    assert 256 * 512 == R.CFL[0] * R.CFL[1]
    assert 64 * 128 == R.NPSUM[0] * R.NPSUM[1] and 128 * 128 == 2 * 8192
    assert 7 * 1171 == 8192 + 5 and 82 * 100 == 8192 + 8


def test_face_plane_sweeps():
    shape = (4, 6)
    assert R.last_column(shape) == [5, 11, 17, 23]
    assert R.last_row(shape) == [18, 19, 20, 21, 22, 23]


@pytest.mark.parametrize("shape", R.ENERGY_SHAPES)
def test_exact_energies_equal_the_oracle(oracle, shape):
    a4, b4 = R.quarter_ints(shape, 3)
    a, b = a4 / 4.0, b4 / 4.0
    phi = np.ones(shape)
    assert np.all(oracle.smoothed_heaviside(phi, R.ENERGY_W_T) == 1.0)
    ke = oracle.compute_kinetic_energy(a, b, R.KE_RHO_F, R.KE_RHO_S, phi, R.ENERGY_W_T, R.DX, R.DY)
    assert ke == R.ke_exact(a4, b4) and ke > 0
    ed = oracle.compute_viscous_dissipation(a, b, R.ED_MU_F, phi, R.ENERGY_W_T, R.DX, R.DY,
                                            R.ED_ETA_S)
    assert ed == R.dissipation_exact(a4, b4) and ed > 0
    # one item changed: the exact value follows it
    k = a.size // 2
    a4.ravel()[k] += 8
    a = a4 / 4.0
    ke2 = oracle.compute_kinetic_energy(a, b, R.KE_RHO_F, R.KE_RHO_S, phi, R.ENERGY_W_T, R.DX, R.DY)
    assert ke2 == R.ke_exact(a4, b4) != ke


@pytest.mark.parametrize("shape", R.TS_SHAPES)
def test_timestep_parameters_bind_as_planned(oracle, shape):
    a, b = R.ts_base(shape)
    assert np.abs(a).max() <= 0.5 and np.abs(b).max() <= 0.5 and np.hypot(a, b).max() <= 1.0
    solid = oracle.compute_timestep(0 * a, 0 * b, **dict(R.TS_PAR, CFL=0.2))
    base = oracle.compute_timestep(a, b, **R.TS_PAR)
    # c_s = 2 up to the reference's guards; the fluid bound does not bind
    assert base == solid == 0.2 * R.DX / (np.sqrt(4.0 / (1.0 + 1e-12)) + 1e-14)
    for k in (0, a.size - 1):
        for which in (0, 1):
            f = [a.copy(), b.copy()]
            f[which].ravel()[k] = R.TS_SPIKE
            dt = oracle.compute_timestep(f[0], f[1], **R.TS_PAR)
            assert dt < base and dt == 0.2 * R.DX / (np.hypot(f[0], f[1]).max() + 1e-6)
    # the slow solid: the fluid bound binds on the base field, and a NaN removes it
    slow = oracle.compute_timestep(a, b, **R.TS_PAR_SLOW)
    assert slow == 0.2 * R.DX / (np.hypot(a, b).max() + 1e-6)
    f = a.copy(); f.ravel()[a.size // 2] = np.nan
    with np.errstate(invalid="ignore"):
        nan_dt = oracle.compute_timestep(f, b, **R.TS_PAR_SLOW)
    assert nan_dt == oracle.compute_timestep(0 * a, 0 * b, **R.TS_PAR_SLOW) > slow
    f.ravel()[a.size // 2] = np.inf
    assert oracle.compute_timestep(f, b, **R.TS_PAR) == 0.0
    assert oracle.compute_timestep(-0.0 * np.ones(shape), -0.0 * np.ones(shape), **R.TS_PAR) == solid


def test_epoch_distortion_reference():
    J = np.full((9, 12), 2.0); phi = np.ones((9, 12))
    np.testing.assert_array_equal(R.epoch_distortion(J, phi), [-np.inf, np.inf, 0.0])
    phi[3, 4] = 0.0; J[3, 4] = 7.0
    np.testing.assert_array_equal(R.epoch_distortion(J, phi), [7.0, 7.0, 1.0])
    phi[0, 0] = -1.0
    np.testing.assert_array_equal(R.epoch_distortion(J, phi), [7.0, 2.0, 2.0])
    J[8, 11] = np.nan                                       # not a solid cell: ignored
    np.testing.assert_array_equal(R.epoch_distortion(J, phi), [7.0, 2.0, 2.0])
    J[3, 4] = np.nan
    out = R.epoch_distortion(J, phi)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 2.0


@pytest.mark.parametrize("shape", R.SOFT_SHAPES)
def test_centre_sums_equal_the_soft_disc_restatement(shape):
    ny, nx = shape
    rng = np.random.default_rng(5)
    cells = sorted({int(k) for k in rng.integers(0, ny * nx, 40)} | {0, ny * nx - 1})
    phi = np.ones(shape); phi.ravel()[cells] = -1.0
    J = np.ones(shape); u = np.zeros((ny, nx + 1)); v = np.zeros((ny + 1, nx))
    d = SNP.soft_diag(phi, J, u, v, R.DX, R.DY)
    assert tuple(d[:3]) == R.centre_sums(cells, nx)


def test_cfl_switch_reference():
    shape = (5, 7)
    u = np.full(shape, R.CFL_BASE); v = np.full(shape, -R.CFL_BASE)
    assert R.cfl_took_sl(u, v) is False
    assert R.CFL_DT * R.CFL_BASE / R.CFL_DX == 2.0 ** -9
    assert R.CFL_DT * R.CFL_U_SPIKE / R.CFL_DX == 2.0 and R.CFL_DT * R.CFL_U_SPIKE / R.CFL_DY <= 0.9
    assert R.CFL_DT * R.CFL_V_SPIKE / R.CFL_DY == 2.0
    assert R.CFL_DT * R.CFL_V_BELOW / R.CFL_DY == 0.5 and R.CFL_DT * R.CFL_V_BELOW / R.CFL_DX > 0.9
    for plane, spike, want in ((u, R.CFL_U_SPIKE, True), (u, -R.CFL_U_SPIKE, True),
                               (v, R.CFL_V_SPIKE, True), (v, R.CFL_V_BELOW, False),
                               (u, np.nan, True), (v, np.nan, False)):
        old = plane[2, 3]; plane[2, 3] = spike
        assert R.cfl_took_sl(u, v) is want, (spike, want)
        plane[2, 3] = old


def test_two_solid_reference_equals_the_oracle_centroid(oracle):
    ny, nx = 9, 12
    X, Y, _, _ = oracle.create_grid(nx, ny, 1.0, 1.0)
    pa = np.ones((ny, nx)); pb = np.ones((ny, nx)); J = np.ones((ny, nx))
    d = R.two_solid_diag(pa, pb, X, Y, J)
    assert np.isnan(d[:4]).all() and d[4] == 1.0
    pa[2, 5] = 0.0; pb[6, 6] = -1.0; J[4, 4] = 0.25
    d = R.two_solid_diag(pa, pb, X, Y, J)
    assert tuple(d[:2]) == oracle.disc_centroid(pa, X, Y) == (X[2, 5], Y[2, 5])
    assert tuple(d[2:4]) == oracle.disc_centroid(pb, X, Y) == (X[6, 6], Y[6, 6])
    assert d[4] == 0.25
    J[0, 1] = np.nan
    assert np.isnan(R.two_solid_diag(pa, pb, X, Y, J)[4])
