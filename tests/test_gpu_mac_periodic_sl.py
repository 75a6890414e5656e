"""GPU parity of the periodic MAC tier's semi-Lagrangian predictor (mac.py:587-633 and
integrator "imex-sl" of benchmarks/mac_taylor_green_convergence.py; pyrmt_amd.mac through
librmt's macper_sl.hip) against scipy and the reference's own results
(tests/golden/mac_periodic_sl*.npz, gen_mac_periodic_sl.py).

Bars.  Everything here is equal to rounding, like all that lies behind this tier's FFT pair:
1e-12 of the expected field's max-abs (an independent NumPy restatement lands within 6.1e-14
of the reference at these shapes and time steps, test_mac_periodic_sl_cpu.py).  The central
branch is momentum_predictor_periodic_imex bit for bit, and the device loop is this package's
operators composed, bit for bit.  The Taylor-Green runs that cross the CFL switch are held to
4x the distance by which noise of 1e-12 of scale, injected after every predictor and
projection of the reference loop, moves the reference's result (recorded in the fixture),
the margin of the tier's 500-step states.  Each test prints the distance it measured before
it asserts.
"""
import numpy as np
import pytest

from conftest import golden
from test_mac_periodic_sl_cpu import SHAPES, fixture

pytestmark = pytest.mark.gpu

# macper_sl.hip: a workgroup of the prefilter takes SPL_L = 128 samples of a line (8 threads
# of SPL_CH = 16), so an extent of L + 1 or 2L - 1 crosses a workgroup edge with a short last
# chunk, and 17, 31 do the same to a thread's stretch
L, CH = 128, 16
THIN = tuple((n, 4) for n in (CH + 1, 2 * CH - 1, L + 1, 2 * L - 1))
THIN += tuple((4, n) for n, _ in THIN)


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


def _close(what, a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    d = np.abs(a - b).max() / np.abs(b).max()
    print(f"{what}: {d:.3g} of max-abs (bar {rel:g})")
    assert d <= rel, (what, d)


@pytest.mark.parametrize("ny,nx", SHAPES + THIN)
def test_spline_filter_vs_scipy(M, ny, nx):
    from scipy.ndimage import spline_filter
    if (ny, nx) in SHAPES:
        f = fixture(ny, nx)["p"]
    else:
        f = np.random.default_rng(100 * ny + nx).standard_normal((ny, nx))
    got = M.spline_filter_per(f)
    assert got.shape == (ny, nx)
    _close(f"{ny}x{nx} spline_filter_per", got, spline_filter(f, order=3, mode="grid-wrap"))


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_operators_vs_reference(M, ny, nx):
    g = fixture(ny, nx)
    dx, dy, nu, dt = (float(g[k]) for k in ("dx", "dy", "nu", "dt_sl"))
    t = f"{ny}x{nx} "
    _close(t + "_interp_per", M._interp_per(g["p"], g["iq"], g["jq"]), g["interp"])
    _close(t + "_sl_advect_per u", M._sl_advect_per(g["u"], g["u"], g["v"], 0.0, 0.5, dx, dy, dt),
           g["adv_u"])
    _close(t + "_sl_advect_per v", M._sl_advect_per(g["v"], g["u"], g["v"], 0.5, 0.0, dx, dy, dt),
           g["adv_v"])
    su, sv, took = M._predictor_semilag(g["u"], g["v"], nu, dx, dy, dt, g["lap"], 0.9)
    assert took is True and float(g["cfl_sl"]) > 0.9
    _close(t + "semilag u*", su, g["su"]); _close(t + "semilag v*", sv, g["sv"])
    pu, pv = M.momentum_predictor_periodic_semilag(g["u"], g["v"], nu, dx, dy, dt, g["lap"])
    np.testing.assert_array_equal(pu, su); np.testing.assert_array_equal(pv, sv)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_interp_at_integer_coordinates(M, ny, nx):
    """tests/test_semilag.py:17-19 of the reference: the nodes return the field."""
    g = fixture(ny, nx)
    I, J = np.meshgrid(np.arange(float(nx)), np.arange(float(ny)))
    got = M._interp_per(g["p"], I, J)
    assert got.shape == (ny, nx)
    d = np.abs(got - g["p"]).max()
    print(f"{ny}x{nx} _interp_per at the nodes: {d:.3g} (bar 1e-9)")
    assert d < 1e-9


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_central_branch_is_the_imex_predictor(M, ny, nx):
    g = fixture(ny, nx)
    dx, dy, nu, dt = (float(g[k]) for k in ("dx", "dy", "nu", "dt_central"))
    assert float(g["cfl_central"]) < 0.9
    su, sv, took = M._predictor_semilag(g["u"], g["v"], nu, dx, dy, dt, g["lap"], 0.9)
    assert took is False
    iu, iv = M.momentum_predictor_periodic_imex(g["u"], g["v"], nu, dx, dy, dt, g["lap"])
    np.testing.assert_array_equal(su, iu); np.testing.assert_array_equal(sv, iv)
    # and the reference's, whose semilag output at this dt is its IMEX output bit for bit
    _close(f"{ny}x{nx} central u*", su, g["iu"]); _close(f"{ny}x{nx} central v*", sv, g["iv"])


def _composed(M, u, v, nu, dx, dy, dt, rho, nsteps):
    """momentum_predictor_periodic_semilag + project_per, nsteps times, on the device."""
    import torch
    ny, nx = u.shape
    lap = M.lap_eigs_periodic(nx, ny, dx, dy); eig = M.poisson_eigs_periodic(nx, ny, dx, dy)
    u = torch.from_numpy(np.array(u)).cuda(); v = torch.from_numpy(np.array(v)).cuda()
    nsl = 0
    for _ in range(nsteps):
        us, vs, took = M._predictor_semilag(u, v, nu, dx, dy, dt, lap, 0.9)
        nsl += took
        u, v, p = M.project_per(us, vs, dx, dy, dt, rho, eig)
    return tuple(t.cpu().numpy() for t in (u, v, p)), nsl


@pytest.mark.parametrize("ny,nx", ((5, 7), (33, 130)))
def test_device_loop_bitwise_vs_composed_operators(M, ny, nx):
    g = fixture(ny, nx)
    dx, dy, nu, dt = (float(g[k]) for k in ("dx", "dy", "nu", "dt_sl"))
    want, nsl = _composed(M, g["u"], g["v"], nu, dx, dy, dt, 1.3, 3)
    sim = M.MacPeriodic(ny, nx, dx, dy, nu, dt, 1.3, semilag=True)
    sim.set(g["u"], g["v"])
    sim.step(2); sim.step(1)
    print(f"{ny}x{nx} SL loop: {sim.sl_steps} of 3 steps on the SL branch (composed {nsl})")
    assert sim.sl_steps == nsl >= 1
    for name, w in zip("uvp", want):
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        np.testing.assert_array_equal(sim.get(name), w, err_msg=name)


@pytest.fixture(scope="module")
def switch45(M):
    """The N = 45 Taylor-Green run across the switch, composed (once for the module)."""
    g = golden("mac_periodic_sl")
    dx = 2 * np.pi / 45
    Xs = M._tg_faces(45)[1:]
    u, v = M.tg_exact(*Xs, 0.05, 0.0)
    return _composed(M, u, v, 0.05, dx, dx, float(g["tg45_dt"]), 1.0, 12)


@pytest.mark.parametrize("split", ((12,), (5, 7)))
def test_switch_run_bitwise_vs_composed_operators(M, switch45, split):
    g = golden("mac_periodic_sl")
    want, nsl = switch45
    sim = M.MacTaylorGreen(45, 0.05, float(g["tg45_dt"]), semilag=True)
    for n in split:
        sim.step(n)
    assert sim.nsteps == 12
    print(f"N=45 switch run as step{split}: {sim.sl_steps} SL steps (composed {nsl}, "
          f"reference {int(g['tg45_sl_steps'])})")
    assert sim.sl_steps == nsl == int(g["tg45_sl_steps"])
    for name, w in zip("uvp", want):
        np.testing.assert_array_equal(sim.get(name), w, err_msg=name)


@pytest.mark.parametrize("N", (64, 45))
def test_switch_run_vs_reference(M, N):
    g = golden("mac_periodic_sl")
    sim = M.MacTaylorGreen(N, 0.05, float(g[f"tg{N}_dt"]), semilag=True)
    sim.step(12)
    nu_, nv_, np_ = (float(x) for x in g[f"tg{N}_noise"])
    du = np.abs(sim.get("u") - g[f"tg{N}_u"]).max()
    dv = np.abs(sim.get("v") - g[f"tg{N}_v"]).max()
    pr = g[f"tg{N}_p"]
    dp = np.abs(sim.get("p") - pr).max() / np.abs(pr).max()
    print(f"TG switch run N={N}: |du| {du:.3g} (bar {4 * nu_:.3g}) |dv| {dv:.3g} "
          f"(bar {4 * nv_:.3g}) |dp| / max|p| {dp:.3g} (bar {4 * np_:.3g}); "
          f"SL steps {sim.sl_steps} (reference {int(g[f'tg{N}_sl_steps'])})")
    assert sim.sl_steps == int(g[f"tg{N}_sl_steps"])
    assert du <= 4 * nu_ and dv <= 4 * nv_
    assert dp <= 4 * np_


@pytest.mark.parametrize("k,err_bar", ((0, 8e-3), (1, 6e-2)))
def test_run_one_semilag(M, k, err_bar):
    """The reference's integrator="imex-sl" at dt = 0.02 and dt = 2 dx (CFL 2), and its own
    bars (tests/test_semilag.py)."""
    g = golden("mac_periodic_sl")
    dt = float(g["run_dt"][k]); ref = float(g["run_sl"][k, 0])
    e, d = M.taylor_green_run_one(64, nu=0.05, T=1.0, dt=dt, semilag=True)
    print(f"run_one semilag dt={dt:.4g}: err {e!r} (reference {ref!r}, relative "
          f"{e / ref - 1:.2g}), max|div| {d:.2g}")
    assert abs(e - ref) <= 1e-6 * ref
    assert e < err_bar and d < 1e-12
