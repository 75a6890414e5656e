"""GPU parity and accuracy of the periodic MAC tier (mac.py:445-540, 636-650 and
benchmarks/mac_taylor_green_convergence.py; pyrmt_amd.mac through librmt's rmt_mac_per_*)
against the reference's own results (tests/golden/mac_periodic*.npz, gen_mac_periodic.py).

Bars.  The stencil operators (divergence, gradients, explicit predictor) are bit-exact.
Everything that goes through the FFT pair (rocFFT here, pocketfft in the reference) is held
to 1e-12 of the expected field's max-abs, the project's bar for that pair
(test_gpu_periodic.py, test_gpu_imex.py).  The projected field's divergence is held to
1e-12 of the divergence going in (the reference alone leaves 4e-14 of it on unit-normal
data).  The device loop (rmt_mac_per_steps), with the fused predictor + divergence kernel on
and off, is bit-identical to this package's operators composed.  The 500-step Taylor-Green
states are held to 1e-10 (u, v) and 1e-8 max|p| (p): noise of 1e-12 of scale injected after
every predictor and projection of the reference loop moves u, v by 2.8e-11 (N = 64) and
3.6e-11 (N = 45) and p by 1.1e-9 and 1.5e-9 after 500 steps; the bars are 3-4x that.
Each test prints the distance it measured before it asserts.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (20, 36), (64, 64), (33, 130))
_cache = {}


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


def _fixture(ny, nx):
    if (ny, nx) not in _cache:
        if ny * nx > 1000:
            d = dict(golden(f"mac_periodic_{ny}x{nx}"))
        else:
            g = golden("mac_periodic")
            k = f"s{ny}x{nx}_"
            d = {n[len(k):]: g[n] for n in g.files if n.startswith(k)}
        for a in d.values():
            a.setflags(write=False)
        _cache[(ny, nx)] = d
    return _cache[(ny, nx)]


def _close(what, a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.abs(b).max()
    d = np.abs(a - b).max() / scale
    print(f"{what}: {d:.3g} of max-abs (bar {rel:g})")
    assert d <= rel, (what, d)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_stencil_operators_bitwise(M, ny, nx):
    g = _fixture(ny, nx)
    dx, dy = float(g["dx"]), float(g["dy"])
    np.testing.assert_array_equal(M.divergence_per(g["u"], g["v"], dx, dy), g["div"])
    np.testing.assert_array_equal(M.grad_p_u_per(g["p"], dx), g["gu"])
    np.testing.assert_array_equal(M.grad_p_v_per(g["p"], dy), g["gv"])
    pu, pv = M.momentum_predictor_periodic(g["u"], g["v"], float(g["nu"]), dx, dy,
                                           float(g["dt"]))
    np.testing.assert_array_equal(pu, g["pu"])
    np.testing.assert_array_equal(pv, g["pv"])


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_fft_operators_vs_reference(M, ny, nx):
    g = _fixture(ny, nx)
    dx, dy, nu, dt, rho = (float(g[k]) for k in ("dx", "dy", "nu", "dt", "rho"))
    t = f"{ny}x{nx} "
    _close(t + "solve_poisson", M.solve_poisson_periodic(g["p"], g["eig"]), g["sol_p"])
    _close(t + "solve_helmholtz",
           M.solve_helmholtz_periodic(g["p"], g["lap"], float(g["coef"])), g["sol_h"])
    iu, iv = M.momentum_predictor_periodic_imex(g["u"], g["v"], nu, dx, dy, dt, g["lap"])
    _close(t + "imex u*", iu, g["iu"]); _close(t + "imex v*", iv, g["iv"])
    u, v, phi = M.project_per(g["u"], g["v"], dx, dy, dt, rho, g["eig"])
    _close(t + "project u", u, g["proj_u"]); _close(t + "project v", v, g["proj_v"])
    _close(t + "project phi", phi, g["proj_phi"])
    # the projected field is divergence-free to 1e-12 of what went in
    left = np.abs(M.divergence_per(u, v, dx, dy)).max() / np.abs(g["div"]).max()
    print(f"{t}max|div| after / before the projection: {left:.3g} (bar 1e-12)")
    assert left <= 1e-12


def test_helmholtz_periodic_roundtrip(M):
    """tests/test_mac.py:172-185: (I - c L) applied to the solve recovers the rhs."""
    N = 32; dx = 2 * np.pi / N
    rhs = np.random.default_rng(1).standard_normal((N, N))
    c = 0.7
    x = M.solve_helmholtz_periodic(rhs, M.lap_eigs_periodic(N, N, dx, dx), c)
    lapx = ((np.roll(x, -1, 1) - 2 * x + np.roll(x, 1, 1)) / dx**2
            + (np.roll(x, -1, 0) - 2 * x + np.roll(x, 1, 0)) / dx**2)
    res = np.max(np.abs((x - c * lapx) - rhs))
    print(f"Helmholtz round trip residual {res:.3g} (bar 1e-10)")
    assert res < 1e-10


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("integrator", ("explicit", "imex"))
@pytest.mark.parametrize("ny,nx", ((5, 7), (33, 130)))
def test_device_loop_bitwise_vs_composed_operators(M, gpu, ny, nx, integrator, fused):
    """rmt_mac_per_steps against this package's own operators composed three times: the halo
    and wrap test of the fused kernel (an extent below the tile; a tile edge crossed in x
    with the wrap inside a partial tile)."""
    import torch
    g = _fixture(ny, nx)
    dx, dy, nu, dt, rho = (float(g[k]) for k in ("dx", "dy", "nu", "dt", "rho"))
    key = ("composed", ny, nx, integrator)
    if key not in _cache:
        u = torch.from_numpy(g["u"].copy()).cuda(); v = torch.from_numpy(g["v"].copy()).cuda()
        for _ in range(3):
            if integrator == "imex":
                us, vs = M.momentum_predictor_periodic_imex(u, v, nu, dx, dy, dt, g["lap"])
            else:
                us, vs = M.momentum_predictor_periodic(u, v, nu, dx, dy, dt)
            u, v, p = M.project_per(us, vs, dx, dy, dt, rho, g["eig"])
        _cache[key] = tuple(t.cpu().numpy() for t in (u, v, p))
    sim = M.MacPeriodic(ny, nx, dx, dy, nu, dt, rho, integrator, options={"macp_fused": fused})
    assert sim.ctx.get_option("macp_fused") == fused
    sim.set(g["u"], g["v"])
    sim.step(2); sim.step(1)
    for name, want in zip("uvp", _cache[key]):
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        np.testing.assert_array_equal(sim.get(name), want, err_msg=name)


@pytest.mark.parametrize("name", ("exp", "imex"))
def test_taylor_green_second_order_convergence(M, name):
    """tests/test_mac.py:161-169 on the GPU, and the reference's own errors."""
    kw = {} if name == "exp" else {"integrator": "imex"}
    e32, d32 = M.taylor_green_run_one(32, nu=0.05, T=0.1, dt=2e-4, **kw)
    e64, d64 = M.taylor_green_run_one(64, nu=0.05, T=0.1, dt=2e-4, **kw)
    order = np.log(e32 / e64) / np.log(2)
    ref = golden("mac_periodic")["tg_" + name]
    print(f"TG {name}: err {e32!r} {e64!r} order {order:.3f} max|div| {d32:.2g} {d64:.2g}; "
          f"relative to the reference {e32 / ref[0, 0] - 1:.2g} {e64 / ref[1, 0] - 1:.2g}")
    assert order > 1.8, f"TG spatial order {order:.2f} < 1.8"
    assert d32 < 1e-12 and d64 < 1e-12, "periodic projection not divergence-free"
    if name == "exp":
        np.testing.assert_array_equal(ref[:, 0], (1.5834614734709447e-05, 3.9253076215683845e-06))
    else:
        np.testing.assert_array_equal(ref[:, 0], (1.5932988545113585e-05, 4.0241544926445514e-06))
    assert abs(e32 - ref[0, 0]) <= 1e-6 * ref[0, 0]
    assert abs(e64 - ref[1, 0]) <= 1e-6 * ref[1, 0]


def test_imex_stable_beyond_explicit_viscous_limit(M):
    """tests/test_mac.py:188-199, the IMEX half: dt at 6x the explicit limit dx^2 / (4 nu)."""
    N, nu = 64, 0.2
    dx = 2 * np.pi / N
    dt = 6.0 * dx**2 / (4 * nu)
    g = golden("mac_periodic")
    assert dt == float(g["tg_big_dt"])
    e, d = M.taylor_green_run_one(N, nu=nu, T=2.0, dt=dt, implicit_visc=True)
    ref = float(g["tg_big"][0])
    print(f"TG imex at 6x the viscous limit: err {e!r} (reference {ref!r}, relative "
          f"{e / ref - 1:.2g}), max|div| {d:.2g}")
    assert np.isfinite(e) and np.isfinite(d)
    assert e < 5e-3 and d < 1e-12
    assert abs(e - ref) <= 1e-6 * ref


@pytest.mark.parametrize("name", ("exp", "imex"))
@pytest.mark.parametrize("N", (64, 45))
def test_taylor_green_500_step_state(M, N, name):
    g = golden("mac_periodic")
    sim = M.MacTaylorGreen(N, 0.05, 2e-4, "explicit" if name == "exp" else "imex")
    sim.step(500)
    du = np.abs(sim.get("u") - g[f"tg{N}_{name}_u"]).max()
    dv = np.abs(sim.get("v") - g[f"tg{N}_{name}_v"]).max()
    pr = g[f"tg{N}_{name}_p"]
    dp = np.abs(sim.get("p") - pr).max() / np.abs(pr).max()
    print(f"TG {name} N={N} after 500 steps: |du| {du:.3g} |dv| {dv:.3g} (bar 1e-10), "
          f"|dp| / max|p| {dp:.3g} (bar 1e-8)")
    assert du <= 1e-10 and dv <= 1e-10
    assert dp <= 1e-8
