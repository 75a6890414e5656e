"""GPU parity: librmt's HIP kernels (through the C ABI, via pyrmt_amd) against the
reference's golden vectors and the oracle, on the same inputs.

Bars (stated per test):
  * bit-exact for kernels with no transcendental function and no FFT (FD helpers,
    upwind, bilinear, SL-RK4, solid stress, Rhie-Chow divergence, pressure gradient,
    WENO5, pure-fluid momentum, BCs);
  * a momentum step with a solid is bit-exact too on a level set whose H is exact (phi in
    {-1, 0, +1}: H = {0, 0.5, 1}, no sin): tests/test_gpu_offsquare.py, off the square;
  * kernels using sin (smoothed Heaviside) / exp (extrapolation weights) / the DCT-I:
    tolerance stated in the test (device libm and rocFFT differ from glibc/pocketfft in
    the last bits);
  * whole-loop traces: the north-star bar, centroid / energy within 1e-6 relative
    (BASELINE.json), and Ghia RMS within 1e-10 of the reference value.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def _eq(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_fd_helpers_bitwise(gpu):
    g = golden("primitives")
    dx, dy, N = float(g["dx"]), float(g["dy"]), int(g["N"])
    _eq(gpu.grad_central_x_2nd(g["f"], dx), g["gx"])
    _eq(gpu.grad_central_y_2nd(g["f"], dy), g["gy"])
    _eq(gpu.diff_upwind_3rd(g["f"], g["u"], dx, 1), g["up1"])
    _eq(gpu.diff_upwind_3rd(g["f"], g["u"], dy, 0), g["up0"])
    # non-finite -> NaN, huge -> clamped (tests/test_interp_extrap_energy.py:70-81)
    _eq(gpu.bilinear_interpolate(g["f"], g["xq"], g["yq"], dx, dy, N, N), g["bil"])


def test_heaviside_sin_tolerance(gpu):
    g = golden("primitives")
    H = gpu.smoothed_heaviside(g["Hin"], 2 * float(g["dx"]))
    np.testing.assert_allclose(H, g["H"], rtol=0, atol=4e-16)   # device sin vs glibc sin


@pytest.mark.parametrize("mode,kw", [
    ("legacy", {}),
    ("band", dict(band=True, detg_clamp=3.0)),
    ("iso", dict(band=True, detg_clamp=0.0, isochoric=True)),
])
def test_solid_stress_bitwise(gpu, mode, kw):
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    w_cut = 2 * dx if kw.pop("band", False) else 0.0
    r = gpu.solid_cauchy_stress(o["X1"], o["X2"], dx, dy, 0.7, 0.3, o["phi"], w_cut=w_cut, **kw)
    for name, v in zip(("sxx", "sxy", "syy", "J"), r):
        _eq(v, o[f"{mode}_{name}"])


def test_stress_clamp_bounds_J(gpu):
    """tests/test_stress.py:54-65 (detG clamp) bit-exact against the golden."""
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    X, Y, _, _ = gpu.create_grid(49, 49, 1.0, 1.0)
    J = gpu.solid_cauchy_stress(10 * X, Y.copy(), dx, dy, 1.0, 0.0, o["phi"], w_cut=2 * dx,
                                detg_clamp=3.0)[3]
    _eq(J, o["clamp_J"])


def test_sl_advection_bitwise(gpu, oracle):
    s = golden("soft_disc_step12")
    N = int(s["N"])
    X, Y, dx, dy = gpu.create_grid(N, N, 1.0, 1.0)
    for q, ref in (("X1", "X1_adv"), ("X2", "X2_adv")):
        out = gpu.advect_reference_map(s[q], s["a"], s["b"], X, Y, float(s["dt"]), dx, dy,
                                       s["phi_pre"], "semilagrangian")
        _eq(out, s[ref])


def test_extrapolation_bitwise(gpu, oracle):
    """Exact raster-order (Gauss-Seidel) semantics of functions.py:48-163, with the
    weights from the libm-exact exp (pyrmt_amd/csrc/exp_glibc.h): bit-exact."""
    s = golden("soft_disc_step12")
    N = int(s["N"])
    dx = dy = 1.0 / (N - 1)
    X1e, X2e = gpu.extrapolate_reference_map(s["X1_m"], s["X2_m"], s["phi_pre"], dx, dy, 3)
    _eq(X1e, s["X1_ext"]); _eq(X2e, s["X2_ext"])
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    X, Y, _, _ = gpu.create_grid(49, 49, 1.0, 1.0)
    solid = (o["phi"] < 0).astype(float)
    L1e, L2e = gpu.extrapolate_reference_map((1.3 * X + 0.2 * Y) * solid,
                                             (-0.4 * X + 0.9 * Y) * solid, o["phi"], dx, dy, 3)
    _eq(L1e, o["L1e"]); _eq(L2e, o["L2e"])
    D1e, D2e = gpu.extrapolate_reference_map(o["X1"] * solid, o["X2"] * solid, o["phi"], dx, dy, 3)
    _eq(D1e, o["D1e"]); _eq(D2e, o["D2e"])


def _extrap_case(name):
    """Inputs that stress the multi-wave sweep's ordering (k_ex_sweep): long target rows
    (a flat solid edge spans the whole width), several disjoint bodies, solids touching the
    walls, rows wider than one 64-word chunk, many layers, and nothing / everything solid."""
    ny, nx, layers = {"disc1024": (1024, 1024, 3), "slab": (301, 517, 4),
                      "discs3": (700, 640, 2), "rect_l1": (200, 300, 1),
                      "rect_l6": (200, 300, 6), "wide": (96, 4500, 3),
                      "corner": (257, 257, 3), "empty": (64, 80, 3), "full": (64, 80, 3),
                      "tiny": (96, 96, 3),
                      "disc4096": (4096, 4096, 3)}[name]
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    X, Y = np.meshgrid(x, y)
    X1 = X + 0.05 * np.sin(2 * np.pi * Y) * np.cos(np.pi * X)
    X2 = Y + 0.03 * np.sin(2 * np.pi * X)
    disc = lambda cx, cy, R: np.sqrt((X1 - cx) ** 2 + (X2 - cy) ** 2) - R
    if name in ("disc1024", "disc4096", "rect_l1", "rect_l6", "wide", "tiny"):
        phi = disc(0.6, 0.5, 0.2)
    elif name == "slab":
        phi = X2 - 0.4 - 0.02 * np.sin(6 * X1)
    elif name == "discs3":
        phi = np.minimum(np.minimum(disc(0.3, 0.3, 0.12), disc(0.7, 0.35, 0.1)), disc(0.5, 0.75, 0.15))
    elif name == "corner":
        phi = disc(0.0, 0.0, 0.3)
    elif name == "empty":
        phi = np.ones((ny, nx))
    else:
        phi = -np.ones((ny, nx))
    solid = (phi < 0).astype(float)
    if name == "tiny":   # the spacing of N = 8192: det(Aw) < 1e-10 for every fit (config 5)
        return X1 * solid, X2 * solid, phi, 1.0 / 8192, 1.0 / 8192, layers
    return X1 * solid, X2 * solid, phi, 1.0 / (nx - 1), 1.0 / (ny - 1), layers


# cases the chain path must take itself (the others exceed its ring distance and fall back)
_CHAIN_CASES = {"disc1024", "discs3", "rect_l1", "rect_l6", "corner", "disc4096"}
# cases where no fit can be accepted: k_ex_none proves the call is the identity (path 2)
_NOOP_CASES = {"empty", "full", "tiny"}


@pytest.mark.parametrize("name", ["disc1024", "slab", "discs3", "rect_l1", "rect_l6", "wide",
                                  "corner", "empty", "full", "tiny", "disc4096"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_extrapolation_vs_oracle(gpu, oracle, name, mode):
    """Both extrapolation paths reproduce the serial raster-order chain bit for bit, at the
    bench size (4096^2) too: mode 0 = geometry-first chain (extrap_chain.hip), 1 = row-ticket
    sweep alone, 2 = the chain's pre-passes followed by a forced sweep fallback."""
    X1, X2, phi, dx, dy, layers = _extrap_case(name)
    r1, r2 = _extrap_ref(oracle, name)
    gpu.extrapolation_mode(mode)
    try:
        g1, g2 = gpu.extrapolate_reference_map(X1, X2, phi, dx, dy, layers)
        path = gpu.extrapolation_last_path(*phi.shape)
    finally:
        gpu.extrapolation_mode(0)
    _eq(g1, r1); _eq(g2, r2)
    if mode == 0 and name in _CHAIN_CASES:
        assert path == 0, "chain path fell back"
    if mode != 1 and name in _NOOP_CASES:
        assert path == 2, "no-op proof not taken"
        _eq(g1, X1); _eq(g2, X2)
    elif mode != 0:
        assert path == 1


def test_extrapolation_mode_is_per_context(gpu, oracle):
    """Two contexts of one grid in one process, the sweep-only mode on one of them alone:
    alternating calls each take their own context's path, and all give the oracle's bits."""
    import ctypes
    import torch
    from pyrmt_amd import _lib as L, functions as F
    X1, X2, phi, dx, dy, layers = _extrap_case("rect_l1")
    r1, r2 = _extrap_ref(oracle, "rect_l1")
    a, b = F._Ctx(*phi.shape, 0), F.ctx_for(*phi.shape)
    a.set_option("extrap_mode", 1)
    d1, d2, dphi = (torch.from_numpy(x).cuda() for x in (X1, X2, phi))
    for c, want in ((a, 1), (b, 0), (a, 1)):
        o1, o2, path = torch.empty_like(d1), torch.empty_like(d1), ctypes.c_int(-1)
        L.check(L.lib().rmt_extrapolate_reference_map(c.bind(), F._p(d1), F._p(d2), F._p(dphi),
                                                      dx, dy, layers, F._p(o1), F._p(o2)))
        L.check(L.lib().rmt_extrap_last_path(c.bind(), ctypes.byref(path)))
        assert path.value == want
        assert (o1.cpu().numpy() == r1).all() and (o2.cpu().numpy() == r2).all()


_EXTRAP_REF = {}


def _extrap_ref(oracle, name):
    if name not in _EXTRAP_REF:
        X1, X2, phi, dx, dy, layers = _extrap_case(name)
        _EXTRAP_REF[name] = oracle.extrapolate_reference_map(X1, X2, phi, dx, dy, layers)
    return _EXTRAP_REF[name]


def test_momentum_pure_fluid_bitwise(gpu, oracle):
    """phi = 1 everywhere -> H = 1 exactly (no sin): bit-exact RK4 momentum."""
    g = golden("lid_cavity_short")
    N = int(g["N"])
    X, Y, dx, dy = gpu.create_grid(N, N, 1.0, 1.0)
    phi = np.ones((N, N))
    args = (g["a"], g["b"], g["p"], X, Y)
    ref = oracle.momentum_step_rk4(*args, 1, 1.0, 0.0, 0.0, 0.0, dx, dy, 3e-3, 0.0, 1.0, phi,
                                   1e-3, 2 * dx)
    out = gpu.momentum_step_rk4(*args, gpu.NoSlipLid(1.0), 0.0, 0.0, 0.0, dx, dy, 3e-3, 0.0, 1.0,
                                phi, 1e-3, 2 * dx)
    _eq(out[0], ref[0]); _eq(out[1], ref[1])


def test_momentum_solid_tolerance(gpu):
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    m = gpu.momentum_step_rk4(o["a"], o["b"], o["p"], o["X1"], o["X2"], gpu.FreeSlipBox(), 0.7, 0.3,
                              0.02, dx, dy, 2e-3, 1.0, 1.0, o["phi"], 0.01, 2 * dx)
    np.testing.assert_allclose(m[0], o["mfs_u"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(m[1], o["mfs_v"], rtol=0, atol=1e-14)
    _eq(m[5], o["mfs_J"])
    m = gpu.momentum_step_rk4(o["a"], o["b"], o["p"], o["X1"], o["X2"], gpu.NoSlipLid(1.0), 0.7,
                              0.3, 0.0, dx, dy, 2e-3, 1.0, 1.0, o["phi"], 0.01, 2 * dx,
                              stress_band=True, detg_clamp=3.0)
    np.testing.assert_allclose(m[0], o["mband_u"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(m[1], o["mband_v"], rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape", [(49, 49), (65, 65), (257, 129), (256, 256), (130, 200),
                                   (300, 4096), (1024, 1024), (4096, 4096), (32, 32),
                                   (30, 94)])
def test_dct_solve_sizes(gpu, oracle, shape):
    """functions.py:1107-1119 against scipy's pocketfft (the reference's own call) on random
    right-hand sides.  Covers the LDS FFT's radix sets (2..13: 49, 65, 129, 4096; up to 23:
    256, 300; the matrix-form 29 / 31 passes: 1024 (n - 1 = 3 11 31), 32, 30, 94) and the
    rocFFT fallback (130, 200: a prime factor > 31 in n - 1).
    Bar: |p_gpu - p_ref| <= 1e-13 * max|p_ref| (different FFT algorithms round differently)."""
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    rng = np.random.default_rng(ny * 7 + nx)
    rhs = rng.standard_normal((ny, nx))
    eig = oracle._precompute_poisson_eigenvalues(nx, ny, dx, dy)
    ref = oracle._solve_poisson_dct(rhs, eig)
    got = gpu._solve_poisson_dct(rhs, eig)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= 1e-13, err


@pytest.mark.parametrize("shape", [(16, 64), (17, 65), (33, 130), (130, 200), (300, 1001)])
def test_divergence_rc_tiles_bitwise(gpu, oracle, shape):
    """functions.py:1016-1070 (Rhie-Chow divergence) bit for bit against the oracle's C
    restatement, at shapes that end the 64 x 16 tiles of k_divergence_t at every offset:
    the kernel shares each gradient / face quotient between neighbouring cells (lane
    shuffles, register reuse down the column), so the tile edges take the extra values."""
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    rng = np.random.default_rng(ny * 31 + nx)
    a, b, p = (rng.standard_normal((ny, nx)) for _ in range(3))
    _eq(gpu._compute_divergence_rc(a, b, p, 2e-3, 1.0, dx, dy),
        oracle._compute_divergence_rc(a, b, p, 2e-3, 1.0, dx, dy))


def test_projection_pieces(gpu):
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    a, b, p = o["a"], o["b"], o["p"]
    _eq(gpu._compute_divergence_rc(a, b, p, 2e-3, 1.0, dx, dy), o["rc"])
    gx, gy = gpu._compute_pressure_gradient(p, dx, dy)
    _eq(gx, o["gpx"]); _eq(gy, o["gpy"])
    eig = gpu._precompute_poisson_eigenvalues(49, 49, dx, dy)
    dct = gpu._solve_poisson_dct(a, eig)           # rocFFT vs pocketfft
    np.testing.assert_allclose(dct, o["dct"], rtol=0, atol=1e-14 * np.abs(o["dct"]).max() * 100)
    lid = gpu.NoSlipLid(1.0)
    pa, pb, pp, _, _ = gpu.pressure_projection_amg(a, b, dx, dy, 2e-3, 1.0, lid, p_prev=p,
                                                   eigenvalues=eig)
    for got, ref in ((pa, o["proj_a"]), (pb, o["proj_b"]), (pp, o["proj_p"])):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
    pa, pb, pp, _, _ = gpu.pressure_projection_amg(a, b, dx, dy, 2e-3, 1.0, lid, p_prev=None,
                                                   eigenvalues=eig)
    for got, ref in ((pa, o["projn_a"]), (pb, o["projn_b"]), (pp, o["projn_p"])):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))


def test_compute_timestep(gpu):
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    a, b = o["a"], o["b"]
    dts = [gpu.compute_timestep(a, b, dx, dy, 0.2, 1e-3, 0.1, 1.0, 0.0, 1.0, mu_f=0.01, eta_s=0.01),
           gpu.compute_timestep(a, b, dx, dy, 0.2, 1e-2, 0.0, 0.0, 0.0, 1.0, mu_f=1e-3),
           gpu.compute_timestep(a, b, dx, dy, 0.2, 1e-4, 1.0, 1.0, 0.0, 1.0, mu_f=1e-3, kappa=2.0),
           gpu.compute_timestep(a, b, dx, dy, 0.3, 1.0, 1.0, 2.0, 0.05, 1.0, mu_f=1e-3, eta_s=0.1)]
    _eq(dts, o["dts"])


def test_weno5_bitwise_vs_oracle(gpu, oracle):
    w = golden("weno")
    dx, dy = float(w["dx"]), float(w["dy"])
    _eq(gpu._weno5_rhs(w["q"], w["a"], w["b"], dx, dy, w["phi"], 0.0),
        oracle._weno5_rhs(w["q"], w["a"], w["b"], dx, dy, w["phi"], 0.0))
    _eq(gpu.advect_weno5_rk3(w["q"], w["a"], w["b"], dx, dy, 1e-3, w["phi"], 0.0), w["qn"])


def test_error_behaviour(gpu):
    N = 17
    X, Y, dx, dy = gpu.create_grid(N, N, 1.0, 1.0)
    a = np.zeros((N, N)); b = np.zeros((N, N)); a[3, 4] = np.nan
    with pytest.raises(FloatingPointError):
        gpu.advect_reference_map(X, a, b, X, Y, 1e-3, dx, dy, X, "semilagrangian")
    with pytest.raises(ValueError):
        gpu.advect_reference_map(X, b, b, X, Y, 1e-3, dx, dy, X, "bogus")
    phi = X - 0.5
    assert gpu.reinitialize_level_set(phi, dx, dy, method="none") is phi
    with pytest.raises(ValueError):
        gpu.reinitialize_level_set(phi, dx, dy, method="bogus")


def test_reference_bc_callables_are_identified(gpu):
    """The drivers' lambdas (soft_disc_in_lid_driven.py:171) work unchanged."""
    from pyrmt_amd.bc import resolve_bc, resolve_shape

    def no_slip_lid_bc(u, v, lid_speed=1.0):
        u = u.copy(); v = v.copy()
        u[:, 0] = 0.0; v[:, 0] = 0.0; u[:, -1] = 0.0; v[:, -1] = 0.0
        u[0, :] = 0.0; v[0, :] = 0.0; u[-1, :] = lid_speed; v[-1, :] = 0.0
        u[0, 0] = u[0, -1] = u[-1, 0] = u[-1, -1] = 0.0
        v[0, 0] = v[0, -1] = v[-1, 0] = v[-1, -1] = 0.0
        return u, v
    assert resolve_bc(lambda u, v: no_slip_lid_bc(u, v, 1.0)) == (1, 1.0)
    d = resolve_shape(lambda X, Y: np.sqrt((X - 0.6) ** 2 + (Y - 0.5) ** 2) - 0.2)
    assert (d.x0, d.y0, d.R) == (0.6, 0.5, 0.2)


# ── whole loop bodies (device-resident fused step) ────────────────────────────────
def test_soft_disc_trace_N65(gpu):
    """Configs 2/4 loop body, 30 steps at N=65 against the reference trace."""
    from pyrmt_amd.simulation import soft_disc_in_lid_driven
    g = golden("soft_disc_trace")
    sim = soft_disc_in_lid_driven(65)
    sim.step(30)
    d = sim.diagnostics()
    tr = np.stack([d["t"], d["cx"], d["cy"], d["minJ"], d["maxJ"]], axis=1)
    np.testing.assert_allclose(tr[:, 0], g["traj"][:, 0], rtol=1e-12)
    np.testing.assert_allclose(tr[:, 1:3], g["traj"][:, 1:3], rtol=1e-6, atol=0)  # north star
    np.testing.assert_allclose(tr[:, 1:3], g["traj"][:, 1:3], rtol=1e-12, atol=0)  # achieved
    np.testing.assert_allclose(tr[:, 3:], g["traj"][:, 3:], rtol=1e-10)
    for k in ("X1", "X2"):
        np.testing.assert_allclose(sim.get(k), g[k], rtol=0, atol=1e-11)
    for k in ("a", "b", "p"):
        np.testing.assert_allclose(sim.get(k), g[k], rtol=0, atol=1e-10 * max(1, np.abs(g[k]).max()))


def test_soft_disc_t_end_clipping(gpu):
    from pyrmt_amd.simulation import soft_disc_in_lid_driven
    g = golden("soft_disc_driver33")
    sim = soft_disc_in_lid_driven(33)
    sim.step(100, t_end=0.006)
    d = sim.diagnostics()
    assert len(d["t"]) == len(g["traj"])
    np.testing.assert_allclose(d["t"], g["traj"][:, 0], rtol=1e-13)
    np.testing.assert_allclose(np.stack([d["cx"], d["cy"]], 1), g["traj"][:, 1:3], rtol=1e-12)


def test_disc_taylor_green_weno5_energies(gpu):
    """Config 3 loop body, 10 steps at N=64: KE, SE, dissipation, total energy."""
    from pyrmt_amd.simulation import disc_in_taylor_green
    g = golden("disc_tg_trace")
    sim = disc_in_taylor_green(64, "weno5")
    sim.step(10)
    d = sim.diagnostics()
    h = np.stack([d[k] for k in ("t", "ke", "se", "diss", "integ")] +
                 [d["ke"] + d["se"] + d["integ"], d["ry"], d["minJ"]], axis=1)
    np.testing.assert_allclose(h, g["hist"], rtol=1e-6)      # north star
    np.testing.assert_allclose(h, g["hist"], rtol=1e-11)     # achieved


def test_lid_cavity_40_steps(gpu):
    from pyrmt_amd.simulation import lid_driven_cavity
    g = golden("lid_cavity_short")
    sim = lid_driven_cavity(1000.0, 129)
    sim.step(40)
    for k in ("a", "b", "p"):
        np.testing.assert_allclose(sim.get(k), g[k], rtol=0, atol=1e-12 * max(1, np.abs(g[k]).max()))


@pytest.mark.parametrize("Re,key", [(100.0, "Re100"), (1000.0, "Re1000")])
def test_ghia_rms_full_run(gpu, Re, key):
    """Config 1 to steady state on the GPU: Ghia RMS within 1e-10 of the reference's
    (pinned by tests/golden/gen_golden.py --ghia from the reference driver)."""
    from pyrmt_amd.simulation import run_lid_driven_cavity, ghia_rms
    pin = golden("ghia_pinned")
    gd = golden(f"ghia{int(Re)}_data")
    sim, steps = run_lid_driven_cavity(Re, 129)
    assert steps == int(pin[f"{key}_steps"])
    rms = ghia_rms(sim, gd["y"], gd["u"])
    assert abs(rms - float(pin[f"{key}_rms"])) < 1e-10, (rms, float(pin[f"{key}_rms"]))


# ── standalone exports of the reference's per-step diagnostics / blended RHS ────────
def test_velocity_rhs_blended_bitwise(gpu):
    """functions.py:897-944 (pyRMT/__init__.py:16): H and rho_local are inputs, so no
    transcendental function is involved: bit-exact against the reference's fixture."""
    g = golden("vrhs")
    dx, dy = float(g["dx"]), float(g["dy"])
    args = (g["u"], g["v"], g["p"], g["sxx"], g["sxy"], g["syy"], dx, dy, g["phi"], 0.01, g["H"],
            None, None, g["rho"])
    ru, rv = gpu.velocity_rhs_blended_optimized(*args, 0.0, 0.0)
    _eq(ru, g["ru0"]); _eq(rv, g["rv0"])
    ru, rv = gpu.velocity_rhs_blended_optimized(*args, g["fx"], g["fy"])
    _eq(ru, g["ru1"]); _eq(rv, g["rv1"])


def test_energy_exports(gpu, oracle):
    """output.py:6-193 (pyRMT/__init__.py:28-31) against the reference's fixture values: the
    strain energy has no transcendental function and is summed in np.sum's order, so it is
    bit-exact; KE and dissipation go through the smoothed Heaviside (device sin vs glibc)."""
    o = golden("operators")
    dx, dy = float(o["dx"]), float(o["dy"])
    se = gpu.compute_strain_energy(o["X1"], o["X2"], o["phi"], 0.7, dx, dy, kappa=0.3)
    assert se == float(o["se"]), (se, float(o["se"]))
    ke = gpu.compute_kinetic_energy(o["a"], o["b"], 1.0, 1.0, o["phi"], 2 * dx, dx, dy)
    ed = gpu.compute_viscous_dissipation(o["a"], o["b"], 0.01, o["phi"], 2 * dx, dx, dy, eta_s=0.02)
    np.testing.assert_allclose(ke, float(o["ke"]), rtol=1e-14)
    np.testing.assert_allclose(ed, float(o["ed"]), rtol=1e-14)
    # larger grids: several full 8192-cell chunks plus a partial one, against the oracle
    N = 333
    X, Y, dx, dy = gpu.create_grid(N, N, 1.0, 1.0)
    phi = np.sqrt((X - 0.45) ** 2 + (Y - 0.55) ** 2) - 0.3
    X1 = X + 0.03 * np.sin(3 * Y); X2 = Y - 0.02 * np.cos(2 * X)
    a = np.sin(2 * np.pi * X) * np.cos(np.pi * Y); b = -np.cos(np.pi * X) * np.sin(2 * np.pi * Y)
    assert gpu.compute_strain_energy(X1, X2, phi, 0.3, dx, dy, 0.1) == \
        oracle.compute_strain_energy(X1, X2, phi, 0.3, dx, dy, kappa=0.1)
    np.testing.assert_allclose(gpu.compute_kinetic_energy(a, b, 1.0, 2.0, phi, 2 * dx, dx, dy),
                               oracle.compute_kinetic_energy(a, b, 1.0, 2.0, phi, 2 * dx, dx, dy),
                               rtol=1e-14)
    np.testing.assert_allclose(gpu.compute_viscous_dissipation(a, b, 0.01, phi, 2 * dx, dx, dy, 0.05),
                               oracle.compute_viscous_dissipation(a, b, 0.01, phi, 2 * dx, dx, dy, 0.05),
                               rtol=1e-14)


@pytest.mark.parametrize("shape", [(40, 37), (97, 130), (257, 129), (300, 1001)])
@pytest.mark.parametrize("bc", ["lid", "freeslip", "periodic"])
def test_momentum_modes_bitwise(gpu, shape, bc):
    """The per-stage kernels (mode 0) and the unfused passes (mode 2) give the same bits:
    solid disc with viscosity (eta_s > 0) and the stress band, tiles that straddle the grid
    edges."""
    ny, nx = shape
    rng = np.random.default_rng(ny * 7 + nx)
    X, Y, dx, dy = gpu.create_grid(nx, ny, 1.0, 1.0)
    u = rng.standard_normal((ny, nx)) * 0.1
    v = rng.standard_normal((ny, nx)) * 0.1
    p = rng.standard_normal((ny, nx))
    X1 = X + 1e-3 * rng.standard_normal((ny, nx))
    X2 = Y + 1e-3 * rng.standard_normal((ny, nx))
    phi = np.sqrt((X - 0.5) ** 2 + (Y - 0.45) ** 2) - 0.2
    kind = {"lid": gpu.NoSlipLid(1.0), "freeslip": gpu.FreeSlipBox(), "periodic": gpu.Periodic()}[bc]
    outs = []
    try:
        for mode in (0, 2):
            gpu.momentum_mode(mode)
            outs.append(gpu.momentum_step_rk4(u, v, p, X1, X2, kind, 0.7, 0.3, 0.05, dx, dy, 2e-3,
                                              1.5, 1.0, phi, 0.01, 2 * dx, stress_band=True,
                                              detg_clamp=3.0))
    finally:
        gpu.momentum_mode(0)
    for o in outs[1:]:
        _eq(o[0], outs[0][0]); _eq(o[1], outs[0][1])


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("case", ["tiny", "tiny_band", "nan", "inf", "negzero"])
def test_momentum_uncertified_operands(gpu, case):
    """The stage kernel's interior tiles divide unchecked only on operands their DivNotes
    certify (divk.hpp); the cases here fail the notes in a whole tile (values below 2^-800),
    in a band of cells, or through one NaN / inf, and must fall back to the checked division:
    every mode bit-identical to the unfused passes (mode 2), signs of zero included."""
    ny, nx = 257, 300
    rng = np.random.default_rng(11)
    X, Y, dx, dy = gpu.create_grid(nx, ny, 1.0, 1.0)
    u = rng.standard_normal((ny, nx)) * 0.1
    v = rng.standard_normal((ny, nx)) * 0.1
    p = rng.standard_normal((ny, nx))
    if case == "tiny":
        u *= 2.0 ** -830; v *= 2.0 ** -830; p *= 2.0 ** -830
    elif case == "tiny_band":
        u[100:120] *= 2.0 ** -1000; p[:, 140:150] *= 2.0 ** -1010
    elif case == "nan":
        u[130, 150] = np.nan
    elif case == "inf":
        v[70, 200] = np.inf
    elif case == "negzero":
        u[:, :] = -0.0; v[:, :] = 0.0; p[:, :] = -0.0
    X1 = X + 1e-3 * rng.standard_normal((ny, nx))
    X2 = Y + 1e-3 * rng.standard_normal((ny, nx))
    phi = np.sqrt((X - 0.5) ** 2 + (Y - 0.45) ** 2) - 0.2
    outs = []
    try:
        for mode in (2, 0):
            gpu.momentum_mode(mode)
            outs.append(gpu.momentum_step_rk4(u, v, p, X1, X2, gpu.NoSlipLid(1.0), 0.7, 0.3, 0.05,
                                              dx, dy, 2e-3, 1.0, 1.0, phi, 0.01, 2 * dx,
                                              stress_band=True, detg_clamp=3.0))
    finally:
        gpu.momentum_mode(0)
    for o in outs[1:]:
        for k in (0, 1):
            a, b = _bits(o[k]), _bits(outs[0][k])
            same = (a == b) | (np.isnan(np.asarray(o[k])) & np.isnan(np.asarray(outs[0][k])))
            assert same.all(), (case, k, np.argwhere(~same)[:5])
