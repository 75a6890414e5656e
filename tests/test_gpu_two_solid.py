"""GPU parity of the two-solid / surface-tension path (pyrmt_amd/csrc/momentum2.hip) against
the reference's golden vectors (tests/golden/two_solid.npz, gen_two_solid.py) and against
compositions of this package's own operators.

Bars:
  * curvature: bit-exact (no transcendental function);
  * contact force: 16 * 2^-52 * k_rep / w_c (delta <= 1 / w_c; the device cos and the rounding
    of 1 + cos each within 2 ulp of a value <= 2, then four correctly rounded products with
    factors <= 1);
  * momentum (surface tension, two solids): 1e-14 on u, v (the device sin inside H, the bar
    of test_gpu_parity.test_momentum_solid_tolerance), J bit-exact; the contact force adds at
    most dt * (its bar) / rho ~ 1e-16;
  * projection with a density array: 1e-12 * max(1, max|ref|) (test_projection_pieces);
  * TwoDiscContact: t, dt to 1e-13 relative, centroids and gap to 1e-6, fields to 1e-11 and p
    to 1e-10 * max|p| (test_soft_disc_trace_N65).
Every test prints the figure it measured before it asserts.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SHAPES = [(48, 48), (64, 128), (35, 130)]
R, K_REP, DT = 0.15, 2.0, 1e-3
MU_S, KAPPA, ETA_S, RHO_S, RHO_F, MU_F = 1.0, 0.3, 0.0, 1.2, 1.0, 0.01
_CASES = {}


def _eq(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def _case(gpu, shape):
    """The fixture's inputs and results at one shape; the level sets are rebuilt (sqrt and the
    arithmetic around it are exact, so these are the generator's arrays bit for bit)."""
    if shape not in _CASES:
        g = golden("two_solid")
        ny, nx = shape
        k = f"s{ny}x{nx}_"
        c = {n[len(k):]: g[n] for n in g.files if n.startswith(k)}
        X, Y, dx, dy = gpu.create_grid(nx, ny, 1.0, 1.0)
        assert dx == float(c["dx"]) and dy == float(c["dy"])
        c.update(X=X, Y=Y, dx=dx, dy=dy, w_t=2 * dx, w_c=3 * dx,
                 pa=gpu.apply_phi_BCs(np.sqrt((X - 0.35) ** 2 + (Y - 0.5) ** 2) - R),
                 pb=gpu.apply_phi_BCs(np.sqrt((X - 0.65) ** 2 + (Y - 0.5) ** 2) - R))
        for comp in "uv":   # the k_rep = 0 result, stored where it differs from k_rep = 2
            full = c["k2_" + comp].copy()
            full.ravel()[c[f"k0_{comp}_idx"]] = c[f"k0_{comp}_val"]
            c["k0_" + comp] = full
        c["k0_J"] = c["k2_J"]
        _CASES[shape] = c
    return _CASES[shape]


# ── 1. curvature ──────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("shape", SHAPES)
def test_curvature_bitwise(gpu, shape):
    c = _case(gpu, shape)
    _eq(gpu.compute_curvature(c["pa"], c["dx"], c["dy"]), c["kap"])


@pytest.mark.parametrize("shape", SHAPES + [(33, 129), (17, 65), (5, 5)])
def test_curvature_vs_gradient_composition(gpu, shape):
    """The tile and halo logic against grad -> host numpy -> grad on a random phi (every cell
    an interface cell), also where the last tile is one cell wide in both axes."""
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 0.7 / (ny - 1)
    phi = np.random.default_rng(ny * 131 + nx).standard_normal(shape)
    px = gpu.grad_central_x_2nd(phi, dx); py = gpu.grad_central_y_2nd(phi, dy)
    mag = np.sqrt(px * px + py * py) + 1e-12
    ref = gpu.grad_central_x_2nd(px / mag, dx) + gpu.grad_central_y_2nd(py / mag, dy)
    _eq(gpu.compute_curvature(phi, dx, dy), ref)


# ── 2. contact force ──────────────────────────────────────────────────────────────
@pytest.mark.parametrize("shape", SHAPES)
def test_contact_force(gpu, shape):
    c = _case(gpu, shape)
    fx, fy = gpu.compute_contact_force(c["pa"], c["pb"], K_REP, c["w_c"], c["dx"], c["dy"])
    bar = 16 * 2.0 ** -52 * K_REP / c["w_c"]
    err = max(np.abs(fx - c["fx"]).max(), np.abs(fy - c["fy"]).max())
    print(f"contact force {shape}: max abs error {err:.3e}, bar {bar:.3e}, "
          f"max |f| {np.abs(c['fx']).max():.3e}")
    assert np.abs(fx).max() > 0
    assert err <= bar
    off = (np.abs(0.5 * (c["pa"] - c["pb"])) >= c["w_c"]) | ~((c["pa"] < 0) | (c["pb"] < 0))
    assert off.any() and not off.all()
    assert np.all(fx[off] == 0.0) and np.all(fy[off] == 0.0)


def test_contact_force_nan_propagates(gpu):
    c = _case(gpu, SHAPES[0])
    pa = c["pa"].copy()
    pa[20, 24] = np.nan
    fx, fy = gpu.compute_contact_force(pa, c["pb"], K_REP, c["w_c"], c["dx"], c["dy"])
    assert np.isnan(fx[20, 24]) and np.isnan(fy[20, 24])
    far = np.ones(pa.shape, bool)
    far[18:23, 22:27] = False       # the NaN reaches its stencil neighbours only
    ref = gpu.compute_contact_force(c["pa"], c["pb"], K_REP, c["w_c"], c["dx"], c["dy"])
    _eq(fx[far], ref[0][far]); _eq(fy[far], ref[1][far])


# ── 3. surface tension ────────────────────────────────────────────────────────────
def test_surface_tension_fixture(gpu):
    o, g = golden("operators"), golden("two_solid")
    dx, dy = float(o["dx"]), float(o["dy"])
    args = (o["a"], o["b"], o["p"], o["X1"], o["X2"], gpu.FreeSlipBox(), 0.7, 0.3, 0.02, dx, dy,
            2e-3, 1.0, 1.0, o["phi"], 0.01, 2 * dx)
    m = gpu.momentum_step_rk4(*args, gamma=0.1)
    eu, ev = np.abs(m[0] - g["st_u"]).max(), np.abs(m[1] - g["st_v"]).max()
    print(f"surface tension: max abs error u {eu:.3e}, v {ev:.3e} (gamma moves u by "
          f"{float(g['st_move']):.3e})")
    np.testing.assert_allclose(m[0], g["st_u"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(m[1], g["st_v"], rtol=0, atol=1e-14)
    _eq(m[5], g["st_J"])
    # below the reference's threshold the gamma = 0 path runs, bit for bit
    m0 = gpu.momentum_step_rk4(*args, gamma=0.0)
    m1 = gpu.momentum_step_rk4(*args, gamma=1e-13)
    for a, b in zip(m0, m1):
        _eq(a, b)
    _eq(m0[0], gpu.momentum_step_rk4(*args)[0])


def _rk4_composed(gpu, u, v, p, X1, X2, phi, bc, mu_s, kappa, dx, dy, dt, rho_s, rho_f, mu_f,
                  w_t, gamma):
    """momentum_step_rk4 (eta_s = 0) from this package's operators; the RK4 combination on the
    host, every multiply and add a separate numpy operation."""
    sxx, sxy, syy, J = gpu.solid_cauchy_stress(X1, X2, dx, dy, mu_s, kappa, phi)
    H = gpu.smoothed_heaviside(phi, w_t)
    dHx = gpu.grad_central_x_2nd(H, dx); dHy = gpu.grad_central_y_2nd(H, dy)
    rho = (1 - H) * rho_s + H * rho_f
    gk = -gamma * gpu.compute_curvature(phi, dx, dy)
    fx = gk * dHx; fy = gk * dHy

    def rhs(us, vs):
        us, vs = gpu.apply_velocity_BCs(bc, us, vs)
        return gpu.velocity_rhs_blended_optimized(us, vs, p, sxx, sxy, syy, dx, dy, phi, mu_f, H,
                                                  dHx, dHy, rho, fx, fy)

    def stage(q, coef, k):
        t = coef * k
        return q + t

    k1u, k1v = rhs(u, v)
    k2u, k2v = rhs(stage(u, 0.5 * dt, k1u), stage(v, 0.5 * dt, k1v))
    k3u, k3v = rhs(stage(u, 0.5 * dt, k2u), stage(v, 0.5 * dt, k2v))
    k4u, k4v = rhs(stage(u, dt, k3u), stage(v, dt, k3v))

    def combine(q, k1, k2, k3, k4):
        s = 2 * k2
        s = k1 + s
        t = 2 * k3
        s = s + t
        s = s + k4
        t = (dt / 6.0) * s
        return q + t

    un, vn = gpu.apply_velocity_BCs(bc, combine(u, k1u, k2u, k3u, k4u),
                                    combine(v, k1v, k2v, k3v, k4v))
    return un, vn, sxx, sxy, syy, J


@pytest.mark.parametrize("bc", ["freeslip", "lid"])
@pytest.mark.parametrize("shape", SHAPES)
def test_surface_tension_vs_composition(gpu, shape, bc):
    c = _case(gpu, shape)
    bc = gpu.FreeSlipBox() if bc == "freeslip" else gpu.NoSlipLid(1.0)
    prm = (0.7, 0.3, c["dx"], c["dy"], 2e-3, RHO_S, RHO_F, MU_F, c["w_t"], 0.1)
    ref = _rk4_composed(gpu, c["u"], c["v"], c["p"], c["X1a"], c["X2a"], c["pa"], bc, *prm)
    mu_s, kappa, dx, dy, dt, rho_s, rho_f, mu_f, w_t, gamma = prm
    got = gpu.momentum_step_rk4(c["u"], c["v"], c["p"], c["X1a"], c["X2a"], bc, mu_s, kappa, 0.0,
                                dx, dy, dt, rho_s, rho_f, c["pa"], mu_f, w_t, gamma=gamma)
    moved = np.abs(got[0] - gpu.momentum_step_rk4(
        c["u"], c["v"], c["p"], c["X1a"], c["X2a"], bc, mu_s, kappa, 0.0, dx, dy, dt, rho_s,
        rho_f, c["pa"], mu_f, w_t)[0]).max()
    print(f"surface tension {shape}: gamma moves u by {moved:.3e}")
    assert moved > 1e-6
    for a, b in zip(got, ref):
        _eq(a, b)


# ── 4. two-solid momentum ─────────────────────────────────────────────────────────
def _two_solid(gpu, c, k_rep, conv=lambda a: a):
    return gpu.momentum_step_rk4_2solids(
        *map(conv, (c["u"], c["v"], c["p"], c["X1a"], c["X2a"], c["X1b"], c["X2b"])),
        gpu.FreeSlipBox(), MU_S, KAPPA, ETA_S, c["dx"], c["dy"], DT, RHO_S, RHO_F,
        conv(c["pa"]), conv(c["pb"]), MU_F, c["w_t"], k_rep=k_rep, w_c=c["w_c"])


@pytest.mark.parametrize("k_rep", [2.0, 0.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_solid_momentum(gpu, shape, k_rep):
    c = _case(gpu, shape)
    k = "k2_" if k_rep > 0 else "k0_"
    un, vn, Jm = _two_solid(gpu, c, k_rep)
    eu, ev = np.abs(un - c[k + "u"]).max(), np.abs(vn - c[k + "v"]).max()
    print(f"two-solid momentum {shape} k_rep={k_rep}: max abs error u {eu:.3e}, v {ev:.3e}")
    np.testing.assert_allclose(un, c[k + "u"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(vn, c[k + "v"], rtol=0, atol=1e-14)
    _eq(Jm, c[k + "J"])


def test_two_solid_numpy_and_tensor_inputs_agree(gpu):
    import torch
    c = _case(gpu, SHAPES[2])
    host = _two_solid(gpu, c, K_REP)
    dev = _two_solid(gpu, c, K_REP, conv=lambda a: torch.from_numpy(a).cuda())
    for h, d in zip(host, dev):
        assert isinstance(h, np.ndarray) and isinstance(d, torch.Tensor) and d.is_cuda
        _eq(h, d.cpu().numpy())
    # w_c defaults to 2 w_t (functions.py:781-782)
    a = gpu.momentum_step_rk4_2solids(
        c["u"], c["v"], c["p"], c["X1a"], c["X2a"], c["X1b"], c["X2b"], gpu.FreeSlipBox(), MU_S,
        KAPPA, ETA_S, c["dx"], c["dy"], DT, RHO_S, RHO_F, c["pa"], c["pb"], MU_F, c["w_t"],
        k_rep=K_REP)
    b = gpu.momentum_step_rk4_2solids(
        c["u"], c["v"], c["p"], c["X1a"], c["X2a"], c["X1b"], c["X2b"], gpu.FreeSlipBox(), MU_S,
        KAPPA, ETA_S, c["dx"], c["dy"], DT, RHO_S, RHO_F, c["pa"], c["pb"], MU_F, c["w_t"],
        k_rep=K_REP, w_c=2.0 * c["w_t"])
    _eq(a[0], b[0]); _eq(a[1], b[1])


# ── 5. projection with a density array constant to rounding ───────────────────────
def test_projection_near_constant_density(gpu):
    c = _case(gpu, SHAPES[0])
    ny, nx = SHAPES[0]
    rho = c["rho"]
    assert 0 < np.ptp(rho) <= 1e-10
    eig = gpu._precompute_poisson_eigenvalues(nx, ny, c["dx"], c["dy"])
    bc = gpu.FreeSlipBox()
    a, b, p, _, _ = gpu.pressure_projection_amg(c["u"], c["v"], c["dx"], c["dy"], DT, rho, bc,
                                                p_prev=c["p"], eigenvalues=eig)
    for name, got, ref in (("a", a, c["proj_a"]), ("b", b, c["proj_b"]), ("p", p, c["proj_p"])):
        bar = 1e-12 * max(1.0, np.abs(ref).max())
        print(f"projection {name}: max abs error {np.abs(got - ref).max():.3e}, bar {bar:.3e}")
    for got, ref in ((a, c["proj_a"]), (b, c["proj_b"]), (p, c["proj_p"])):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
    # the Rhie-Chow divergence takes d_f = dt / mean(rho)
    _eq(gpu._compute_divergence_rc(c["u"], c["v"], c["p"], DT, rho, c["dx"], c["dy"]),
        gpu._compute_divergence_rc(c["u"], c["v"], c["p"], DT, float(np.mean(rho)), c["dx"],
                                   c["dy"]))
    # no previous pressure: the plain divergence
    gpu.pressure_projection_amg(c["u"], c["v"], c["dx"], c["dy"], DT, rho, bc, p_prev=None,
                                eigenvalues=eig)
    # a scalar and an exactly constant array still take the scalar path, bit for bit
    s = gpu.pressure_projection_amg(c["u"], c["v"], c["dx"], c["dy"], DT, 1.0, bc, p_prev=c["p"],
                                    eigenvalues=eig)
    o = gpu.pressure_projection_amg(c["u"], c["v"], c["dx"], c["dy"], DT, np.ones((ny, nx)), bc,
                                    p_prev=c["p"], eigenvalues=eig)
    for x, y in zip(s[:3], o[:3]):
        _eq(x, y)


# ── 6. the two-disc driver ────────────────────────────────────────────────────────
def test_two_disc_contact_driver(gpu):
    g = golden("two_solid")
    N = int(g["drv_N"])
    sim = gpu.simulation.TwoDiscContact(N, tuple(g["drv_centres"]), R, float(g["drv_V0"]), K_REP)
    sim.step(6)
    rec, ref = np.array(sim.record), g["drv_rec"]
    assert rec.shape == ref.shape == (6, 6)
    print("driver record, max abs deviation per column (t, dt, cxa, cxb, gap, minJ):",
          np.abs(rec - ref).max(axis=0))
    fields = {}
    for name in ("a", "b", "p", "X1a", "X2a", "X1b", "X2b", "phi_a", "phi_b"):
        fields[name] = np.abs(sim.get(name) - g["drv_" + name]).max()
    print("driver fields after 6 steps, max abs deviation:",
          {k: f"{v:.3e}" for k, v in fields.items()}, f"max |p| {np.abs(g['drv_p']).max():.3e}")
    np.testing.assert_allclose(rec[:, :2], ref[:, :2], rtol=1e-13, atol=0)
    np.testing.assert_allclose(rec[:, 2:5], ref[:, 2:5], rtol=0, atol=1e-6)
    np.testing.assert_allclose(rec[:, 5], ref[:, 5], rtol=1e-6, atol=0)
    for name, err in fields.items():
        bar = 1e-10 * np.abs(g["drv_p"]).max() if name == "p" else 1e-11
        assert err <= bar, (name, err, bar)
