"""The collocated operators and the RK4 momentum step against the oracle off the square:
nx != ny on every grid, dx != dy on half of them, shapes on the stage kernel's interior-tile
predicate (k_mom_stage / ms_tile, pyrmt_amd/csrc/momentum.hip) and one cell below it, a
transposed grid and two 5-wide ones (tests/offsquare_np.py builds the cases).

Bars:
  * part 1, momentum_step_rk4 with a solid: bit-exact.  The only non-IEEE ingredient of the
    step (gamma = 0) is the sin of the smoothed Heaviside; on the three-level level set
    (phi in {-1, 0, +1}, any w_t < 1) H is exactly {0, 0.5, 1} on the device and in the
    oracle, the ring cells blend the solid and the fluid stress at H = 0.5, and every branch
    on phi is clean, so u*, v*, the stress planes and J of both momentum modes equal the
    oracle's bit for bit: interior and edge tiles, SQ, DC, the last stage, checked and
    unchecked division, the pure-fluid tile shortcut;
  * part 2, every standalone operator without a transcendental function or an FFT: bit-exact;
    smoothed_heaviside on a random field keeps its 4e-16;
  * part 3, the projections: p to 1e-13 max|p_ref| (DCT-I branch, the bar of
    test_dct_solve_sizes) or 1e-12 max|p_ref| (FFT branch, the bar of test_gpu_periodic.py);
    a, b to that p bar carried through the centred gradient of the correction,
    bar_p (dt / rho) / min(dx, dy), plus 4 eps max|a_ref| for the correction's own roundings.
    The worst error / bar of each case is printed; the largest seen are in the docstrings.
"""
import numpy as np
import pytest

import offsquare_np as C

# the shared inputs are read-only arrays; the wrappers copy them to the device at once
pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

EPS = np.finfo(np.float64).eps
grid = pytest.mark.parametrize(
    "shape,kind", [pytest.param(s, k, id=f"{C.sid(s)}-{k}") for s in C.SHAPES for k in C.SPACINGS])


def _eq(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=str(what))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _bc(gpu, name):
    return {"lid": gpu.NoSlipLid(1.0), "freeslip": gpu.FreeSlipBox(), "periodic": gpu.Periodic()}[name]


_KIND = {"lid": (1, 1.0), "freeslip": (2, 0.0), "periodic": (3, 0.0)}   # oracle (bc_kind, lid)
_OUT = ("u", "v", "sxx", "sxy", "syy", "J")
MU_S, KAPPA, MU_F, DT = 0.7, 0.3, 0.01, 2e-3
RHOS = [(1.5, 1.0), (2.0, 2.0)]   # DC off / on (rho_s == rho_f == 2^k)


def _w_t(name, dx):
    return 2 * dx if name == "2dx" else 2.0 ** -7


# ── part 1: the RK4 momentum step ─────────────────────────────────────────────────
def _momentum(gpu, oracle, f, phi, bc, rho, band, eta_s, w_t):
    """One oracle call, then both momentum modes on the same inputs."""
    dx, dy = f["dx"], f["dy"]
    kind, lid = _KIND[bc]
    ref = oracle.momentum_step_rk4(f["u"], f["v"], f["p"], f["X1"], f["X2"], kind, lid, MU_S,
                                   KAPPA, eta_s, dx, dy, DT, rho[0], rho[1], phi, MU_F, w_t,
                                   stress_band=band, detg_clamp=3.0)
    outs = {}
    try:
        for mode in (0, 2):
            gpu.momentum_mode(mode)
            outs[mode] = gpu.momentum_step_rk4(f["u"], f["v"], f["p"], f["X1"], f["X2"],
                                               _bc(gpu, bc), MU_S, KAPPA, eta_s, dx, dy, DT, rho[0],
                                               rho[1], phi, MU_F, w_t, stress_band=band,
                                               detg_clamp=3.0)
    finally:
        gpu.momentum_mode(0)
    return ref, outs


def _first_diff(got, ref):
    d = np.argwhere(_bits(got) != _bits(ref))
    return None if len(d) == 0 else tuple(d[0])


def _assert_step_equal(ref, outs, what):
    for mode, out in outs.items():
        for name, g, r in zip(_OUT, out, ref):
            _eq(g, r, (what, "mode", mode, name, "first differing cell (j, i)", _first_diff(g, r)))


def test_tile_class_coverage(gpu, oracle):
    """The blocks of offsquare_np.BLOCKS reach every tile class: per shape with interior tiles
    an interior tile that is pure fluid and one that straddles the block's edge, on (69, 261)
    an interior tile whose +2 halo is all solid and on (261, 69) such an edge tile, every kind
    of edge tile (S, N, W, E and the four corners) both pure fluid and not, an interior and an
    edge tile that read the ring in their +1 halo only -- and on every one of these level sets
    H is exactly {0, 0.5, 1} on the device and in the oracle, for both values of w_t."""
    seen = {}
    for shape, block in C.SHAPE_BLOCKS:
        phi = C.three_level_phi(shape, C.BLOCKS[shape][block])
        for kind in C.SPACINGS:
            for wname in ("2dx", "2^-7"):
                w_t = _w_t(wname, C.spacing(shape, kind)[0])
                assert w_t < 1.0
                H = oracle.smoothed_heaviside(phi, w_t)
                _eq(np.unique(H), [0.0, 0.5, 1.0])
                _eq(H, np.where(phi > 0, 1.0, np.where(phi < 0, 0.0, 0.5)))
                _eq(gpu.smoothed_heaviside(phi, w_t), H, (shape, block, kind, wname))
                cls = C.tile_classes(phi, w_t)   # the threshold is max(w_t, w_cut, 0) = w_t
                assert sum(c[0] for c in cls) == C.interior_tile_count(shape)
                seen.setdefault(shape, set()).update(cls)
    for shape in C.SHAPES:
        if C.interior_tile_count(shape):
            assert (True, "", "fluid", False) in seen[shape], shape
            assert (True, "", "mixed", True) in seen[shape], shape
        else:
            assert not any(c[0] for c in seen[shape]), shape
    assert (True, "", "solid", False) in seen[(69, 261)]
    assert any(not c[0] and c[2] == "solid" for c in seen[(261, 69)])
    union = set().union(*seen.values())
    for sides in ("S", "N", "W", "E", "SW", "SE", "NW", "NE"):
        assert (False, sides, "fluid", False) in union, sides
        assert any(c[1] == sides and c[2] != "fluid" for c in union), sides
    # the grazing blocks: tile (1, 1) holds phi = 1 only, the ring lies in its +1 halo
    for shape, (jx, ix), (jy, iy) in (((69, 261), (slice(16, 32), 128), (32, slice(64, 128))),
                                      ((36, 132), (slice(16, 32), 63), (15, slice(64, 128)))):
        for block, at in (("graze_x", (jx, ix)), ("graze_y", (jy, iy))):
            phi = C.three_level_phi(shape, C.BLOCKS[shape][block])
            assert (phi[C.TY:2 * C.TY, C.TX:2 * C.TX] == 1.0).all(), (shape, block)
            assert (phi[at] == 0.0).any() and (phi[at] >= 0.0).all(), (shape, block)
    # the 5-wide grids: every tile fails the test on both sides of the thin axis
    assert all(c[1].startswith("SN") for c in seen[(5, 131)])
    assert all(c[1].endswith("WE") for c in seen[(131, 5)])


@pytest.mark.parametrize("bc", ["lid", "freeslip", "periodic"])
@pytest.mark.parametrize("kind", C.SPACINGS)
@pytest.mark.parametrize("shape,block", [pytest.param(s, b, id=f"{C.sid(s)}-{b}")
                                         for s, b in C.SHAPE_BLOCKS])
def test_momentum_bitwise_vs_oracle(gpu, oracle, shape, block, kind, bc):
    """momentum_step_rk4 (modes 0 and 2) against oracle.momentum_step_rk4, bit for bit, on the
    three-level level set: eta_s = 0.05, w_t = 2 dx, both density pairs (DC off / on), with and
    without the stress band (detg_clamp = 3)."""
    f = C.fields(shape, kind)
    phi = C.three_level_phi(shape, C.BLOCKS[shape][block])
    for rho in RHOS:
        for band in (False, True):
            ref, outs = _momentum(gpu, oracle, f, phi, bc, rho, band, 0.05, 2 * f["dx"])
            _assert_step_equal(ref, outs, (rho, "band", band))


@pytest.mark.parametrize("eta_s,wname", [(0.0, "2dx"), (0.05, "2^-7"), (0.0, "2^-7")])
@pytest.mark.parametrize("bc", ["lid", "freeslip", "periodic"])
@pytest.mark.parametrize("kind", C.SPACINGS)
@pytest.mark.parametrize("shape,block", [((37, 133), "straddle"), ((69, 261), "cover"),
                                         ((261, 69), "straddle"), ((5, 131), "thin")],
                         ids=lambda v: C.sid(v) if isinstance(v, tuple) else v)
def test_momentum_bitwise_visc_off_and_narrow_w_t(gpu, oracle, shape, block, kind, bc, eta_s, wname):
    """The subset with eta_s = 0 (the Kelvin-Voigt add off) and with w_t = 2^-7 (another
    threshold for the clamps, the stress band and the pure-fluid tile flags)."""
    f = C.fields(shape, kind)
    phi = C.three_level_phi(shape, C.BLOCKS[shape][block])
    for rho in RHOS:
        for band in (False, True):
            ref, outs = _momentum(gpu, oracle, f, phi, bc, rho, band, eta_s, _w_t(wname, f["dx"]))
            _assert_step_equal(ref, outs, (rho, "band", band))


@pytest.mark.parametrize("kind", C.SPACINGS)
@pytest.mark.parametrize("case", ["tiny", "nan", "negzero"])
def test_momentum_uncertified_operands_vs_oracle(gpu, oracle, case, kind):
    """The operands that fail the interior tiles' DivNotes (test_momentum_uncertified_operands
    compares them with mode 2), here against the oracle on (69, 261): u, v, p scaled by 2^-830,
    one NaN in u inside interior tile (2, 1), an all -0.0 velocity.  Compared as bits, the signs
    of zero included; a NaN equals a NaN whatever its sign and payload (the oracle's x86 and the
    device may pick another operand's payload), every other cell bit for bit."""
    shape = (69, 261)
    f = dict(C.fields(shape, kind))
    u, v, p = f["u"].copy(), f["v"].copy(), f["p"].copy()
    if case == "tiny":
        u *= 2.0 ** -830; v *= 2.0 ** -830; p *= 2.0 ** -830
    elif case == "nan":
        u[40, 100] = np.nan
    else:
        u[:, :] = -0.0; v[:, :] = -0.0
    f.update(u=u, v=v, p=p)
    phi = C.three_level_phi(shape, C.BLOCKS[shape]["straddle"])
    for rho in RHOS:
        ref, outs = _momentum(gpu, oracle, f, phi, "lid", rho, True, 0.05, 2 * f["dx"])
        for mode, out in outs.items():
            for name, g, r in zip(_OUT, out, ref):
                same = (_bits(g) == _bits(r)) | (np.isnan(g) & np.isnan(r))
                assert same.all(), (case, rho, mode, name, np.argwhere(~same)[:5])
        if case == "nan":
            assert np.isnan(ref[0]).any() and not np.isnan(ref[0]).all()


# ── part 2: the standalone operators, bit for bit ─────────────────────────────────
@grid
def test_fd_helpers(gpu, oracle, shape, kind):
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    _eq(gpu.grad_central_x_2nd(f["q"], dx), oracle.grad_central_x_2nd(f["q"], dx))
    _eq(gpu.grad_central_y_2nd(f["q"], dy), oracle.grad_central_y_2nd(f["q"], dy))
    _eq(gpu.diff_upwind_3rd(f["q"], f["u"], dx, 1), oracle.diff_upwind_3rd(f["q"], f["u"], dx, 1))
    _eq(gpu.diff_upwind_3rd(f["q"], f["v"], dy, 0), oracle.diff_upwind_3rd(f["q"], f["v"], dy, 0))


@grid
def test_interpolators(gpu, oracle, shape, kind):
    """500 query points from [-0.1, L + 0.1] per axis and the corners of that box: both clamps
    of both axes are hit."""
    f = C.fields(shape, kind)
    ny, nx = shape
    dx, dy = f["dx"], f["dy"]
    xq, yq = f["xq"], f["yq"]
    assert xq.min() < 0 and yq.min() < 0 and xq.max() > (nx - 1) * dx and yq.max() > (ny - 1) * dy
    for name in ("bilinear_interpolate", "bicubic_interpolate"):
        _eq(getattr(gpu, name)(f["q"], xq, yq, dx, dy, nx, ny),
            getattr(oracle, name)(f["q"], xq, yq, dx, dy, nx, ny), name)


@pytest.mark.parametrize("scheme", ["semilagrangian", "semilagrangian_cubic", "weno5", "central2",
                                    "conservative"])
@grid
def test_advect_reference_map(gpu, oracle, shape, kind, scheme):
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    cuts = (0.0,) if scheme.startswith("semilagrangian") else (0.0, 2 * dx)
    for w_cut in cuts:
        for q in ("X1", "X2"):
            args = (f[q], f["u"], f["v"], f["X"], f["Y"], 1e-3, dx, dy, f["phi"], scheme, w_cut)
            _eq(gpu.advect_reference_map(*args), oracle.advect_reference_map(*args), (q, w_cut))


@grid
def test_eulerian_rhs(gpu, oracle, shape, kind):
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    for name in ("_weno5_rhs", "_central2_rhs", "_conservative_rhs"):
        for w_cut in (0.0, 2 * dx):
            args = (f["X1"], f["u"], f["v"], dx, dy, f["phi"], w_cut)
            _eq(getattr(gpu, name)(*args), getattr(oracle, name)(*args), (name, w_cut))


@pytest.mark.parametrize("mode", ["legacy", "band", "iso"])
@grid
def test_solid_stress(gpu, oracle, shape, kind, mode):
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    kw = {"legacy": {}, "band": dict(w_cut=2 * dx, detg_clamp=3.0),
          "iso": dict(w_cut=2 * dx, detg_clamp=0.0, isochoric=True)}[mode]
    got = gpu.solid_cauchy_stress(f["X1"], f["X2"], dx, dy, MU_S, KAPPA, f["phi"], **kw)
    ref = oracle.solid_cauchy_stress(f["X1"], f["X2"], dx, dy, MU_S, KAPPA, f["phi"], **kw)
    assert (f["phi"] <= 0).any() and (f["phi"] > 0).any()
    for name, g, r in zip(("sxx", "sxy", "syy", "J"), got, ref):
        _eq(g, r, name)


@grid
def test_gradient_divergence_bcs(gpu, oracle, shape, kind):
    """_compute_pressure_gradient, _compute_divergence, and apply_velocity_BCs for the three
    kinds (corners included: the whole planes are compared)."""
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    for g, r in zip(gpu._compute_pressure_gradient(f["p"], dx, dy),
                    oracle._compute_pressure_gradient(f["p"], dx, dy)):
        _eq(g, r)
    _eq(gpu._compute_divergence(f["u"], f["v"], dx, dy),
        oracle._compute_divergence(f["u"], f["v"], dx, dy))
    for bc in ("lid", "freeslip", "periodic"):
        for g, r in zip(gpu.apply_velocity_BCs(_bc(gpu, bc), f["u"], f["v"]),
                        oracle.apply_bc(*_KIND[bc], f["u"], f["v"])):
            _eq(g, r, bc)


@grid
def test_velocity_rhs_blended(gpu, oracle, shape, kind):
    """H and rho_local are inputs, so nothing transcendental: exact, with the scalar-zero and
    the array surface-tension force."""
    f = C.fields(shape, kind)
    for fx, fy in ((0.0, 0.0), (f["f1"], f["f2"])):
        args = (f["u"], f["v"], f["p"], f["s1"], f["s2"], f["s3"], f["dx"], f["dy"], f["phi"],
                MU_F, f["H"], None, None, f["rho"], fx, fy)
        for g, r in zip(gpu.velocity_rhs_blended_optimized(*args),
                        oracle.velocity_rhs_blended_optimized(*args)):
            _eq(g, r)


@grid
def test_periodic_operators(gpu, oracle, shape, kind):
    f = C.fields(shape, kind)
    dx, dy = f["dx"], f["dy"]
    _eq(gpu._compute_divergence_periodic(f["u"], f["v"], dx, dy),
        oracle._compute_divergence_periodic(f["u"], f["v"], dx, dy))
    for g, r in zip(gpu._compute_pressure_gradient_periodic(f["p"], dx, dy),
                    oracle._compute_pressure_gradient_periodic(f["p"], dx, dy)):
        _eq(g, r)


@grid
def test_heaviside_random_field(gpu, oracle, shape, kind):
    """Device sin against glibc's: the bar of test_heaviside_sin_tolerance, 4e-16 absolute."""
    f = C.fields(shape, kind)
    x = f["q"] * 3 * f["dx"]     # most of the field inside the transition width
    w_t = 2 * f["dx"]
    assert (np.abs(x) < w_t).mean() > 0.3 and (x > w_t).any() and (x < -w_t).any()
    np.testing.assert_allclose(gpu.smoothed_heaviside(x, w_t), oracle.smoothed_heaviside(x, w_t),
                               rtol=0, atol=4e-16)


# ── part 3: the projections ───────────────────────────────────────────────────────
_WORST = {}


def _check_projection(tag, got, ref, bar_p_rel, dt, rho, dx, dy):
    (a, b, p), (ar, br, pr) = got, ref
    bar_p = bar_p_rel * np.abs(pr).max()
    ratios = {"p": np.abs(p - pr).max() / bar_p}
    for name, g, r in (("a", a, ar), ("b", b, br)):
        bar = bar_p * (dt / rho) / min(dx, dy) + 4 * EPS * np.abs(r).max()
        ratios[name] = np.abs(g - r).max() / bar
    worst = max(ratios.values())
    key = tag[0]
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    print("projection", tag, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()),
          "| worst so far %.3f" % _WORST[key])
    assert worst <= 1.0, (tag, ratios)


_BIG = [pytest.param(s, k, id=f"{C.sid(s)}-{k}") for s in C.SHAPES if min(s) >= 36
        for k in C.SPACINGS]


@pytest.mark.parametrize("bc", ["lid", "freeslip"])
@pytest.mark.parametrize("shape,kind", _BIG)
def test_projection_neumann(gpu, oracle, shape, kind, bc):
    """pressure_projection_amg (DCT-I branch) against oracle.pressure_projection, with and
    without p_prev (Rhie-Chow / central divergence).  Worst error / bar seen on an MI355X over
    all cases: 0.391 for p (68x260, dx != dy, with p_prev), 0.046 for a, b (68x260, dx = dy, no p_prev)."""
    f = C.fields(shape, kind)
    ny, nx = shape
    dx, dy = f["dx"], f["dy"]
    eig = oracle._precompute_poisson_eigenvalues(nx, ny, dx, dy)
    for p_prev in (f["p"], None):
        ref = oracle.pressure_projection(f["u"], f["v"], dx, dy, DT, 1.0, *_KIND[bc], p_prev, eig)
        got = gpu.pressure_projection_amg(f["u"], f["v"], dx, dy, DT, 1.0, _bc(gpu, bc),
                                          p_prev=p_prev, eigenvalues=eig)[:3]
        _check_projection(("neumann", C.sid(shape), kind, bc, p_prev is not None), got, ref,
                          1e-13, DT, 1.0, dx, dy)


@pytest.mark.parametrize("shape,kind", _BIG)
def test_projection_periodic(gpu, oracle, shape, kind):
    """The periodic branch (reduced-grid FFT) against oracle.pressure_projection_periodic, with
    and without p_prev.  Worst error / bar seen on an MI355X over all cases: 0.011 for p
    (68x260, dx = dy, no p_prev), 0.001 for a, b."""
    f = C.fields(shape, kind)
    ny, nx = shape
    dx, dy = f["dx"], f["dy"]
    eig = oracle._precompute_poisson_eigenvalues_periodic(nx, ny, dx, dy)
    for p_prev in (f["p"], None):
        ref = oracle.pressure_projection_periodic(f["u"], f["v"], dx, dy, DT, 1.0, 3, 0.0, p_prev,
                                                  eig)
        got = gpu.pressure_projection_amg(f["u"], f["v"], dx, dy, DT, 1.0, gpu.Periodic(),
                                          p_prev=p_prev, eigenvalues=eig, bc_type="periodic")[:3]
        _check_projection(("periodic", C.sid(shape), kind, p_prev is not None), got, ref, 1e-12,
                          DT, 1.0, dx, dy)


@pytest.mark.parametrize("shape", [(34, 65), (65, 34), (10, 131)], ids=C.sid)
def test_periodic_fft_solve_offsquare(gpu, oracle, shape):
    """_solve_poisson_fft with mixed parity of m = n - 1 across the two axes (the Nyquist null
    mode exists on the even axis only), dx != dy, to 1e-12 max|p_ref|.  Worst error / bar seen
    on an MI355X: 0.003."""
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 0.7 / (ny - 1)
    rhs = np.random.default_rng(ny * 7 + nx).standard_normal((ny, nx))
    eig = oracle._precompute_poisson_eigenvalues_periodic(nx, ny, dx, dy)
    ref = oracle._solve_poisson_fft(rhs, eig)
    got = gpu._solve_poisson_fft(rhs, eig)
    ratio = np.abs(got - ref).max() / (1e-12 * np.abs(ref).max())
    print("fft solve", C.sid(shape), "error / bar %.3f" % ratio)
    assert ratio <= 1.0, ratio
