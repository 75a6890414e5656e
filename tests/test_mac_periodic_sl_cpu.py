"""The algorithm behind the periodic MAC tier's semi-Lagrangian predictor (macper_sl.hip;
mac.py:587-633), restated in NumPy and held to the reference's own results
(tests/golden/mac_periodic_sl*.npz, gen_mac_periodic_sl.py), and the host side of its Python
names.  No GPU.

The restatement is the project's own text of scipy.ndimage's order-3 "grid-wrap" spline:
  * prefilter_serial: the causal / anticausal recursion pair with the periodic
    initialisations (pole z = sqrt(3) - 2, gain (1 - z)(1 - 1/z), no padding, axis 0 then 1);
  * prefilter_windowed: what the kernels compute -- the pair composed is the two-sided sum
    sqrt(3) * sum_d z^|d| s[(i + d) mod n]; each one-sided half is cut at K = 48 terms
    (|z|^48 / (1 - |z|) = 4.8e-28 left out), so every CH = 16 samples start both recursions
    from a warm-up of their own;
  * evaluate: reduce q - n floor(q / n), four weights, the taps f-1 .. f+2 each wrapped by an
    integer modulo, sum_a sum_b (c[ja, ib] wj[a]) wi[b].
Bars: the restatement against the fixtures 1e-12 of max-abs (the tier's bar for results equal
to rounding), the windowed form against the serial one 1e-14.
"""
import numpy as np
import pytest

from conftest import golden

SHAPES = ((2, 3), (3, 2), (5, 7), (20, 36), (64, 64), (33, 130))
Z = np.sqrt(3.0) - 2.0
K, CH = 48, 16            # macper_sl.hip: SPL_K, SPL_CH
_cache = {}


def fixture(ny, nx):
    """The SL fixture of a shape with the u, v, p, iu, iv, lap it was made from."""
    if (ny, nx) not in _cache:
        big = ny * nx > 1000
        d = {}
        for stem in ("mac_periodic", "mac_periodic_sl"):
            if big:
                d.update(golden(f"{stem}_{ny}x{nx}"))
            else:
                g = golden(stem)
                k = f"s{ny}x{nx}_"
                d.update({n[len(k):]: g[n] for n in g.files if n.startswith(k)})
        for a in d.values():
            a.setflags(write=False)
        _cache[(ny, nx)] = d
    return _cache[(ny, nx)]


# ------------------------------------------------------------------ the restatement --
def _line_serial(c):
    """One axis, lines along the last axis, in place on a copy."""
    c = c * ((1.0 - Z) * (1.0 - 1.0 / Z))
    n = c.shape[-1]
    zi = Z ** np.arange(1, n)
    c[..., 0] = (c[..., 0] + (zi * c[..., :0:-1]).sum(-1)) / (1.0 - Z**n)
    for i in range(1, n):
        c[..., i] += Z * c[..., i - 1]
    c[..., n - 1] = (c[..., n - 1] + (zi * c[..., :n - 1]).sum(-1)) * Z / (Z**n - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = Z * (c[..., i + 1] - c[..., i])
    return c


def _line_windowed(s):
    n = s.shape[-1]
    out = np.empty_like(s)
    for a in range(0, n, CH):
        cp = np.zeros(s.shape[:-1])
        for p in range(a - (K - 1), a):
            cp = s[..., p % n] + Z * cp
        keep = []
        for k in range(CH):
            cp = s[..., (a + k) % n] + Z * cp
            keep.append(cp)
        cm = np.zeros(s.shape[:-1])
        for p in range(a + CH + K - 1, a + CH - 1, -1):
            cm = s[..., p % n] + Z * cm
        for k in range(CH - 1, -1, -1):
            if a + k < n:
                out[..., a + k] = np.sqrt(3.0) * (keep[k] + Z * cm)
            cm = s[..., (a + k) % n] + Z * cm
    return out


def _two_axes(line, f):
    c = line(np.array(f, dtype=np.float64).T).T          # axis 0 (j) first
    return line(np.ascontiguousarray(c))                 # then axis 1 (i)


def prefilter_serial(f):
    return _two_axes(_line_serial, f)


def prefilter_windowed(f):
    return _two_axes(_line_windowed, f)


def _axis(q, n):
    r = q - n * np.floor(q / n)
    f = np.floor(r)
    y = r - f
    t = 1.0 - y
    w0 = t * t * t / 6
    w1 = (y * y * (y - 2) * 3 + 4) / 6
    w2 = (t * t * (t - 2) * 3 + 4) / 6
    w = (w0, w1, w2, 1 - w0 - w1 - w2)
    base = np.clip(f, 0, n).astype(np.int64) - 1
    return w, [(base + a) % n for a in range(4)]


def evaluate(c, iq, jq):
    ny, nx = c.shape
    iq = np.asarray(iq, dtype=np.float64); jq = np.asarray(jq, dtype=np.float64)
    wj, tj = _axis(jq, ny)
    wi, ti = _axis(iq, nx)
    s = np.zeros(iq.shape)
    for a in range(4):
        for b in range(4):
            s += (c[tj[a], ti[b]] * wj[a]) * wi[b]
    return s


def sl_advect(cf, cu, cv, ox, oy, dx, dy, dt):
    ny, nx = cf.shape
    I, J = np.meshgrid(np.arange(nx), np.arange(ny))
    xf = (I + ox) * dx; yf = (J + oy) * dy
    velx = evaluate(cu, xf / dx, yf / dy - 0.5)
    vely = evaluate(cv, xf / dx - 0.5, yf / dy)
    xm = xf - 0.5 * dt * velx; ym = yf - 0.5 * dt * vely
    vxm = evaluate(cu, xm / dx, ym / dy - 0.5)
    vym = evaluate(cv, xm / dx - 0.5, ym / dy)
    xd = xf - dt * vxm; yd = yf - dt * vym
    return evaluate(cf, xd / dx - ox, yd / dy - oy)


def _close(what, a, b, rel):
    d = np.abs(np.asarray(a) - b).max() / np.abs(b).max()
    print(f"{what}: {d:.3g} of max-abs (bar {rel:g})")
    assert d <= rel, (what, d)


# --------------------------------------------------------------------------- tests --
def test_fixture_shapes():
    np.testing.assert_array_equal(golden("mac_periodic_sl")["shapes"], SHAPES)


@pytest.mark.parametrize("prefilter", (prefilter_serial, prefilter_windowed))
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_restatement_against_the_reference(ny, nx, prefilter):
    g = fixture(ny, nx)
    dx, dy, dt = float(g["dx"]), float(g["dy"]), float(g["dt_sl"])
    t = f"{ny}x{nx} {prefilter.__name__} "
    _close(t + "_interp_per", evaluate(prefilter(g["p"]), g["iq"], g["jq"]), g["interp"], 1e-12)
    cu, cv = prefilter(g["u"]), prefilter(g["v"])
    au = sl_advect(cu, cu, cv, 0.0, 0.5, dx, dy, dt)
    av = sl_advect(cv, cu, cv, 0.5, 0.0, dx, dy, dt)
    _close(t + "_sl_advect_per u", au, g["adv_u"], 1e-12)
    _close(t + "_sl_advect_per v", av, g["adv_v"], 1e-12)
    den = 1.0 - dt * float(g["nu"]) * g["lap"]
    _close(t + "semilag u*", np.real(np.fft.ifft2(np.fft.fft2(au) / den)), g["su"], 1e-12)
    _close(t + "semilag v*", np.real(np.fft.ifft2(np.fft.fft2(av) / den)), g["sv"], 1e-12)


@pytest.mark.parametrize("ny,nx", SHAPES + ((7, 1000), (129, 4), (4, 255)))
def test_windowed_prefilter_equals_the_serial_one(ny, nx):
    f = np.random.default_rng(ny * 1000 + nx).standard_normal((ny, nx))
    _close(f"{ny}x{nx} windowed vs serial prefilter", prefilter_windowed(f),
           prefilter_serial(f), 1e-14)


def test_interpolation_at_the_nodes_returns_the_field():
    """tests/test_semilag.py:17-19 of the reference, on the restatement."""
    g = fixture(5, 7)
    I, J = np.meshgrid(np.arange(7.0), np.arange(5.0))
    assert np.abs(evaluate(prefilter_windowed(g["p"]), I, J) - g["p"]).max() < 1e-9


def test_recorded_cfl_margins_and_branches():
    for ny, nx in SHAPES:
        g = fixture(ny, nx)
        sw = float(g["cfl_switch"])
        assert sw == 0.9
        assert float(g["cfl_sl"]) - sw >= 1e-3 and sw - float(g["cfl_central"]) >= 1e-3
        cfl = lambda dt: dt * max(np.abs(g["u"]).max() / float(g["dx"]),      # noqa: E731
                                  np.abs(g["v"]).max() / float(g["dy"]))
        assert cfl(float(g["dt_sl"])) == float(g["cfl_sl"])
        assert cfl(float(g["dt_central"])) == float(g["cfl_central"])
    g = golden("mac_periodic_sl")
    for N, nsl in ((64, 5), (45, 4)):
        cfl = g[f"tg{N}_cfl"]
        assert cfl.shape == (12,) and float(g[f"tg{N}_dt"]) == 0.95 * (2 * np.pi / N)
        assert np.abs(cfl - 0.9).min() == float(g[f"tg{N}_margin"]) >= 1e-3
        # SL in the first steps, central afterwards: the switch is crossed inside the run
        assert (cfl > 0.9).tolist() == [True] * nsl + [False] * (12 - nsl)
        assert int(g[f"tg{N}_sl_steps"]) == nsl
        assert g[f"tg{N}_noise"].shape == (3,) and (g[f"tg{N}_noise"] > 0).all()
    np.testing.assert_array_equal(g["run_sl"][:, 0],
                                  (8.144265683086139e-05, 0.019197405911016357))


def test_host_shape_checks():
    from pyrmt_amd import mac
    p = np.zeros((5, 7)); q = np.zeros(9)
    lap = mac.lap_eigs_periodic(7, 5, 1.0, 1.0)
    for bad in (np.zeros(7), np.zeros((1, 7)), np.zeros((5, 1)), np.zeros((2, 5, 7))):
        with pytest.raises(ValueError):
            mac.spline_filter_per(bad)
        with pytest.raises(ValueError):
            mac._interp_per(bad, q, q)
    with pytest.raises(ValueError):
        mac._interp_per(p, q, np.zeros(8))
    with pytest.raises(ValueError):
        mac._sl_advect_per(p, p, np.zeros((7, 5)), 0.0, 0.5, 1.0, 1.0, 0.1)
    with pytest.raises(ValueError):
        mac._sl_advect_per(np.zeros((5, 6)), p, p, 0.0, 0.5, 1.0, 1.0, 0.1)
    with pytest.raises(ValueError):
        mac.momentum_predictor_periodic_semilag(p, np.zeros((5, 6)), 0.05, 1.0, 1.0, 0.1, lap)
    with pytest.raises(ValueError):
        mac.momentum_predictor_periodic_semilag(p, p, 0.05, 1.0, 1.0, 0.1,
                                                mac.lap_eigs_periodic(5, 7, 1.0, 1.0))


def test_semilag_keyword_names():
    from pyrmt_amd import mac
    R = mac._resolve_periodic_semilag
    assert R(None, True) == "imex" and R("imex", True) == "imex"
    assert R("implicit-viscosity", True) == "imex"
    assert R(None, False) == "explicit" and R("imex", False) == "imex"
    with pytest.raises(ValueError):
        R("explicit", True)
    with pytest.raises(ValueError):
        R("imex-elastic", True)
    # the name itself stays refused, and says where the loop is
    with pytest.raises(NotImplementedError, match="semilag=True"):
        R("imex-sl", True)
    # the loop classes and run_one resolve before they need the device
    with pytest.raises(ValueError):
        mac.MacPeriodic(5, 7, 1.0, 1.0, 0.05, 0.1, integrator="explicit", semilag=True)
    with pytest.raises(ValueError):
        mac.taylor_green_run_one(32, integrator="explicit", semilag=True)
