"""The config-5 MAC loop (rmt_mac_sim_step) where its geometry-dependent decisions (mac_sched
per call; mac_cover, mac_diag_rows and the stress grid per step) change: the cases of tests/test_mac_geometry_cpu.py (discs at and across walls, K = 1, 5, 8, N no
multiple of 4 or 64 and odd, a box wider than 256 columns, the origin near and inside a disc,
a grid smaller than one SL tile) against the oracle, and every implementation switch against
the full-grid passes bit for bit.  Then the t_end clipping of the last step, the empty map, and
the single operators away from the fixture's N = 32.

Bars, those test_mac_multi_disc_trace holds for 8 steps at N = 64: centroids rtol 1e-10, J
range rtol 1e-9, u, v and the maps atol 1e-9, t and dt equal, the initial maps bit-equal.  The
single operators restate NumPy's operand order and are compared bit for bit.
"""
import functools
import warnings

import numpy as np
import pytest

from test_mac_geometry_cpu import CASES, EMPTY, FOLDS, initial_flow, oracle_run

pytestmark = pytest.mark.gpu

# all six option sets on these; boxes on / off alone on the rest
SIX = ({"mac_boxes": 0}, {"mac_boxes": 1}, {"mac_boxes": 1, "mac_noop_host": 0},
       {"mac_boxes": 1, "mac_face_sl": 0}, {"mac_boxes": 0, "mac_face_sl": 0},
       {"mac_boxes": 1, "mac_m2_bound": 0})
ALL_SIX = {"walls", "cut", "eight", "near_origin", "wide", "small", "swirl"}
# a call begins with a full pass per disc: the steps of a case over several calls
CALLS = {12: (2, 1, 9), 6: (2, 1, 3), 3: (1, 2), 1: (1,)}


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


def _sim(M, name, options=None):
    """The device loop of a case, started from the case's initial flow (rest for most)."""
    N, specs, kw, _ = CASES[name]
    sim = M.MacMultiDisc(N, specs=specs, options=options, **kw)
    uv = initial_flow(name)
    if uv is not None:
        sim.field("u").copy_(sim.torch.as_tensor(uv[0]))
        sim.field("v").copy_(sim.torch.as_tensor(uv[1]))
    return sim


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def _abs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def _compare(tag, sim, recs, osim, discs=None):
    """The device run against the oracle's records and final state: the figures printed, then
    held to the bars."""
    K = len(osim.specs)
    discs = range(K) if discs is None else discs
    d = sim.diagnostics()
    assert len(d["t"]) == len(recs)
    cx = np.array([r["cx"] for r in recs]); cy = np.array([r["cy"] for r in recs])
    fig = dict(cx=_rel(d["cx"][:, discs], cx[:, discs]), cy=_rel(d["cy"][:, discs], cy[:, discs]),
               u=_abs(sim.get("u"), osim.u), v=_abs(sim.get("v"), osim.v),
               X=max(_abs(sim.get(n, k), osim.refs[k][q]) for k in discs
                     for q, n in enumerate(("X1", "X2"))))
    if len(discs) == K:
        fig["minJ"] = _rel(d["minJ"], [r["minJ"] for r in recs])
        fig["maxJ"] = _rel(d["maxJ"], [r["maxJ"] for r in recs])
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    np.testing.assert_array_equal(d["t"], [r["t"] for r in recs])
    np.testing.assert_array_equal(d["dt"], [r["dt"] for r in recs])
    np.testing.assert_allclose(d["cx"][:, discs], cx[:, discs], rtol=1e-10)
    np.testing.assert_allclose(d["cy"][:, discs], cy[:, discs], rtol=1e-10)
    if len(discs) == K:
        np.testing.assert_allclose(d["minJ"], [r["minJ"] for r in recs], rtol=1e-9)
        np.testing.assert_allclose(d["maxJ"], [r["maxJ"] for r in recs], rtol=1e-9)
    np.testing.assert_allclose(sim.get("u"), osim.u, rtol=0, atol=1e-9)
    np.testing.assert_allclose(sim.get("v"), osim.v, rtol=0, atol=1e-9)
    for k in discs:
        np.testing.assert_allclose(sim.get("X1", k), osim.refs[k][0], rtol=0, atol=1e-9)
        np.testing.assert_allclose(sim.get("X2", k), osim.refs[k][1], rtol=0, atol=1e-9)
    return d


def _state(sim, K):
    f = {f"{n}{k}": sim.get(n, k) for n in ("X1", "X2", "phi") for k in range(K)}
    f.update({n: sim.get(n) for n in ("u", "v", "p")})
    return sim.diagnostics(), f


def _same_bits(a, b, tag=""):
    (d0, f0), (d1, f1) = a, b
    for k in d0:
        np.testing.assert_array_equal(d1[k], d0[k], err_msg=f"{tag} {k}")
    for k in f0:
        np.testing.assert_array_equal(f1[k], f0[k], err_msg=f"{tag} {k}")


# ------------------------------------------------------------ a. against the oracle --
@pytest.mark.parametrize("name", sorted(CASES))
def test_geometry_vs_oracle(M, name):
    """The device loop of a case against the oracle's run at the module's bars; the worst
    figures are printed first (DESIGN.md section 2 has them per case)."""
    N, specs, kw, steps = CASES[name]
    r = oracle_run(name)
    sim = _sim(M, name)
    assert sim.dt == r["sim"].dt
    for k in range(len(specs)):
        np.testing.assert_array_equal(sim.get("X1", k), r["X1_0"][k])
    sim.step(steps)
    d = _compare(f"geometry {name}:", sim, r["recs"], r["sim"])
    # a folded map is flagged in the step that folds (and ends the run), nothing else is
    np.testing.assert_array_equal(d["diverged"], [int(name in FOLDS)] * steps)
    if name in FOLDS:
        sim.step(2)
        assert len(sim.diagnostics()["t"]) == steps


# ------------------------------------------------------------ b. switch variants --
@pytest.mark.parametrize("name", sorted(CASES))
def test_geometry_switches_are_bit_identical(M, name):
    """Every field and diagnostic of each option set against the mac_boxes = 0 run (see
    test_mac_box_mode_is_bit_identical for the switches), the steps split over several calls.

    `origin_inside` found a defect here although both its option sets take the same full-grid
    path: two runs differed at cell (11, 7) of disc 0 (a garbage X2, 1.3e263 seen, or other
    last bits) in 10 of 11 runs on an MI355X, from the unstaged tail of a long chain record
    (test_ring_band_extrapolation_bitwise)."""
    N, specs, kw, steps = CASES[name]
    out = []
    for opts in (SIX if name in ALL_SIX else SIX[:2]):
        sim = _sim(M, name, opts)
        for c in CALLS[steps]:
            sim.step(c)
        out.append((opts, _state(sim, len(specs))))
    assert len(out[0][1][0]["t"]) == steps
    for opts, st in out[1:]:
        _same_bits(out[0][1], st, f"{name} {opts}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ring_band_extrapolation_bitwise(gpu, oracle, mode):
    """The extrapolation of `origin_inside`'s first step alone: the unknown cells are a thin
    ring with known cells on both sides, so a window is nearly full and the fit at (11, 7) has
    45 static and 35 same-call sources -- a chain record of 5152 bytes, more than k_ex_chain
    stages (5120: the tail of the last sum kept what the buffer held before; X2 there was
    0.06858031130899522 for ...506, or garbage).  Such a record now sends the call to the
    sweep.  Every mode bit for bit against the serial order."""
    N, specs, _, _ = CASES["origin_inside"]
    R, cx, cy = specs[0]
    from oracle import mac_oracle as MO
    X1, X2 = MO.MacMultiDisc(N, specs=specs).refs[0]
    phi = oracle.rebuild_phi_disc(X1, X2, cx, cy, R)
    m = (phi <= 0).astype(float)
    assert (phi >= 0).sum() == 64                       # the ring
    ref = oracle.extrapolate_reference_map(X1 * m, X2 * m, phi, 1.0 / N, 1.0 / N, 3)
    gpu.functions.extrapolation_mode(mode)
    try:
        for _ in range(2):
            got = gpu.extrapolate_reference_map(X1 * m, X2 * m, phi, 1.0 / N, 1.0 / N, 3)
            np.testing.assert_array_equal(got[0], ref[0])
            np.testing.assert_array_equal(got[1], ref[1])
    finally:
        gpu.functions.extrapolation_mode(0)


# ------------------------------------------------------------ c. t_end, the empty map --
def test_t_end_clips_the_last_step(M):
    """sim.step(10, t_end = 3.5 dt): three full steps and one of t_end - t, computed as the
    reference driver computes it; nothing after t has reached t_end."""
    from oracle import mac_oracle as MO
    N, specs, kw, _ = CASES["one"]
    osim = MO.MacMultiDisc(N, specs=specs, **kw)
    t_end = 3.5 * osim.dt
    recs = []
    while osim.t < t_end:
        recs.append(osim.step(t_end))
    assert len(recs) == 4 and recs[2]["dt"] == osim.dt and 0 < recs[3]["dt"] < osim.dt
    sim = M.MacMultiDisc(N, specs=specs, **kw)
    sim.step(10, t_end=t_end)
    d = _compare("t_end:", sim, recs, osim)
    assert d["dt"][3] == recs[3]["dt"] and d["t"][3] == recs[3]["t"]
    sim.step(3, t_end=t_end)
    assert len(sim.diagnostics()["t"]) == 4


@functools.lru_cache(maxsize=None)
def _empty_oracle():
    from oracle import mac_oracle as MO
    N, specs = EMPTY
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # the mean of an empty selection
        osim = MO.MacMultiDisc(N, specs=specs)
        rec = osim.step()
    return osim, rec


def test_empty_map(M):
    """A disc holding no cell centre (the `b[1] < b[0]` branch of the box mode): one record,
    flagged (a disc without cells ends the run), its centroid NaN; the other disc, u and v as
    the oracle's first step; boxes on and off bit-identical; later calls add nothing."""
    N, specs = EMPTY
    osim, rec = _empty_oracle()
    assert np.isnan(rec["cx"][0]) and np.isfinite(rec["cx"][1])
    out = []
    for boxes in (1, 0):
        sim = M.MacMultiDisc(N, specs=specs, options={"mac_boxes": boxes})
        assert not sim.get("X1", 0).any() and not sim.get("X2", 0).any()
        sim.step(3)
        d = _compare(f"empty map, mac_boxes {boxes}:", sim, [rec], osim, discs=[1])
        assert len(d["t"]) == 1 and d["diverged"][0] == 1
        assert np.isnan(d["cx"][0, 0]) and np.isnan(d["cy"][0, 0])
        assert not sim.get("X1", 0).any() and not sim.get("X2", 0).any()
        out.append(_state(sim, 2))
        sim.step(2)
        assert len(sim.diagnostics()["t"]) == 1
    # (NaN == NaN under assert_array_equal)
    _same_bits(out[1], out[0], "empty map")


# ------------------------------------------------------------ d. single operators --
OP_N = [5, 6, 33, 100, 257]


def _faces(N):
    rng = np.random.default_rng(N + 1)
    u = rng.standard_normal((N, N + 1)); u[:, 0] = 0.0; u[:, -1] = 0.0
    v = rng.standard_normal((N + 1, N)); v[0, :] = 0.0; v[-1, :] = 0.0
    return rng, u, v


@pytest.mark.parametrize("N", OP_N)
def test_predictor_bitwise_sizes(M, N):
    from oracle import mac_oracle as MO
    rng, u, v = _faces(N)
    dx = dy = 1.0 / N
    fu = rng.standard_normal(u.shape); fv = rng.standard_normal(v.shape)
    for kw in (dict(fu=fu, fv=fv, rho=1.3), dict()):
        us, vs = M.momentum_predictor(u, v, 0.01, dx, dy, 0.3 * dx, 1.0, **kw)
        uo, vo = MO.momentum_predictor(u, v, 0.01, dx, dy, 0.3 * dx, 1.0, **kw)
        np.testing.assert_array_equal(us, uo)
        np.testing.assert_array_equal(vs, vo)


@pytest.mark.parametrize("N", OP_N)
def test_divergence_gradient_bitwise_sizes(M, N):
    from oracle import mac_oracle as MO
    rng, u, v = _faces(N)
    dx = dy = 1.0 / N
    p = rng.standard_normal((N, N))
    np.testing.assert_array_equal(M.divergence(u, v, dx, dy), MO.divergence(u, v, dx, dy))
    np.testing.assert_array_equal(M.gradient_p_u(p, dx), MO.gradient_p_u(p, dx))
    np.testing.assert_array_equal(M.gradient_p_v(p, dy), MO.gradient_p_v(p, dy))


@pytest.mark.parametrize("N", OP_N)
def test_contact_stress_bitwise_sizes(M, N):
    """Two analytic discs overlapping by 0.008 (centres 0.412 apart, radii 0.2 + 0.22): cells
    with both phi < eps = 3 dx at every N, so fc > 0 there, and the boundary rows and columns
    take the zero gradient."""
    from oracle import mac_oracle as MO
    dx = dy = 1.0 / N
    xc = (np.arange(N) + 0.5) * dx
    X, Y = np.meshgrid(xc, xc)
    pa = np.sqrt((X - 0.3) ** 2 + (Y - 0.45) ** 2) - 0.2
    pb = np.sqrt((X - 0.7) ** 2 + (Y - 0.55) ** 2) - 0.22
    eps = 3 * dx
    ref = MO.contact_stress(pa, pb, 2.0, 0.6, eps, dx, dy)
    assert ((pa < eps) & (pb < eps)).any() and any(np.abs(t).max() > 0 for t in ref)
    for a, b in zip(M.contact_stress(pa, pb, 2.0, 0.6, eps, dx, dy), ref):
        np.testing.assert_array_equal(a, b)
