"""The soft disc under the integrator ladder (benchmarks/mac_soft_disc_lid.py), the parts that
need no GPU: the NumPy restatement of tests/mac_soft_disc_np.py against the reference's fixture
(bit for bit where there is no CG, sine or spline; to the project's existing bars elsewhere:
1e-14 of the amplitude behind the sine, 1e-12 for a step's fields), the fixture's own conditions,
resolve_integrator (the reference's tests/test_integrator_selector.py restated), the dt table and
the -sl parsing of the driver, and the refusals, which are raised on the host."""
import numpy as np
import pytest

from conftest import golden
import mac_soft_disc_np as NP


@pytest.fixture(scope="module")
def fx():
    return golden("mac_soft_disc")


@pytest.fixture(scope="module")
def ops():
    return golden("mac_soft_disc_ops")


@pytest.fixture(scope="module")
def MO():
    from oracle import mac_oracle
    return mac_oracle


# ---------------------------------------------------------------- the fixture ----
@pytest.mark.parametrize("name", list(NP.TRACES))
def test_trace_fixture_holds_its_conditions(fx, name):
    kw, nsteps, keep = NP.TRACES[name]
    rec, sl, cfl, its = (fx[f"{name}_{k}"] for k in ("record", "sl", "cfl", "its"))
    assert rec.shape == (nsteps, 5) and sl.shape == cfl.shape == (nsteps,) and its.shape == (nsteps, 2)
    assert np.isfinite(rec).all() and fx[f"{name}_keep"].tolist() == list(keep)
    # dt is not clipped: the last row passes t_end by less than dt
    dt, t_end = float(fx[f"{name}_dt"]), float(fx[f"{name}_t_end"])
    assert dt == kw["dt"] and rec[-2, 0] < t_end <= rec[-1, 0] < t_end + dt
    np.testing.assert_array_equal(rec[:, 0], np.cumsum(np.full(nsteps, dt)))
    assert (rec[:, 3] >= 0).all() and (rec[:, 4] <= 20).all()
    use_sl, use_imex, _ = NP.resolve(kw["integrator"])
    assert (its > 0).all() if use_imex else not its.any()
    if use_sl:
        assert sl.any() and not sl.all() and np.abs(cfl - NP.CFL_SWITCH).min() >= 1e-6
        np.testing.assert_array_equal(sl, cfl > NP.CFL_SWITCH)
    else:
        assert not sl.any()


def test_sl_traces_are_the_issue_s(fx):
    assert NP.DT_REF == 0.009375
    for name in ("imex_sl", "elastic_sl"):
        assert float(fx[f"{name}_dt"]) == 5 * NP.DT_REF
        assert int(fx[f"{name}_sl"].sum()) == 15 and len(fx[f"{name}_sl"]) == 18
    cfl = fx["imex_sl_cfl"]
    assert cfl[0] == 0.0 and abs(cfl[1] - 0.57) < 0.01 and abs(cfl.max() - 1.27) < 0.01
    assert abs(np.abs(cfl - NP.CFL_SWITCH).min() - 0.058) < 1e-3


def test_ops_fixture_covers_the_edge_cases(ops):
    for shape in NP.SHAPES:
        k, g = NP.key(shape), NP.op_inputs(shape)
        assert g["dx"] != g["dy"] and np.isfinite(g["u0"]).all() and np.isfinite(g["X1"]).all()
        cfl = g["dt"] * max(np.abs(g["u0"]).max() / g["dx"], np.abs(g["v0"]).max() / g["dy"])
        assert abs(cfl - 0.5) < 1e-12
        assert (g["phi"] <= g["w_cut"]).any() and (g["phi"] > g["w_cut"]).any()
        assert (g["phi"] <= 0)[1:-1, 1:-1].any()
        for iso, clamp in NP.stored_variants(shape):
            v = NP.vkey(iso, clamp)
            fu, fv, J = (ops[f"{k}_{v}_{n}"] for n in ("fu", "fv", "J"))
            assert fu.shape == (shape[0], shape[1] + 1) and fv.shape == (shape[0] + 1, shape[1])
            assert (fu[:, [0, -1]] == 0).all() and (fv[[0, -1], :] == 0).all() and fu.any()
            assert (J[g["phi"] > 0] == 1.0).all()
            if clamp and shape[0] >= 9:
                assert (J == 5.0).any()       # the detG clamp fires
        assert ops[f"{k}_diag"][0] == (g["phi"] <= 0).sum() > 0


# ---------------------------------------------------------------- the restatement ----
@pytest.mark.parametrize("shape", NP.SHAPES, ids=NP.key)
def test_bitwise_operators(ops, shape):
    k, g = NP.key(shape), NP.op_inputs(shape)
    umc, vmc = NP.midpoint_centres(g["u0"], g["v0"], g["u1"], g["v1"])
    np.testing.assert_array_equal(umc, ops[f"{k}_umc"])
    np.testing.assert_array_equal(vmc, ops[f"{k}_vmc"])
    uc, _ = NP.midpoint_centres(g["u0"], g["v0"], g["u0"], g["v0"])
    np.testing.assert_array_equal(uc, 0.5 * (g["u0"][:, :-1] + g["u0"][:, 1:]))   # 0.5 (u + u) is u
    for w, tag in ((g["w_cut"], "adv"), (0.0, "adv0")):
        if f"{k}_{tag}" in ops.files:
            np.testing.assert_array_equal(NP.advect_xi_conservative(
                g["X1"], g["u0"], g["v0"], g["dx"], g["dy"], g["dt"], g["phi"], w), ops[f"{k}_{tag}"])
    J = ops[f"{k}_{NP.vkey(False, 0.0)}_J"]
    d = NP.soft_diag(g["phi"], J, g["u0"], g["v0"], g["dx"], g["dy"])
    np.testing.assert_array_equal(d, ops[f"{k}_diag"])
    np.testing.assert_allclose(d[1:3] / d[0], ops[f"{k}_centroid"], rtol=1e-15)


@pytest.mark.parametrize("shape", NP.SHAPES, ids=NP.key)
def test_solid_force_restated(oracle, ops, shape):
    k, g = NP.key(shape), NP.op_inputs(shape)
    for iso, clamp in NP.stored_variants(shape):
        v = NP.vkey(iso, clamp)
        fu, fv, J, S = NP.solid_force(oracle, g["X1"], g["X2"], g["phi"], g["dx"], g["dy"], g["w_t"],
                                      NP.MU_S, NP.KAPPA, clamp, iso)
        np.testing.assert_array_equal(J, ops[f"{k}_{v}_J"])
        sbar, fbar = ops[f"{k}_{v}_bars"]
        if f"{k}_{v}_S" in ops.files:
            assert (sbar, fbar) == NP.force_bar(ops[f"{k}_{v}_S"], g["phi"], g["w_t"], g["dx"], g["dy"])
            np.testing.assert_allclose(np.stack(S), ops[f"{k}_{v}_S"], rtol=0, atol=sbar)
        np.testing.assert_allclose(fu, ops[f"{k}_{v}_fu"], rtol=0, atol=fbar)
        np.testing.assert_allclose(fv, ops[f"{k}_{v}_fv"], rtol=0, atol=fbar)


STEPS = [(name, k) for name, (_, _, keep) in NP.TRACES.items() for k in keep]


@pytest.mark.parametrize("name,k", STEPS, ids=[f"{n}-{k}" for n, k in STEPS])
def test_one_step_restated(oracle, MO, fx, name, k):
    kw = NP.TRACES[name][0]
    s = {f: fx[f"{name}_before{k}_{f}"] for f in ("u", "v", "X1", "X2")}
    out = NP.step(oracle, MO, s, kw["integrator"], kw["dt"], kw.get("mu_s", 0.1),
                  kw.get("scheme", "semilagrangian"))
    assert out["sl"] == bool(fx[f"{name}_sl"][k - 1])
    np.testing.assert_array_equal(out["J"], fx[f"{name}_after{k}_J"])
    for f in ("u", "v", "X1", "X2"):
        np.testing.assert_allclose(out[f], fx[f"{name}_after{k}_{f}"], rtol=0, atol=NP.STEP_BAR,
                                   err_msg=f)
    # the bar is a fair demand here: the reference's one-ulp response, as the generator measured
    assert fx[f"{name}_noise{k}"].max() <= 0.1 * NP.STEP_BAR
    if name == "explicit":      # the map half: no CG, sine or spline
        for f in ("X1", "X2", "phi"):
            np.testing.assert_array_equal(out[f], fx[f"{name}_after{k}_{f}"], err_msg=f)
    # the record row of the step from the diagnostics' selections
    d = NP.soft_diag(out["phi"], out["J"], out["u"], out["v"], NP.DX, NP.DX)
    np.testing.assert_allclose([d[1] / d[0], d[2] / d[0], d[3], d[4]], fx[f"{name}_record"][k - 1, 1:],
                               rtol=1e-13)


# ---------------------------------------------------------------- the host surface ----
@pytest.fixture(scope="module")
def mac():
    from pyrmt_amd import mac
    return mac


def test_resolve_integrator(mac):
    """The reference's tests/test_integrator_selector.py."""
    r = mac.resolve_integrator
    assert mac.INTEGRATORS == ("explicit", "imex", "imex-elastic")
    assert r("explicit") == ("explicit", False, False)
    assert r("imex") == ("imex", True, False)
    assert r("imex-elastic") == ("imex-elastic", True, True)
    assert r("IMEX_Elastic")[0] == "imex-elastic" and r("elastic")[0] == "imex-elastic"
    assert r("implicit-viscosity")[0] == "imex" and r("semi-implicit")[0] == "imex"
    assert r("forward-euler")[0] == "explicit" and r(" exp ")[0] == "explicit"
    assert r(None) == ("explicit", False, False)
    assert r(None, imex=True) == ("imex", True, False)
    assert r(None, implicit_visc=True) == ("imex", True, False)
    assert r(None, elastic_imex=True) == ("imex-elastic", True, True)
    with pytest.raises(ValueError, match="unknown integrator"):
        r("bogus")
    with pytest.raises(ValueError, match="not available"):
        r("imex-elastic", supports_elastic=False)
    with pytest.raises(ValueError, match="not available"):
        r(None, elastic_imex=True, supports_elastic=False)


def test_default_dt_table(mac):
    """mac_soft_disc_lid.py:63-74 for N = 32 and 128, mu_s 0.1 and 8."""
    for N in (32, 128):
        dx = 1.0 / N
        for mu_s in (0.1, 8.0):
            adv, visc = 0.3 * dx / 1.0, 0.2 * dx * dx / 0.01
            el = 0.3 * dx / (np.sqrt(mu_s / 1.0) + 1e-9)
            want = {"explicit": min(adv, visc, el), "imex": min(adv, el), "imex-elastic": adv,
                    "imex-sl": min(2.0 * adv, el), "imex-elastic-sl": 2.0 * adv}
            for name, dt in want.items():
                assert mac.MacSoftDisc.default_dt(N, name, mu_s) == dt, (N, mu_s, name)
    assert mac.MacSoftDisc.default_dt(32, "explicit") == NP.DT_REF


def test_sl_suffix_parsing(mac):
    """mac_soft_disc_lid.py:57-62."""
    P = mac.MacSoftDisc.parse_integrator
    assert P(None) == ("explicit", False, False, False)
    assert P(None, imex=True) == ("imex", False, True, False)
    assert P("imex-sl") == ("imex-sl", True, True, False)
    assert P("IMEX_SL") == ("imex-sl", True, True, False)
    assert P("-sl") == ("imex-sl", True, True, False)               # an empty base is imex
    assert P("imex-elastic-sl") == ("imex-elastic-sl", True, True, True)
    assert P("elastic_sl") == ("imex-elastic-sl", True, True, True)
    assert P("explicit-sl") == ("explicit-sl", True, True, False)   # the suffix forces use_imex
    assert P("imex-elastic") == ("imex-elastic", False, True, True)
    assert P("explicit", imex=True) == ("explicit", False, False, False)   # the name wins


def test_refusals_come_before_the_device(mac):
    with pytest.raises(NotImplementedError, match="FMM"):
        mac.MacSoftDisc(32, scheme="conservative")
    with pytest.raises(NotImplementedError, match="FMM"):
        mac.MacSoftDisc(32, reinit=True)
    with pytest.raises(NotImplementedError, match="FMM"):
        mac.mac_soft_disc_run(32, 0.1, scheme="conservative")
    with pytest.raises(ValueError, match="unknown integrator"):
        mac.MacSoftDisc(32, integrator="rk4")
    with pytest.raises(ValueError, match="unknown integrator"):
        mac.MacSoftDisc(32, integrator="bogus-sl")
    with pytest.raises(ValueError, match="scheme"):
        mac.MacSoftDisc(32, scheme="upwind")
    with pytest.raises(ValueError, match="finite"):
        mac.mac_soft_disc_run(32, np.inf)


def test_names_exported():
    from pyrmt_amd import mac, _lib
    for name in ("INTEGRATORS", "resolve_integrator", "solid_force", "midpoint_centres", "soft_diag",
                 "advect_xi_conservative", "MacSoftDisc", "mac_soft_disc_run"):
        assert hasattr(mac, name), name
    for name in ("rmt_mac_solid_force", "rmt_mac_midpoint_centres", "rmt_mac_soft_diag",
                 "rmt_mac_advect_xi_conservative"):
        assert name in _lib.SIGNATURES, name
