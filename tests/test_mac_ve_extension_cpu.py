"""The four-roll-mill viscoelastic driver without a GPU: the NumPy restatement
(tests/mac_ve_extension_np.py) against the reference's own outputs
(tests/golden/mac_ve_extension_ops.npz, mac_ve_extension_runs.npz), the conditions that make the
GPU comparisons of test_gpu_mac_ve_extension.py meaningful, and the public surface.

Bars: the restatement makes the reference's NumPy calls in the reference's order, the oracle
gives the reference's bits for advection and extrapolation, and both sides run on one NumPy
here, so every fixture is an == case -- operators, per-step records, final planes, step counts
and t.
"""
import inspect
import json

import numpy as np
import pytest

from conftest import golden
import mac_ve_extension_np as E

NP, same_bits = E.NP, E.same_bits
eq = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def ops():
    return golden("mac_ve_extension_ops")


@pytest.fixture(scope="module")
def runs():
    return golden("mac_ve_extension_runs")


# ------------------------------------------------------------------ public surface --
def test_public_names_and_signatures():
    from pyrmt_amd import mac
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(mac.momentum_predictor_periodic_imex_elastic) == \
        "u v nu dx dy dt lap_eig cs2 chi_c fu fv rho".split()
    assert inspect.signature(mac.momentum_predictor_periodic_imex_elastic).parameters[
        "rho"].default == 1.0
    d = {k: p.default for k, p in
         inspect.signature(mac.MacViscoelasticExtension).parameters.items()}
    assert d == dict(N=128, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.05, rho=1.0, R=0.13,
                     integrator=None, imex=False, elastic_imex=False, dt=None)
    d = {k: p.default for k, p in inspect.signature(mac.mac_ve_extension_run).parameters.items()}
    assert d["N"] == 128 and d["t_end"] == 12.0 and d["tau"] == 0.5 and d["dt"] is None
    assert sig(mac.compare_integrators) == "N tau t_end eps_rate G mu_f".split()
    for name in ("ve_centre_kinematics", "ve_face_force", "ve_lock", "ve_record",
                 "imex_elastic_rhs"):
        assert callable(getattr(mac, name))
    for name in ("step", "history", "get"):
        assert callable(getattr(mac.MacViscoelasticExtension, name))


def test_abi_table_entries():
    from pyrmt_amd import _lib
    for name, nargs in (("rmt_mac_ve_centre_kinematics", 8), ("rmt_mac_ve_face_force", 12),
                        ("rmt_mac_per_imex_elastic_rhs", 15),
                        ("rmt_mac_per_predictor_imex_elastic", 18), ("rmt_mac_ve_lock", 12),
                        ("rmt_mac_ve_record", 7)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["rmt_ve_lam_max"] == (_lib._I, [_lib._P, _lib._L, _lib._P, _lib._P,
                                                           _lib._L, _lib._P])
    with open(E.FLOOR_JSON) as f:
        j = json.load(f)
    assert j["repeats"] == 20 and j["fft_rel"] == E.FFT_REL and j["bar_factor"] == E.BAR_FACTOR


def test_argument_errors_on_the_host():
    """Shape mismatches and extents below 3 raise before any device is touched."""
    from pyrmt_amd import mac
    z = np.zeros
    with pytest.raises(ValueError, match="one shape"):
        mac.ve_centre_kinematics(z((5, 5)), z((5, 6)), 0.1, 0.1)
    with pytest.raises(ValueError, match=">= 3"):
        mac.ve_centre_kinematics(z((2, 5)), z((2, 5)), 0.1, 0.1)
    with pytest.raises(ValueError, match="one shape"):
        mac.ve_face_force(z((5, 5)), z((5, 5)), z((5, 5)), z((6, 5)), 0.3, 0.1, 0.1, 0.1)
    with pytest.raises(ValueError, match=">= 3"):
        mac.ve_face_force(*(z((5, 2)),) * 4, 0.3, 0.1, 0.1, 0.1)
    with pytest.raises(ValueError, match="one shape"):
        mac.momentum_predictor_periodic_imex_elastic(z((5, 5)), z((5, 5)), 0.1, 0.1, 0.1, 0.1,
                                                     z((5, 5)), 0.3, z((5, 4)), z((5, 5)),
                                                     z((5, 5)))
    with pytest.raises(ValueError, match="one shape"):
        mac.ve_lock(z((5, 5)), z((5, 5)), z((5, 5)), z((4, 5)), z((5, 5)), 0.1, 150.0, 1.0,
                    "imex")
    with pytest.raises(ValueError, match="mode"):
        mac.ve_lock(*(z((5, 5)),) * 5, 0.1, 150.0, 1.0, "exact")
    with pytest.raises(ValueError, match="one shape"):
        mac.ve_record(z(5), z(5), z(5), z(5), z(6), 0)
    with pytest.raises(ValueError, match=">= 3"):
        mac.MacViscoelasticExtension(N=2)
    with pytest.raises(ValueError, match="finite t_end"):
        mac.mac_ve_extension_run(N=8, t_end=np.inf)


def test_resolve_integrator_routing():
    """The driver resolves through resolve_integrator before anything else: an unknown name
    raises there, and the names, aliases and legacy booleans give the ladder's three rungs."""
    from pyrmt_amd import mac
    with pytest.raises(ValueError, match="unknown integrator"):
        mac.MacViscoelasticExtension(N=8, integrator="rk4")
    for kw, want in ((dict(), "explicit"), (dict(imex=True), "imex"),
                     (dict(elastic_imex=True), "imex-elastic"),
                     (dict(integrator="implicit-elastic"), "imex-elastic"),
                     (dict(integrator="IMEX_visc"), "imex"),
                     (dict(integrator="explicit", imex=True), "explicit")):
        name, imex, elastic = mac.resolve_integrator(supports_elastic=True, **kw)
        assert (name, imex, elastic) == (want, want != "explicit", want == "imex-elastic")
        assert E.resolve(**kw)[0] == want or "integrator" in kw
    assert mac.VE_LOCK_MODES == {"explicit": 0, "imex": 1, "imex-elastic": 2}


# --------------------------------------------------------- restatement == reference --
@pytest.mark.parametrize("shape", E.SHAPES, ids=E.key)
def test_operators_equal_the_reference(ops, shape):
    g, k = E.op_inputs(shape), E.key(shape)
    eq(np.array([float(np.sum(g[n])) for n in sorted(g)]), ops[k + "_checksum"])
    H = NP.heaviside(g["phi"], E.W_T)
    assert (H == 0.0).any() and (H == 1.0).any() and ((H > 0.0) & (H < 1.0)).any()
    sm = g["phi"] <= 0
    assert sm[0, 0] and sm[:, 0].any() and sm[0, :].any() and not sm[-1, -1]
    r = E.op_results(NP, g, shape == E.ARITH_ONLY)
    want = {"kin", "rhs", "lock_explicit", "record"}
    if shape != E.ARITH_ONLY:
        want |= {"force", "pred", "lock_imex", "lock_imex-elastic"}
    assert set(r) == want == {n[len(k) + 1:] for n in ops.files if n.startswith(k + "_")} - {
        "checksum"}
    for name, val in r.items():
        assert same_bits(val, ops[f"{k}_{name}"]), (k, name)


def test_chi_one_and_no_force_is_the_imex_right_hand_side():
    """With chi = 1 and f = 0 the elastic right-hand side is u - dt adv: the defect and the
    force add exact zeros."""
    g = E.op_inputs((5, 7))
    one, zero = np.ones((5, 7)), np.zeros((5, 7))
    ru, rv = NP.imex_elastic_rhs(g["u"], g["v"], E.DX, E.DY, E.DT, E.CS2, one, zero, zero, E.RHO)
    au, av = E._adv(g["u"], g["v"], E.DX, E.DY)
    assert same_bits(ru, g["u"] - E.DT * au) and same_bits(rv, g["v"] - E.DT * av)


def _cases():
    return [(E.short_key(*c), E.short_kwargs(*c), E.SHORT_STEPS) for c in E.short_cases()] + [
        (E.LARGE["key"], E.large_kwargs(), E.LARGE["steps"])]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_short_runs_equal_the_reference(oracle, runs, case):
    k, kw, nsteps = case
    kw = dict(kw)
    t, hist, sim = E.run(oracle, NP, kw.pop("N"), kw.pop("t_end"), **kw)
    rec = runs[k + "_record"]
    # the fixture's conditions: no cell changes side under rounding
    assert runs[k + "_min_abs_phi"].min() >= E.MIN_ABS_PHI
    assert len(set(runs[k + "_cells"].tolist())) == 1
    assert len(rec) == nsteps and runs[k + "_dts"][-1] < 0.75 * runs[k + "_dts"][0]
    # step count, t and dt, then everything else
    assert sim.nsteps == nsteps and not sim.stopped and t == rec[-1, 0]
    eq(np.array(sim.dts), runs[k + "_dts"])
    eq(np.array(sim.cells), runs[k + "_cells"])
    assert same_bits(np.array(sim.record), rec), k
    assert hist == [tuple(rec[-1])]
    for name, val in sim.state().items():
        assert same_bits(val, runs[f"{k}_{name}"]), (k, name)


def test_large_step_is_where_the_stabiliser_matters():
    """The large-step case runs at dt_adv, 20 x the short runs' step: c_el k_max^2 is of order
    one there (and 1e-3 at the short step)."""
    N = E.LARGE["N"]
    dt, dx = E.large_dt(), 1.0 / N
    assert dt == pytest.approx(20.0 * E.short_dt(N))
    kmax2 = 8.0 / (dx * dx)
    assert 0.5 < dt * dt * 0.3 * kmax2 < 50.0 and E.short_dt(N)**2 * 0.3 * kmax2 < 0.05


def test_long_run_records(runs):
    """The reference's record of its eight N = 40 runs: which reach the end, and its own five
    checks on them (test_ve_imex_fsi.py, test_elastic_imex.py)."""
    R = {k: runs["long_" + k] for k in E.LONG}
    for k, r in R.items():
        assert bool(r[0]) == (k not in E.DIVERGING), k
    assert R["fsi_explicit"][1] == 401 and R["fsi_explicit"][5] == 1.5141660580750749
    assert R["fsi_explicit"][4] == 1.5142405835503951
    bxx = lambda k: R[k][5]
    assert abs(bxx("fsi_imex") - bxx("fsi_explicit")) / bxx("fsi_explicit") < 0.03
    assert abs(bxx("fsi_imex_3x") - bxx("fsi_explicit")) / bxx("fsi_explicit") < 0.06
    assert abs(bxx("el_elastic_small") - bxx("el_explicit")) / bxx("el_explicit") < 0.025
    assert np.isfinite(bxx("el_elastic_8x"))


@pytest.mark.parametrize("name", E.DIVERGING)
def test_diverging_runs_stop_as_predicted(oracle, runs, name):
    """The two runs that blow up, in the restatement: the step at which the loop's own test
    (:170) ends them and the clause that does -- the outcome a device run is predicted to have.
    Each stops at the reference's step; the explicit run at 3 x the viscous step on `u not all
    finite` (step 12: psi overflows within the step, b_e = inf), the plain IMEX run at 8 x the
    elastic step on `lam_max > 1e4` with every plane still finite (step 6, max|u| = 7e142)."""
    kw = dict(E.LONG_CFG, **E.LONG[name])
    t_end = kw.pop("t_end")
    t, hist, sim = E.run(oracle, NP, kw.pop("N"), t_end, **kw)
    r = runs["long_" + name]
    print(f"{name}: stopped at step {sim.nsteps}, t = {t!r}, by {sim.clause!r}")
    assert sim.stopped and not E.reached(hist, t_end)
    assert sim.nsteps == r[1] and t == r[2]
    assert sim.clause == E.DIVERGING[name]
    st = sim.state()
    assert all(np.isfinite(st[k]).all() for k in ("X1", "X2", "phi"))
