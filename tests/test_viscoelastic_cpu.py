"""The viscoelastic layer without a GPU: the NumPy restatement (tests/viscoelastic_np.py)
against the reference's own outputs (tests/golden/viscoelastic_ops.npz,
viscoelastic_uniform32.npz), the conditions that make the GPU comparisons of
test_gpu_viscoelastic.py meaningful, and the public surface.

Bars: bit for bit for ucm_* and viscoelastic_stress (arithmetic only).  The other operators go
through NumPy's exp / log / sin / cos / arctan2, whose SIMD loops differ between builds, so ==
would pin the machine and not the code: each case is held to viscoelastic_np.bar(case), 4 x the
case's measured noise floor (profiles/viscoelastic/floor.json, tools/ve_floor.py).
"""
import inspect
import json

import numpy as np
import pytest

from conftest import golden
import viscoelastic_np as V

NP = V.NP


@pytest.fixture(scope="module")
def ops():
    return golden("viscoelastic_ops")


@pytest.fixture(scope="module")
def uni():
    return golden("viscoelastic_uniform32")


_close = V.assert_close


# ------------------------------------------------------------------ public surface --
SIGNATURES = {
    "ucm_local_rhs": "b11 b12 b22 L11 L12 L21 L22 tau",
    "ucm_local_step": "b11 b12 b22 L11 L12 L21 L22 tau dt",
    "sym_log": "a b c", "sym_exp": "a b c",
    "logconf_local_rhs": "p11 p12 p22 L11 L12 L21 L22 tau",
    "logconf_local_step": "p11 p12 p22 L11 L12 L21 L22 tau dt",
    "relax_exact": "p11 p12 p22 tau dt",
    "logconf_local_step_strang": "p11 p12 p22 L11 L12 L21 L22 tau dt",
    "viscoelastic_stress": "b11 b12 b22 G b_ref G_inf",
}
FUSED = ("ucm_local_step", "logconf_local_step", "logconf_local_step_strang")


def test_public_names_and_signatures():
    import pyrmt_amd
    from pyrmt_amd import viscoelastic as ve
    assert pyrmt_amd.viscoelastic is ve
    for name, params in SIGNATURES.items():
        sig = inspect.signature(getattr(ve, name))
        want = params.split() + (["nsteps"] if name in FUSED else [])
        assert list(sig.parameters) == want, name
        if name in FUSED:
            assert sig.parameters["nsteps"].default == 1
    s = inspect.signature(ve.viscoelastic_stress).parameters
    assert s["b_ref"].default is None and s["G_inf"].default == 0.0
    assert inspect.signature(ve.relaxation_tests).parameters["dt"].default == 2e-4
    assert list(inspect.signature(ve.tg_run_compare).parameters) == ["N", "tau", "dt", "T"]
    d = {k: p.default for k, p in inspect.signature(ve.UniformExtension).parameters.items()}
    assert d == dict(N=96, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.02, rho=1.0, R=0.13)
    assert callable(ve.ve_uniform_run)


def test_mismatched_shapes_raise_on_the_host():
    from pyrmt_amd import viscoelastic as ve
    a, b = np.zeros((4, 5)), np.zeros((5, 4))
    with pytest.raises(ValueError):
        ve.sym_exp(a, a, b)
    with pytest.raises(ValueError):
        ve.logconf_local_step(a, a, a, a, b, a, a, 0.5, 0.01)
    with pytest.raises(ValueError):
        ve.viscoelastic_stress(a, a, a, 0.3, (a, a, b), 0.1)
    with pytest.raises(ValueError):
        ve.ucm_local_step(a, a, a, 0.0, 0.0, 0.0, 0.0, 0.5, 0.01, nsteps=0)
    with pytest.raises(ValueError):
        ve.sym_log(np.zeros(0), np.zeros(0), np.zeros(0))


def test_bars_trace_to_the_floor_file():
    with open(V.FLOOR_JSON) as f:
        doc = json.load(f)
    assert doc["repeats"] == 20 and doc["bar_factor"] == V.BAR_FACTOR == 4.0
    for case, floor in doc["floors"].items():
        assert np.isfinite(floor) and floor > 0.0, case
        assert V.bar(case) == 4.0 * floor


# ------------------------------------------------------------------ the restatement --
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.key)
def test_arithmetic_operators_bitwise(ops, shape):
    g, k = V.op_inputs(shape), V.key(shape)
    b, Lc = g["b"], g["L"]
    eq = np.testing.assert_array_equal
    eq(np.stack(NP.ucm_local_step(*b, *Lc, V.TAU, V.DT)), ops[f"{k}_ucm_step"])
    eq(np.stack(NP.viscoelastic_stress(*b, V.G, g["bref"], V.G_INF)), ops[f"{k}_stress_zener"])
    if shape == (33, 70):
        return
    eq(np.stack(NP.ucm_local_rhs(*b, *Lc, V.TAU)), ops[f"{k}_ucm_rhs"])
    eq(np.stack(NP.ucm_local_step(*b, *Lc, V.INF, V.DT)), ops[f"{k}_ucm_step_inf"])
    eq(np.stack(NP.viscoelastic_stress(*b, V.G)), ops[f"{k}_stress"])
    eq(np.stack(NP.viscoelastic_stress(*b, V.G, g["bref"], 0.0)), ops[f"{k}_stress_ginf0"])
    eq(ops[f"{k}_stress_ginf0"], ops[f"{k}_stress"])


def test_zero_d_runs_bitwise(ops):
    for n, (b, Lc, tau) in enumerate(V.relaxation_setups()):
        got = NP.ucm_local_step(*b, *Lc, tau, 2e-4, nsteps=2000)
        np.testing.assert_array_equal(np.array(got), ops[f"zero_d{n}"])


@pytest.mark.parametrize("shape", [s for s in V.SHAPES if s != (33, 70)], ids=V.key)
def test_transcendental_operators_within_bars(ops, shape):
    g, k = V.op_inputs(shape), V.key(shape)
    psi, Lc = g["psi"], g["L"]
    _close(NP.sym_log(*g["b"]), ops[f"{k}_sym_log"], "sym_log")
    _close(NP.sym_exp(*psi), ops[f"{k}_sym_exp"], "sym_exp")
    _close(NP.logconf_local_rhs(*psi, *Lc, V.TAU), ops[f"{k}_logconf_rhs"], "logconf_rhs")
    _close(NP.logconf_local_step(*psi, *Lc, V.TAU, V.DT), ops[f"{k}_step_explicit"],
           "step_explicit")
    _close(NP.logconf_local_step_strang(*psi, *Lc, V.TAU, V.DT), ops[f"{k}_step_strang"],
           "step_strang")
    _close(NP.relax_exact(*psi, V.TAU, V.DT), ops[f"{k}_relax_exact"], "relax_exact")


def test_special_values(ops):
    s = V.special_inputs()
    with np.errstate(all="ignore"):
        _close(NP.sym_log(*s["neg"]), ops["special_sym_log"], "special_sym_log")
        _close(NP.sym_exp(*s["psi"]), ops["special_sym_exp"], "special_sym_exp")
        _close(NP.logconf_local_rhs(*s["psi"], *s["L"], V.TAU), ops["special_rhs"], "special_rhs")
        _close(NP.logconf_local_step(*s["psi"], *s["L"], V.TAU, V.DT),
               ops["special_step_explicit"], "special_step_explicit")
        _close(NP.logconf_local_step_strang(*s["psi"], *s["L"], V.TAU, V.DT),
               ops["special_step_strang"], "special_step_strang")
    # what the cells are there for: the NaN comes out of the maximums, theta = +-pi/2, the clamp
    r = ops["special_rhs"]
    assert np.isnan(r[:, 3]).all() and np.isnan(r[:, 4]).all() and np.isfinite(r[:, :3]).all()
    l1, l2, th = NP.eig2(*s["psi"])
    assert th[0] == 0.0 and th[1] == 0.5 * np.pi and th[2] == -0.5 * np.pi
    assert l1[5] == 800.0     # exp overflows for certain, far from where an ulp decides
    assert (NP.eig2(*s["neg"])[1][:2] < 0).all()
    assert ops["special_sym_log"][2, 1] != 0.0 and np.isfinite(ops["special_sym_log"]).all()


@pytest.mark.parametrize("gap", V.GAPS, ids=lambda g: f"{g:g}")
def test_gap_ladder(ops, gap):
    """Every cell lies on its rung's side of the `deg` threshold, at least a factor 3 from it,
    by construction (nothing is masked); the right-hand side within the rung's own bar."""
    g = V.gap_inputs(gap)
    lg = NP.lam_gap(*g["psi"])
    assert lg.size == 32
    if gap >= 3e-10:
        assert (lg >= 3e-10).all() and (lg <= 1.2 * gap).all(), (lg.min(), lg.max())
    else:
        assert (lg <= 3e-11).all(), lg.max()
    _close(NP.logconf_local_rhs(*g["psi"], *g["L"], V.TAU), ops[f"gap_{gap:g}"], f"gap_{gap:g}")


@pytest.mark.parametrize("N", V.TG_N)
def test_taylor_green_runs(ops, N):
    """The fields within their bars, and no right-hand side of any run sees a cell near the
    `deg` threshold 1e-10: |lam2 - lam1| is below 1e-13 or at least 1e-4 in every step.  (At
    N = 16 the small class is exactly 0, the initial state.  At N = 33 row and column 16 sit
    at x = pi to rounding, where sin(x) = 1.2e-16 and not 0: there the stretch is ~1e-16 and
    the gap ~1e-17 throughout, three orders below anything an ulp of exp can move across
    1e-10.)"""
    for tau, dt in V.TG_CASES:
        for strang in (False, True):
            gaps = []
            p = V.tg_run(NP, N, tau, dt, strang, gaps=gaps)
            case = V.tg_key(N, tau, dt, strang)
            _close(p, ops[case], case)
            lg = np.stack(gaps)
            small = lg < 1e-4
            assert (lg[small] < 1e-13).all(), (case, lg[small].max())
            if N == 16:
                assert (lg[small] == 0.0).all() and (lg[0] == 0.0).all()
            assert not small[1:].all()


def test_taylor_green_compare(ops):
    got = V.tg_compare(NP, *V.TG_COMPARE)
    for v, ref, case in zip(got, ops["tg_compare"], ("tg_compare_diff",
                                                      "tg_compare_min_eig_explicit",
                                                      "tg_compare_min_eig_strang")):
        _close([np.array([v])], np.array([[ref]]), case)


# ------------------------------------------------------------------ uniform extension --
@pytest.fixture(scope="module")
def loops(oracle, uni):
    """Each run asks for more steps than fit: t_end ends it, with a clipped twelfth step."""
    return {tau: V.UniformLoop(oracle, NP, tau=tau).step(V.UNI_STEPS + 5,
                                                         float(uni[f"tau{tau:g}_t_end"]))
            for tau in V.UNI_TAUS}


@pytest.mark.parametrize("tau", V.UNI_TAUS, ids=lambda t: f"tau{t:g}")
def test_uniform_loop_against_the_reference(uni, loops, tau):
    sim, k = loops[tau], f"tau{tau:g}_"
    rec, ref = np.array(sim.record), uni[k + "record"]
    assert len(rec) == V.UNI_STEPS == int(uni["steps"])
    np.testing.assert_array_equal(np.array(sim.dts), uni[k + "dts"])
    np.testing.assert_array_equal(rec[:, 0], ref[:, 0])
    np.testing.assert_array_equal(rec[:, 3], ref[:, 3])
    assert sim.dts[-1] < 0.75 * sim.dts[0] and not sim.t < float(uni[k + "t_end"])
    c = f"uni_tau{tau:g}_"
    # (the velocity is imposed: no transcendental reaches the maps, so they are an == case)
    np.testing.assert_array_equal(sim.X1, uni[k + "X1"])
    np.testing.assert_array_equal(sim.X2, uni[k + "X2"])
    _close(sim.psi, uni[k + "psi"], c + "psi")
    _close(sim.be, uni[k + "be"], c + "be")
    _close([rec[:, 1]], ref[None, :, 1], c + "lam")
    _close([rec[:, 2]], ref[None, :, 2], c + "bxx")
    np.testing.assert_array_equal(sim.phi, uni[k + "phi"])
    # no cell can change side under rounding-level differences; every step has solid cells
    assert sim.min_abs_phi >= 1e-6, sim.min_abs_phi
    assert (rec[:, 3] > 0).all() and not sim.stopped


def test_uniform_loop_probe(oracle):
    """N = 32, 40 steps at tau = 0.5: finite, 52 solid cells, |phi| never below 1e-6, and
    b_xx(centre) on the stagnation point's analytic 2 - e^{-t} (eps = tau = 0.5)."""
    sim = V.UniformLoop(oracle, NP, tau=0.5).step(40)
    rec = np.array(sim.record)
    assert len(rec) == 40 and np.isfinite(rec).all()
    assert (rec[:, 3] >= 48).all() and rec[-1, 3] == 52     # (the count moves between 48 and 56)
    print(f"min|phi| {sim.min_abs_phi:.3e}, b_xx(c) {rec[-1, 2]:.6f}, analytic "
          f"{2.0 - np.exp(-sim.t):.6f}")
    assert sim.min_abs_phi >= 1e-6
    assert np.abs(rec[:, 2] - (2.0 - np.exp(-rec[:, 0]))).max() <= 1e-3
