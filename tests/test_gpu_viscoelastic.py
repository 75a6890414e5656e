"""GPU parity of the viscoelastic constitutive layer (viscoelastic.hip, pyrmt_amd.viscoelastic)
against the reference's pyRMT/viscoelastic.py and its three stand-alone drivers
(tests/golden/viscoelastic_ops.npz, viscoelastic_uniform32.npz; where a shape is not in the
fixture, the NumPy restatement tests/viscoelastic_np.py, which test_viscoelastic_cpu.py pins to
the reference).

Bars: == for ucm_*, viscoelastic_stress, the fused 0-D runs, the reduction, the uniform loop's
maps, t and dt (arithmetic and sqrt only); == between one fused launch and single calls, Strang
and explicit at tau = inf, relax_exact's identity cases; every case behind exp / log / sin /
cos / atan2 within viscoelastic_np.bar(case) = 4 x its measured noise floor
(profiles/viscoelastic/floor.json), printed before it is asserted.
"""
import ctypes
import math

import numpy as np
import pytest

from conftest import golden
import viscoelastic_np as V

pytestmark = pytest.mark.gpu

NP, close, same_bits = V.NP, V.assert_close, V.same_bits
ALL = V.SHAPES + ((V.LONG_N,),)
eq = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def VE(gpu):
    from pyrmt_amd import viscoelastic
    return viscoelastic


@pytest.fixture(scope="module")
def ops():
    return golden("viscoelastic_ops")


@pytest.fixture(scope="module")
def uni():
    return golden("viscoelastic_uniform32")


def _ref(ops, shape, name, compute):
    """The fixture's entry of a shape, or the restatement where it holds none."""
    k = f"{V.key(shape)}_{name}"
    return ops[k] if k in ops.files else np.stack(compute())


def test_long_n_reaches_the_second_trip(gpu):
    """LONG_N's last cell is the first one of a second grid-stride trip; the smaller shapes
    take one trip in one to ten workgroups."""
    from pyrmt_amd import _lib as L
    b, t = ctypes.c_int(), ctypes.c_int()
    L.check(L.lib().rmt_ve_launch_shape(V.LONG_N, ctypes.byref(b), ctypes.byref(t)))
    assert (b.value, t.value) == (V.VE_MAXB, V.VE_T) and b.value * t.value == V.LONG_N - 1
    L.check(L.lib().rmt_ve_launch_shape(33 * 70, ctypes.byref(b), ctypes.byref(t)))
    assert b.value == 10 and b.value * t.value >= 33 * 70
    L.check(L.lib().rmt_ve_launch_shape(1, ctypes.byref(b), ctypes.byref(t)))
    assert b.value == 1


# ------------------------------------------------------------------ bit-exact cases --
@pytest.mark.parametrize("shape", ALL, ids=V.key)
def test_arithmetic_operators_bitwise(VE, ops, shape):
    g = V.op_inputs(shape)
    b, Lc, bref = g["b"], g["L"], g["bref"]
    for name, got, compute in (
            ("ucm_step", VE.ucm_local_step(*b, *Lc, V.TAU, V.DT),
             lambda: NP.ucm_local_step(*b, *Lc, V.TAU, V.DT)),
            ("ucm_step_inf", VE.ucm_local_step(*b, *Lc, V.INF, V.DT),
             lambda: NP.ucm_local_step(*b, *Lc, V.INF, V.DT)),
            ("ucm_rhs", VE.ucm_local_rhs(*b, *Lc, V.TAU), lambda: NP.ucm_local_rhs(*b, *Lc, V.TAU)),
            ("stress", VE.viscoelastic_stress(*b, V.G), lambda: NP.viscoelastic_stress(*b, V.G)),
            ("stress_zener", VE.viscoelastic_stress(*b, V.G, bref, V.G_INF),
             lambda: NP.viscoelastic_stress(*b, V.G, bref, V.G_INF)),
            ("stress_ginf0", VE.viscoelastic_stress(*b, V.G, bref, 0.0),
             lambda: NP.viscoelastic_stress(*b, V.G))):
        assert isinstance(got[0], np.ndarray) and got[0].shape == tuple(shape)
        assert same_bits(np.stack(got), _ref(ops, shape, name, compute)), name


def test_zero_d_fused_runs_bitwise(VE, ops):
    """2000 fused steps of the three 0-D set-ups, scalars in and floats out."""
    for n, (b, Lc, tau) in enumerate(V.relaxation_setups()):
        got = VE.ucm_local_step(*b, *Lc, tau, 2e-4, nsteps=2000)
        assert all(type(v) is float for v in got)
        eq(np.array(got), ops[f"zero_d{n}"])
        eq(np.array(got), np.array(NP.ucm_local_step(*b, *Lc, tau, 2e-4, nsteps=2000)))


def test_relaxation_driver(VE, ops):
    """The 0-D driver's three errors: its own pass marks, and the reference's values (the
    steady-shear and elastic-limit errors are arithmetic only; the relaxation error compares
    with exp(-t / tau), evaluated by NumPy's array loop here and its scalar there)."""
    e1, e2, e3 = VE.relaxation_tests()
    print(f"relaxation_tests: {e1:.6e} {e2:.6e} {e3:.6e}; reference {ops['relaxation']}")
    assert e1 < 1e-3 and e2 < 1e-3 and e3 < 1e-6
    assert (e2, e3) == tuple(ops["relaxation"][1:])
    assert abs(e1 - ops["relaxation"][0]) <= 4 * np.finfo(float).eps


# ------------------------------------------------------------------ same-bits cases --
@pytest.mark.parametrize("shape", [(65,), (33, 70)], ids=V.key)
def test_fused_steps_are_single_steps(VE, shape):
    import torch
    g = V.op_inputs(shape)
    dev = lambda ps: [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in ps]
    psi, b, Lc = dev(g["psi"]), dev(g["b"]), dev(g["L"])
    for step, s0, case in ((VE.ucm_local_step, b, None),
                           (VE.logconf_local_step, psi, "step7_explicit"),
                           (VE.logconf_local_step_strang, psi, "step7_strang")):
        fused = step(*s0, *Lc, V.TAU, V.DT, nsteps=7)
        s = s0
        for _ in range(7):
            s = step(*s, *Lc, V.TAU, V.DT)
        assert all(isinstance(p, torch.Tensor) and p.is_cuda for p in fused)
        for a, c in zip(fused, s):
            assert same_bits(a.cpu().numpy(), c.cpu().numpy()), step.__name__
        host = [p.cpu().numpy() for p in fused]
        if case is None:
            assert same_bits(np.stack(host), np.stack(NP.ucm_local_step(*g["b"], *g["L"], V.TAU,
                                                                        V.DT, nsteps=7)))
        else:
            close(host, np.stack(NP.stepper(case.endswith("strang"))(*g["psi"], *g["L"], V.TAU,
                                                                     V.DT, nsteps=7)), case)


@pytest.mark.parametrize("shape", [(64,), (9, 9)], ids=V.key)
def test_strang_at_tau_inf_is_the_explicit_step(VE, shape):
    g = V.op_inputs(shape)
    for nsteps in (1, 3):
        a = VE.logconf_local_step_strang(*g["psi"], *g["L"], V.INF, V.DT, nsteps=nsteps)
        b = VE.logconf_local_step(*g["psi"], *g["L"], V.INF, V.DT, nsteps=nsteps)
        assert same_bits(np.stack(a), np.stack(b))


def test_relax_exact_identity_cases(VE):
    """dt = 0.0 or tau = inf: the input's bits, for the special cells (NaN, inf, -0.0) and a
    tensor that is no log of an SPD one as well."""
    s = V.special_inputs()
    for psi in (s["psi"], s["neg"], V.op_inputs((33, 70))["psi"]):
        for tau, dt in ((V.TAU, 0.0), (V.INF, V.DT), (V.INF, 0.0)):
            got = VE.relax_exact(*psi, tau, dt)
            assert same_bits(np.stack(got), np.stack(psi)), (tau, dt)
    assert VE.relax_exact(0.25, -0.0, 0.5, V.INF, 0.1) == (0.25, 0.0, 0.5)
    assert math.copysign(1.0, VE.relax_exact(0.25, -0.0, 0.5, 0.5, 0.0)[1]) == -1.0


# ------------------------------------------------------------ transcendental operators --
@pytest.mark.parametrize("shape", ALL, ids=V.key)
def test_transcendental_operators_within_bars(VE, ops, shape):
    g = V.op_inputs(shape)
    psi, Lc, b = g["psi"], g["L"], g["b"]
    for case, got, compute in (
            ("sym_log", VE.sym_log(*b), lambda: NP.sym_log(*b)),
            ("sym_exp", VE.sym_exp(*psi), lambda: NP.sym_exp(*psi)),
            ("logconf_rhs", VE.logconf_local_rhs(*psi, *Lc, V.TAU),
             lambda: NP.logconf_local_rhs(*psi, *Lc, V.TAU)),
            ("step_explicit", VE.logconf_local_step(*psi, *Lc, V.TAU, V.DT),
             lambda: NP.logconf_local_step(*psi, *Lc, V.TAU, V.DT)),
            ("step_strang", VE.logconf_local_step_strang(*psi, *Lc, V.TAU, V.DT),
             lambda: NP.logconf_local_step_strang(*psi, *Lc, V.TAU, V.DT)),
            ("relax_exact", VE.relax_exact(*psi, V.TAU, V.DT),
             lambda: NP.relax_exact(*psi, V.TAU, V.DT))):
        assert got[0].shape == tuple(shape)
        close(got, _ref(ops, shape, case, compute), case, f"{V.key(shape)} {case}")


def test_scalars_broadcast(VE):
    """Scalar operands beside arrays are broadcast by the shim: the bits of full planes."""
    g = V.op_inputs((9, 9))
    full = [np.full((9, 9), v) for v in (0.25, -0.5, 0.375, -0.25)]
    a = VE.logconf_local_step(*g["psi"], 0.25, -0.5, 0.375, -0.25, V.TAU, V.DT)
    b = VE.logconf_local_step(*g["psi"], *full, V.TAU, V.DT)
    assert same_bits(np.stack(a), np.stack(b))
    a = VE.sym_exp(0.5, g["psi"][1], -0.25)
    b = VE.sym_exp(np.full((9, 9), 0.5), g["psi"][1], np.full((9, 9), -0.25))
    assert same_bits(np.stack(a), np.stack(b))
    got = VE.sym_exp(0.0, 0.0, 0.0)
    assert got == (1.0, 0.0, 1.0) and all(type(v) is float for v in got)


def test_special_values(VE, ops):
    s = V.special_inputs()
    psi, Lc = s["psi"], s["L"]
    close(VE.sym_log(*s["neg"]), ops["special_sym_log"], "special_sym_log")
    close(VE.sym_exp(*psi), ops["special_sym_exp"], "special_sym_exp")
    close(VE.logconf_local_rhs(*psi, *Lc, V.TAU), ops["special_rhs"], "special_rhs")
    close(VE.logconf_local_step(*psi, *Lc, V.TAU, V.DT), ops["special_step_explicit"],
          "special_step_explicit")
    close(VE.logconf_local_step_strang(*psi, *Lc, V.TAU, V.DT), ops["special_step_strang"],
          "special_step_strang")
    r = np.stack(VE.logconf_local_rhs(*psi, *Lc, V.TAU))
    assert np.isnan(r[:, 3]).all() and np.isnan(r[:, 4]).all()     # out of the maximums


@pytest.mark.parametrize("gap", V.GAPS, ids=lambda g: f"{g:g}")
def test_gap_ladder(VE, ops, gap):
    g = V.gap_inputs(gap)
    close(VE.logconf_local_rhs(*g["psi"], *g["L"], V.TAU), ops[f"gap_{gap:g}"], f"gap_{gap:g}")


# ---------------------------------------------------------------------- Taylor-Green --
@pytest.mark.parametrize("N", V.TG_N)
def test_taylor_green_fields(VE, ops, N):
    """50 steps from psi = 0 under the frozen gradient, fused, both steppers."""
    Lc = V.tg_velocity_gradient(N)
    z = np.zeros((N, N))
    for tau, dt in V.TG_CASES:
        for strang, step in ((False, VE.logconf_local_step), (True, VE.logconf_local_step_strang)):
            case = V.tg_key(N, tau, dt, strang)
            close(step(z, z, z, *Lc, tau, dt, nsteps=V.TG_STEPS), ops[case], case)


def test_taylor_green_compare(VE, ops):
    got = VE.tg_run_compare(*V.TG_COMPARE)
    for v, ref, case in zip(got, ops["tg_compare"], ("tg_compare_diff",
                                                      "tg_compare_min_eig_explicit",
                                                      "tg_compare_min_eig_strang")):
        close([np.array([v])], np.array([[ref]]), case)


# ------------------------------------------------------------------------- reduction --
def _lam_case(VE, b, phi, at=0):
    got = VE.lam_max(*b, phi, at=at)
    assert isinstance(got, np.ndarray) and got.shape == (3,)
    with np.errstate(invalid="ignore"):
        lam = V.lam_max_plane(*b)          # (*, + and sqrt: NumPy holds the device's plane)
    sm = phi <= 0
    want = lam[sm].max() if sm.any() else -np.inf
    assert np.isnan(got[0]) if np.isnan(want) else got[0] == want, (got[0], want)
    assert got[1] == sm.sum() and got[2] == np.ravel(b[0])[at]
    return got


def test_lam_max_one_item_at_a_time(VE):
    n = V.LAM_TRIP + 77
    g = V.op_inputs((n,))
    base = [p.copy() for p in g["b"]]
    off = np.ones(n)
    spots = dict(first=0, last=n - 1, second_trip=V.LAM_TRIP + 5, wave_edge=64)
    for name, k in spots.items():
        b = [p.copy() for p in base]
        b[0][k] = 50.0
        phi = off.copy(); phi[k] = -0.25                      # the mask is this one cell
        got = _lam_case(VE, b, phi, at=k)
        assert got[1] == 1 and got[0] > 40.0, name
        phi = -off                                            # ... and every cell
        assert _lam_case(VE, b, phi, at=n - 1)[0] == got[0], name
    # phi == 0 counts as solid; a mask of several cells on both trips
    phi = off.copy(); phi[[3, 700, V.LAM_TRIP + 9]] = (0.0, -0.0, -1e-300)
    assert _lam_case(VE, base, phi)[1] == 3
    # a NaN inside the mask comes out, one outside does not
    for k in spots.values():
        b = [p.copy() for p in base]
        b[1][k] = np.nan
        phi = -off
        assert np.isnan(_lam_case(VE, b, phi)[0])
        phi = -off; phi[k] = 0.5
        assert np.isfinite(_lam_case(VE, b, phi)[0])
    # an empty mask: -inf and 0
    got = _lam_case(VE, base, off)
    assert got[0] == -np.inf and got[1] == 0
    # the shapes of the elementwise cases
    for shape in ((1,), (63,), (65,), (9, 9), (33, 70)):
        g = V.op_inputs(shape)
        _lam_case(VE, g["b"], g["psi"][1], at=int(np.prod(shape)) - 1)


# ----------------------------------------------------------------- uniform extension --
@pytest.fixture(scope="module")
def runs(VE, uni):
    """Each run asks for more steps than fit: t_end ends it, with a clipped twelfth step."""
    return {tau: VE.UniformExtension(V.UNI_N, tau=(0.0 if tau == V.INF else tau))
            .step(V.UNI_STEPS + 5, float(uni[f"tau{tau:g}_t_end"])) for tau in V.UNI_TAUS}


@pytest.mark.parametrize("tau", V.UNI_TAUS, ids=lambda t: f"tau{t:g}")
def test_uniform_extension_against_the_reference(uni, runs, tau):
    sim, k, c = runs[tau], f"tau{tau:g}_", f"uni_tau{tau:g}_"
    rec, ref = np.array(sim.record), uni[k + "record"]
    assert sim.tau == tau and sim.nsteps == len(rec) == V.UNI_STEPS and not sim.stopped
    eq(np.array(sim.dts), uni[k + "dts"])
    eq(rec[:, 0], ref[:, 0])
    assert sim.t == ref[-1, 0]
    # the velocity is imposed: no transcendental reaches the maps or phi
    eq(sim.get("X1"), uni[k + "X1"])
    eq(sim.get("X2"), uni[k + "X2"])
    eq(sim.get("phi"), uni[k + "phi"])
    close([sim.get(n) for n in ("p11", "p12", "p22")], uni[k + "psi"], c + "psi")
    close([sim.get(n) for n in ("be11", "be12", "be22")], uni[k + "be"], c + "be")
    close([rec[:, 1]], ref[None, :, 1], c + "lam")
    close([rec[:, 2]], ref[None, :, 2], c + "bxx")
    if tau == 0.5:     # the stagnation point's analytic solution for eps = tau = 0.5
        err = np.abs(rec[:, 2] - (2.0 - np.exp(-rec[:, 0]))).max()
        print(f"b_xx(centre) against 2 - exp(-t): {err:.3e}")
        assert err <= 1e-3
    else:              # elastic: e^{2 eps t}
        assert np.abs(rec[:, 2] - np.exp(rec[:, 0])).max() <= 1e-3


def test_uniform_extension_clipping_and_run(VE, uni):
    sim = VE.UniformExtension(V.UNI_N)
    dt = sim.dt
    assert dt == uni["tau0.5_dts"][0]
    sim.step(10, t_end=3.5 * dt)
    t3 = 0.0 + dt + dt + dt
    assert sim.nsteps == 4 and sim.dts == [dt, dt, dt, 3.5 * dt - t3]
    assert sim.t == t3 + (3.5 * dt - t3) and sim.dt == dt
    sim.step(3)                      # nothing is left before no t_end: three full steps
    assert sim.nsteps == 7 and sim.dts[4:] == [dt] * 3
    t, hist, run = VE.ve_uniform_run(V.UNI_N, float(uni["tau0.5_t_end"]), 0.5, return_sim=True)
    assert t == uni["tau0.5_record"][-1, 0] and len(hist) == 1
    assert hist[0][:3] == run.record[-1] and hist[0][3] == run.umax
    with pytest.raises(ValueError):
        VE.ve_uniform_run(V.UNI_N, math.inf)
