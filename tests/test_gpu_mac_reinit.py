"""GPU parity of reference-map reinitialisation with stored deformation (mac_reinit.hip,
pyrmt_amd.mac.MacReinitDisc) against the reference's benchmarks/mac_reinit_test.py
(tests/golden/mac_reinit_trace32.npz, mac_reinit_ops.npz; inputs of the operator cases from
tests/mac_reinit_np.py).

Bars: bit-exact for everything without a transcendental function (the multi-plane advection,
J_ep, Ftot, the distortion reduction, the maps / Fs / phiref of a step, the fused force against
its own unfused composition); S, behind smoothed_heaviside's device sine, to 1e-14 absolute
(test_gpu_parity.py's bar for such outputs); a step's u, v to 1e-12 (test_mac_projection); the
60-step run to rtol 1e-9 on the trace and atol 1e-9 on the fields (test_mac_multi_disc_trace),
its reinitialisation steps exactly.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden
import mac_reinit_np as NP
from mac_faces_np import faces_of_stress

pytestmark = pytest.mark.gpu

CASES = [NP.key(s) for s in NP.SHAPES]


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


@pytest.fixture(scope="module")
def ops():
    return golden("mac_reinit_ops")


@pytest.fixture(scope="module")
def trace():
    return golden("mac_reinit_trace32")


def _inputs(name, ops):
    """(X1, X2, Fs, phi, dx, dy, w_t, mu_s, fixture prefix) of an operator case."""
    if name == "s40":
        dx = float(ops["s40_dx"])
        return (ops["s40_X1"], ops["s40_X2"], list(ops["s40_Fs"]), ops["s40_phi"], dx, dx, 2.0 * dx,
                0.3)
    g = NP.op_inputs(NP.SHAPES[CASES.index(name)])
    return g["X1"], g["X2"], g["Fs"], g["phi"], g["dx"], g["dy"], g["w_t"], NP.MU_S


def _single_plane(gpu, q, g, masked):
    """The parent's path for one plane: rmt_advect_sl_rk4, then rmt_mask_solid."""
    import torch
    from pyrmt_amd import _lib as L, functions as F
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = gpu.advect_semilagrangian_rk4(dev(q), dev(g["a"]), dev(g["b"]), dev(g["Xg"]), dev(g["Yg"]),
                                        NP.ADV_DT, g["dx"], g["dy"])
    if masked:
        phi = dev(g["phi"])
        L.check(L.lib().rmt_mask_solid(F.ctx_for(*q.shape).bind(), F._p(out), F._p(phi), F._p(out)),
                "rmt_mask_solid")
    return out.cpu().numpy()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_multi_plane_advection_bitwise(gpu, ops, name, masked):
    g = NP.op_inputs(NP.SHAPES[CASES.index(name)])
    single = [_single_plane(gpu, q, g, masked) for q in g["q"]]
    for n in (1, 2, 6, 8):
        got = gpu.advect_reference_maps(g["q"][:n], g["a"], g["b"], g["Xg"], g["Yg"], NP.ADV_DT,
                                        g["dx"], g["dy"], phi=g["phi"] if masked else None)
        assert len(got) == n
        for k in range(n):
            np.testing.assert_array_equal(got[k], single[k], err_msg=f"{n} planes, plane {k}")
    if masked:
        np.testing.assert_array_equal(np.stack(got), ops[f"{name}_advm"])
        assert np.signbit(got[7][g["phi"] > 0]).any() and np.isnan(got[3]).any()
    else:
        for row, k in enumerate(ops[f"{name}_adv_planes"]):
            np.testing.assert_array_equal(got[k], ops[f"{name}_adv"][row])


def test_multi_plane_advection_guards(gpu):
    g = NP.op_inputs((9, 9))
    args = (g["Xg"], g["Yg"], NP.ADV_DT, g["dx"], g["dy"])
    with pytest.raises(ValueError):
        gpu.advect_reference_maps([g["q"][0]] * 9, g["a"], g["b"], *args)
    with pytest.raises(ValueError):
        gpu.advect_reference_maps([], g["a"], g["b"], *args)
    a = g["a"].copy(); a[4, 4] = np.inf
    with pytest.raises(FloatingPointError, match="non-finite velocity"):
        gpu.advect_reference_maps(g["q"][:2], a, g["b"], *args)
    # an output plane that is an input plane is refused by the library
    import torch
    from pyrmt_amd import functions as F
    q = torch.from_numpy(g["q"][0]).cuda()
    d = [torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("a", "b", "Xg", "Yg")]
    with pytest.raises(ValueError, match="output plane"):
        F._advect_sl_rk4_multi(F.ctx_for(9, 9), [q], *d, NP.ADV_DT, g["dx"], g["dy"], None, [q])


@pytest.mark.parametrize("name", CASES + ["s40"])
def test_total_stress(M, ops, name):
    X1, X2, Fs, phi, dx, dy, w_t, mu_s = _inputs(name, ops)
    Sxx, Sxy, Syy, J, Ft = M.total_stress(X1, X2, Fs, phi, dx, dy, w_t, mu_s, with_Ftot=True)
    np.testing.assert_array_equal(J, ops[f"{name}_J"])
    np.testing.assert_array_equal(np.stack(Ft), ops[f"{name}_Ftot"])
    # S = (1 - H) mu_s b: device sin against glibc's sin
    np.testing.assert_allclose(np.stack([Sxx, Sxy, Syy]), ops[f"{name}_S"], rtol=0, atol=1e-14)
    # without Ftot: the same four planes
    for a, b in zip(M.total_stress(X1, X2, Fs, phi, dx, dy, w_t, mu_s), (Sxx, Sxy, Syy, J)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", CASES + ["s40"])
def test_total_force_equals_its_unfused_composition(gpu, M, ops, name):
    import torch
    X1, X2, Fs, phi, dx, dy, w_t, mu_s = _inputs(name, ops)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    X1, X2, phi = dev(X1), dev(X2), dev(phi)
    Fs = [dev(p) for p in Fs]
    fu, fv, J = M.total_force(X1, X2, Fs, phi, dx, dy, w_t, mu_s)
    Sxx, Sxy, Syy, J0 = M.total_stress(X1, X2, Fs, phi, dx, dy, w_t, mu_s)
    fu0, fv0 = faces_of_stress(gpu, Sxx, Sxy, Syy, dx, dy)
    np.testing.assert_array_equal(fu.cpu().numpy(), fu0.cpu().numpy())
    np.testing.assert_array_equal(fv.cpu().numpy(), fv0.cpu().numpy())
    np.testing.assert_array_equal(J.cpu().numpy(), J0.cpu().numpy())
    np.testing.assert_array_equal(J.cpu().numpy(), ops[f"{name}_J"])
    # against the reference: S to 1e-14 (above), a one-sided difference sums (3 + 4 + 1) S over
    # 2 h, a divergence two of them, a face the mean of two divergences
    tol = 2 * 8 * 1e-14 / (2 * min(dx, dy))
    np.testing.assert_allclose(fu.cpu().numpy(), ops[f"{name}_fu"], rtol=0, atol=tol)
    np.testing.assert_allclose(fv.cpu().numpy(), ops[f"{name}_fv"], rtol=0, atol=tol)


@pytest.mark.parametrize("name", CASES + ["s40"])
def test_epoch_distortion_bitwise(M, ops, name):
    phi = _inputs(name, ops)[3]
    np.testing.assert_array_equal(M.epoch_distortion(ops[f"{name}_J"], phi), ops[f"{name}_dist"])


def test_epoch_distortion_edge_cases(M):
    J = np.full((9, 12), 2.0); phi = np.ones((9, 12))
    np.testing.assert_array_equal(M.epoch_distortion(J, phi), [-np.inf, np.inf, 0.0])
    phi[3, 4] = 0.0; phi[8, 11] = -1.0; J[8, 11] = np.nan
    out = M.epoch_distortion(J, phi)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 2.0


def _state(trace, tag):
    return {k: trace[f"{tag}_{k}"] for k in ("u", "v", "X1", "X2", "Fs", "phiref")}


def _sim(M, trace, **kw):
    return M.MacReinitDisc(int(trace["N"]), reinit_J=float(trace["reinit_J"]),
                           mu_s=float(trace["mu_s"]), mu_f=float(trace["mu_f"]),
                           rho=float(trace["rho"]), U_lid=float(trace["U_lid"]), **kw)


@pytest.mark.parametrize("k", [26, 40, 53])
def test_one_step_from_captured_state(M, trace, k):
    rec = trace["record"]
    sim = _sim(M, trace)
    assert sim.dt == float(trace["dt"])
    sim.set_state(dict(_state(trace, f"before{k}"), t=rec[k - 2, 0], n_reinit=int(rec[k - 2, 4])))
    sim.step(1)
    s = sim.state()
    assert s["n_reinit"] == int(rec[k - 1, 4]) and s["t"] == rec[k - 1, 0]
    assert (s["n_reinit"] - int(rec[k - 2, 4])) == (1 if k in (26, 53) else 0)
    for name in ("X1", "X2", "Fs", "phiref"):
        np.testing.assert_array_equal(s[name], trace[f"after{k}_{name}"], err_msg=name)
    np.testing.assert_allclose(s["u"], trace[f"after{k}_u"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(s["v"], trace[f"after{k}_v"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(sim.get("phi"), trace[f"after{k}_phi"])
    r = sim.record[-1]
    np.testing.assert_allclose(r[1:4], rec[k - 1, 1:4], rtol=1e-13)   # J_ep is bit-exact
    np.testing.assert_allclose(r[5], rec[k - 1, 5], rtol=0, atol=1e-12)


@pytest.fixture(scope="module")
def run60(M, trace):
    sim = _sim(M, trace)
    sim.step(60)
    return sim


def test_run_start_is_the_reference_start(M, trace):
    s = _sim(M, trace).state()
    # (before step 26 nothing was stored: phiref is still the analytic disc of the start)
    np.testing.assert_array_equal(s["phiref"], trace["before26_phiref"])
    one, zero = np.ones_like(s["X1"]), np.zeros_like(s["X1"])
    np.testing.assert_array_equal(s["Fs"], np.stack([one, zero, zero, one]))
    assert s["t"] == 0.0 and s["n_reinit"] == 0 and not s["u"].any() and not s["v"].any()


def test_run_reinitialises_at_the_reference_steps(run60):
    assert run60.nsteps == 60 and not run60.diverged
    assert run60.reinit_steps == [26, 53]
    assert [r[4] for r in run60.record] == [0] * 25 + [1] * 27 + [2] * 8


def test_run_trace(run60, trace):
    rec = trace["record"][:60]
    got = np.array(run60.record)
    np.testing.assert_allclose(got[:, 0], rec[:, 0], rtol=1e-15)
    for col, what in ((1, "dist"), (2, "minJ_ep"), (3, "maxJ_ep")):
        err = np.abs(got[:, col] / rec[:, col] - 1).max()
        print(f"60-step drift, {what}: max relative {err:.3e}")
        np.testing.assert_allclose(got[:, col], rec[:, col], rtol=1e-9, err_msg=what)


def test_run_final_fields(run60, trace):
    s = run60.state()
    for name in ("u", "v", "X1", "X2", "Fs", "phiref"):
        err = np.abs(s[name] - trace[f"after60_{name}"]).max()
        print(f"60-step drift, {name}: max abs {err:.3e}")
        np.testing.assert_allclose(s[name], trace[f"after60_{name}"], rtol=0, atol=1e-9,
                                   err_msg=name)


def test_t_end_inside_a_step_clips_dt(M, trace):
    rec = trace["record"]
    sim = _sim(M, trace)
    sim.set_state(dict(_state(trace, "after60"), t=rec[59, 0], n_reinit=2))
    sim.step(5, t_end=float(trace["t_end"]))
    assert sim.nsteps == 1 and sim.t == rec[60, 0]
    np.testing.assert_allclose(sim.record[-1][1:4], rec[60, 1:4], rtol=1e-9)
    sim.step(5, t_end=float(trace["t_end"]))
    assert sim.nsteps == 1


def test_without_reinit_the_loop_is_the_same_until_the_first_one(M, run60, trace):
    sim = _sim(M, trace, reinit=False)
    sim.step(30)
    assert all(r[4] == 0 for r in sim.record) and sim.n_reinit == 0 and sim.reinit_steps == []
    np.testing.assert_array_equal(np.array(sim.record[:25]), np.array(run60.record[:25]))
    # step 26: the same step, but nothing is reset; afterwards the runs differ
    assert sim.record[25][1] == run60.record[25][1] > float(trace["reinit_J"])
    assert sim.record[29][1] > run60.record[29][1]


def test_mac_reinit_run_returns_the_time_reached(M, trace):
    dt = float(trace["dt"])
    t, sim = M.mac_reinit_run(int(trace["N"]), 3.5 * dt, reinit_J=float(trace["reinit_J"]),
                              return_sim=True)
    assert sim.nsteps >= 4 and t == sim.t and abs(t - 3.5 * dt) < 1e-15
    np.testing.assert_array_equal([r[0] for r in sim.record[:3]], trace["record"][:3, 0])
    assert M.mac_reinit_run(int(trace["N"]), 2 * dt, reinit=False) == trace["record"][1, 0]


def test_state_round_trip_and_set_state_contract(M):
    """state() -> a fresh sim -> set_state -> state() holds every bit, from a step after a
    reinitialisation (Fs != I, phiref stored); set_state's refusals, its copy of what it is given,
    and its clearing of the `diverged` stop."""
    import torch
    N = 32
    sim = M.MacReinitDisc(N, reinit_J=1.02)
    while sim.n_reinit == 0 and sim.nsteps < 30:
        sim.step(1)
    assert sim.n_reinit == 1 and not sim.diverged
    sim.step(1)
    s = sim.state()
    assert tuple(s) == M.MacReinitDisc.STATE
    fresh = M.MacReinitDisc(N, reinit_J=1.02)
    s0 = fresh.state()
    assert not np.array_equal(s["Fs"], s0["Fs"]) and not np.array_equal(s["phiref"], s0["phiref"])
    fresh.set_state(s)
    s1 = fresh.state()
    for k in M.MacReinitDisc.STATE:
        np.testing.assert_array_equal(s1[k], s[k], err_msg=k)
    assert type(s1["n_reinit"]) is int and s1["n_reinit"] == 1 and type(s1["t"]) is float
    # the state is all a step reads: both sims take the same next step
    sim.step(1); fresh.step(1)
    assert fresh.record[-1] == sim.record[-1]
    for k, a in fresh.state().items():
        np.testing.assert_array_equal(a, sim.state()[k], err_msg=k)
    # refusals
    with pytest.raises(KeyError, match="unknown fields"):
        fresh.set_state({"w": s["u"]})
    with pytest.raises(ValueError, match="u has shape"):
        fresh.set_state({"u": s["u"][:, :-1]})
    with pytest.raises(ValueError, match="Fs has shape"):
        fresh.set_state({"Fs": s["Fs"][:3]})
    # what it is given is copied, not kept
    u_dev, Fs_dev = torch.from_numpy(s["u"]).cuda(), torch.from_numpy(s["Fs"]).cuda()
    u_keep, Fs_keep = u_dev.clone(), Fs_dev.clone()
    fresh.set_state({"u": u_dev, "Fs": Fs_dev})
    assert fresh.u.data_ptr() != u_dev.data_ptr() and fresh.Fs[0].data_ptr() != Fs_dev.data_ptr()
    fresh.step(1)
    assert torch.equal(u_dev, u_keep) and torch.equal(Fs_dev, Fs_keep)
    # a `diverged` stop (no solid cell left: a stored level set that is positive everywhere),
    # cleared by set_state
    fresh.set_state(dict(s, phiref=np.ones((N, N))))
    fresh.step(3)
    n = fresh.nsteps
    assert fresh.diverged and fresh.record[-1][1] == np.inf
    fresh.step(3)
    assert fresh.nsteps == n
    fresh.set_state(s)
    assert not fresh.diverged
    fresh.step(1)
    assert fresh.nsteps == n + 1 and not fresh.diverged and fresh.t > s["t"]
