"""GPU parity of the soft disc under the integrator ladder (mac_soft.hip,
pyrmt_amd.mac.MacSoftDisc) against the reference's benchmarks/mac_soft_disc_lid.py
(tests/golden/mac_soft_disc.npz, mac_soft_disc_ops.npz; traces and operator inputs from
tests/mac_soft_disc_np.py).

Bars: bit-exact for everything without a transcendental function or a CG (the midpoint centres,
the conservative advection, J, the diagnostics' count, min and max, the fused force against its
own unfused composition); the fused force against the reference to 1e-14 of the blended stress's
amplitude times 8 / min(dx, dy) (test_gpu_mac_reinit.py's derivation); a step's u, v and maps to
1e-12 (test_mac_projection), at kept steps where the reference's own one-ulp response is at most a
tenth of that (tests/mac_soft_disc_np.py, the note at TRACES); the traces to rtol 1e-9 on the record and atol 1e-9 on the fields
(test_mac_multi_disc_trace), t to rtol 1e-15, PCG counts and the semi-Lagrangian branch exactly.
The physics checks are the reference's own (tests/test_imex_wall.py:64-76,
tests/test_elastic_imex_fsi.py:25-36) at its N = 48, on the device path alone.
"""
import numpy as np
import pytest

from conftest import golden
import mac_soft_disc_np as NP
from mac_faces_np import faces_of_stress

pytestmark = pytest.mark.gpu

CASES = [NP.key(s) for s in NP.SHAPES]
VARIANTS = [NP.vkey(*v) for v in NP.FORCE_VARIANTS]
INTEGRATOR = {name: kw["integrator"] for name, (kw, _, _) in NP.TRACES.items()}


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


@pytest.fixture(scope="module")
def fx():
    return golden("mac_soft_disc")


@pytest.fixture(scope="module")
def ops():
    return golden("mac_soft_disc_ops")


def _g(name):
    return NP.op_inputs(NP.SHAPES[CASES.index(name)])


# ---------------------------------------------------------------- operators ----
@pytest.mark.parametrize("name", CASES)
def test_midpoint_centres_bitwise(M, ops, name):
    g = _g(name)
    uc, vc = M.midpoint_centres(g["u0"], g["v0"], g["u1"], g["v1"])
    np.testing.assert_array_equal(uc, ops[f"{name}_umc"])
    np.testing.assert_array_equal(vc, ops[f"{name}_vmc"])
    # u0 is u1: the plain centre average of :82-83
    uc, vc = M.midpoint_centres(g["u0"], g["v0"], g["u0"], g["v0"])
    np.testing.assert_array_equal(uc, 0.5 * (g["u0"][:, :-1] + g["u0"][:, 1:]))
    np.testing.assert_array_equal(vc, 0.5 * (g["v0"][:-1, :] + g["v0"][1:, :]))


@pytest.mark.parametrize("name", CASES)
def test_advect_xi_conservative_bitwise(M, ops, name):
    g = _g(name)
    for w, tag in ((g["w_cut"], "adv"), (0.0, "adv0")):
        out = M.advect_xi_conservative(g["X1"], g["u0"], g["v0"], g["dx"], g["dy"], g["dt"],
                                       g["phi"], w)
        if f"{name}_{tag}" in ops.files:
            np.testing.assert_array_equal(out, ops[f"{name}_{tag}"], err_msg=tag)
        np.testing.assert_array_equal(out, NP.advect_xi_conservative(
            g["X1"], g["u0"], g["v0"], g["dx"], g["dy"], g["dt"], g["phi"], w), err_msg=tag)
        # outside H the flux is switched off: xi but for the rounding of the two convex
        # combinations (0.75 xi + 0.25 xi is not xi in every bit)
        np.testing.assert_allclose(out[g["phi"] > w], g["X1"][g["phi"] > w], rtol=4e-16)


def test_device_tensors_stay_on_the_device(M):
    import torch
    g = _g("6x6")
    d = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda()
         for k in ("X1", "X2", "phi", "u0", "v0")}
    out = M.advect_xi_conservative(d["X1"], d["u0"], d["v0"], g["dx"], g["dy"], g["dt"], d["phi"])
    fu, fv, J = M.solid_force(d["X1"], d["X2"], d["phi"], g["dx"], g["dy"], g["w_t"], NP.MU_S)
    uc, vc = M.midpoint_centres(d["u0"], d["v0"], d["u0"], d["v0"])
    st = M.soft_diag(d["phi"], J, d["u0"], d["v0"], g["dx"], g["dy"])
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (out, fu, fv, J, uc, vc, st))
    assert isinstance(M.solid_force(g["X1"], g["X2"], g["phi"], g["dx"], g["dy"], g["w_t"],
                                    NP.MU_S)[0], np.ndarray)


def test_shape_errors_are_value_errors(M):
    g = _g("6x6")
    with pytest.raises(ValueError):
        M.solid_force(g["X1"], g["X2"][:, :5], g["phi"], g["dx"], g["dy"], g["w_t"], NP.MU_S)
    with pytest.raises(ValueError):
        M.solid_force(g["X1"][:4, :4], g["X2"][:4, :4], g["phi"][:4, :4], g["dx"], g["dy"],
                      g["w_t"], NP.MU_S)
    with pytest.raises(ValueError):
        M.advect_xi_conservative(g["X1"], g["v0"], g["u0"], g["dx"], g["dy"], g["dt"], g["phi"])
    with pytest.raises(ValueError):
        M.midpoint_centres(g["u0"], g["v0"], g["u1"][:, :-1], g["v1"])
    with pytest.raises(ValueError):
        M.soft_diag(g["phi"], g["phi"], g["u0"][:-1], g["v0"], g["dx"], g["dy"])


@pytest.mark.parametrize("var", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_solid_force_equals_its_unfused_composition(gpu, M, ops, name, var):
    import torch
    iso, clamp = NP.FORCE_VARIANTS[VARIANTS.index(var)]
    g = _g(name)
    dx, dy, w_t = g["dx"], g["dy"], g["w_t"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    X1, X2, phi = dev(g["X1"]), dev(g["X2"]), dev(g["phi"])
    fu, fv, J = M.solid_force(X1, X2, phi, dx, dy, w_t, NP.MU_S, NP.KAPPA, clamp, iso)
    sxx, sxy, syy, J0 = gpu.solid_cauchy_stress(X1, X2, dx, dy, NP.MU_S, NP.KAPPA, phi,
                                                detg_clamp=clamp, isochoric=iso)
    H = gpu.smoothed_heaviside(phi, w_t)
    Sxx = (1 - H) * sxx; Sxy = (1 - H) * sxy; Syy = (1 - H) * syy
    fu0, fv0 = faces_of_stress(gpu, Sxx, Sxy, Syy, dx, dy)
    np.testing.assert_array_equal(fu.cpu().numpy(), fu0.cpu().numpy())
    np.testing.assert_array_equal(fv.cpu().numpy(), fv0.cpu().numpy())
    np.testing.assert_array_equal(J.cpu().numpy(), J0.cpu().numpy())
    assert (fu[:, [0, -1]] == 0).all() and (fv[[0, -1], :] == 0).all()
    # against the reference (the variants the fixture holds, NP.stored_variants)
    if f"{name}_{var}_J" not in ops.files:
        assert (iso, clamp) not in NP.stored_variants(phi.shape)
        return
    np.testing.assert_array_equal(J.cpu().numpy(), ops[f"{name}_{var}_J"])
    sbar, fbar = ops[f"{name}_{var}_bars"]
    print(f"{name} {var}: max|dfu| {np.abs(fu.cpu().numpy() - ops[f'{name}_{var}_fu']).max():.3e}, "
          f"max|dfv| {np.abs(fv.cpu().numpy() - ops[f'{name}_{var}_fv']).max():.3e} (bar {fbar:.3e})")
    if f"{name}_{var}_S" in ops.files:
        S = np.stack([t.cpu().numpy() for t in (Sxx, Sxy, Syy)])
        assert (sbar, fbar) == NP.force_bar(ops[f"{name}_{var}_S"], g["phi"], w_t, dx, dy)
        print(f"    max|dS| {np.abs(S - ops[f'{name}_{var}_S']).max():.3e} (bar {sbar:.3e})")
        np.testing.assert_allclose(S, ops[f"{name}_{var}_S"], rtol=0, atol=sbar)
    np.testing.assert_allclose(fu.cpu().numpy(), ops[f"{name}_{var}_fu"], rtol=0, atol=fbar)
    np.testing.assert_allclose(fv.cpu().numpy(), ops[f"{name}_{var}_fv"], rtol=0, atol=fbar)


def test_solid_force_on_a_captured_step(M, fx):
    """The force stage of step 30 of the explicit trace (dx == dy, the driver's own call)."""
    dx = NP.DX
    X1, X2, phi = (fx[f"explicit_after30_{k}"] for k in ("X1", "X2", "phi"))
    fu, fv, J = M.solid_force(X1, X2, phi, dx, dx, 2.0 * dx, 0.1)
    np.testing.assert_array_equal(J, fx["explicit_after30_J"])
    tol = float(fx["explicit_fbar"])
    np.testing.assert_allclose(fu, fx["explicit_fu"], rtol=0, atol=tol)
    np.testing.assert_allclose(fv, fx["explicit_fv"], rtol=0, atol=tol)


def _check_diag(got, ref):
    assert got[0] == ref[0] and got[7] == ref[7]
    np.testing.assert_array_equal(got[3:7], ref[3:7])
    np.testing.assert_allclose(got[1:3], ref[1:3], rtol=1e-13)


@pytest.mark.parametrize("name", CASES)
def test_soft_diag(M, ops, name):
    g = _g(name)
    J = ops[f"{name}_{VARIANTS[0]}_J"]
    got = M.soft_diag(g["phi"], J, g["u0"], g["v0"], g["dx"], g["dy"])
    _check_diag(got, ops[f"{name}_diag"])
    np.testing.assert_allclose(got[1:3] / got[0], ops[f"{name}_centroid"], rtol=1e-13)


def test_soft_diag_edge_cases(M):
    ny, nx, dx, dy = 9, 12, 0.1, 0.125
    J = np.full((ny, nx), 2.0); J[2, 3] = -0.5; J[7, 1] = 21.0
    phi = np.ones((ny, nx)); u = np.zeros((ny, nx + 1)); v = np.zeros((ny + 1, nx))
    u[4, 12] = -3.0; v[9, 0] = 0.25
    # no solid cell
    np.testing.assert_array_equal(M.soft_diag(phi, J, u, v, dx, dy),
                                  [0.0, 0.0, 0.0, -0.5, 21.0, 3.0, 0.25, 0.0])
    # a single solid cell, the last one
    phi[8, 11] = 0.0
    got = M.soft_diag(phi, J, u, v, dx, dy)
    _check_diag(got, NP.soft_diag(phi, J, u, v, dx, dy))
    np.testing.assert_array_equal(got[:3], [1.0, 11.5 * dx, 8.5 * dy])
    # a NaN in v: the flag, and max|v| propagates it; an inf in u
    v[3, 5] = np.nan
    got = M.soft_diag(phi, J, u, v, dx, dy)
    assert got[7] == 1.0 and np.isnan(got[6]) and got[5] == 3.0 and got[0] == 1.0
    v[3, 5] = 0.0; u[0, 0] = np.inf
    got = M.soft_diag(phi, J, u, v, dx, dy)
    assert got[7] == 1.0 and got[5] == np.inf and got[6] == 0.25
    # a NaN in J reaches both extremes
    J[0, 0] = np.nan
    got = M.soft_diag(phi, J, u, v, dx, dy)
    assert np.isnan(got[3]) and np.isnan(got[4])


# ---------------------------------------------------------------- the loop ----
def _sim(M, name, **over):
    kw = dict(NP.TRACES[name][0]); kw.update(over)
    return M.MacSoftDisc(NP.N, **kw)


STEPS = [(name, k) for name, (_, _, keep) in NP.TRACES.items() for k in keep]


@pytest.mark.parametrize("name,k", STEPS, ids=[f"{n}-{k}" for n, k in STEPS])
def test_one_step_from_captured_state(M, fx, name, k):
    rec = fx[f"{name}_record"]
    sim = _sim(M, name)
    assert sim.dt == float(fx[f"{name}_dt"])
    sim.set_state(dict({f: fx[f"{name}_before{k}_{f}"] for f in ("u", "v", "X1", "X2")},
                       t=rec[k - 2, 0] if k > 1 else 0.0))
    sim.step(1)
    assert not sim.diverged and sim.nsteps == 1
    s = sim.state()
    assert s["t"] == rec[k - 1, 0]
    for f in ("u", "v", "X1", "X2"):
        err = np.abs(s[f] - fx[f"{name}_after{k}_{f}"]).max()
        print(f"{name} step {k}, {f}: max abs {err:.3e}")
        np.testing.assert_allclose(s[f], fx[f"{name}_after{k}_{f}"], rtol=0, atol=NP.STEP_BAR,
                                   err_msg=f)
    assert list(sim.pcg_iters) == fx[f"{name}_its"][k - 1].tolist()
    assert sim.sl_steps == int(fx[f"{name}_sl"][k - 1])
    np.testing.assert_array_equal(sim.get("J"), fx[f"{name}_after{k}_J"])
    np.testing.assert_allclose(sim.record[-1], rec[k - 1], rtol=1e-12)


def test_explicit_map_half_is_bitwise(M, fx):
    """No CG, sine or spline between the state and the explicit rung's maps and level set."""
    sim = _sim(M, "explicit")
    sim.set_state({f: fx[f"explicit_before12_{f}"] for f in ("u", "v", "X1", "X2")})
    sim.step(1)
    for f in ("X1", "X2", "phi"):
        np.testing.assert_array_equal(sim.get(f), fx[f"explicit_after12_{f}"], err_msg=f)


@pytest.fixture(scope="module")
def runs(M, fx):
    """Each trace run once from the start."""
    out = {}
    for name in NP.TRACES:
        kw = {k: v for k, v in NP.TRACES[name][0].items() if k != "integrator"}
        out[name] = M.mac_soft_disc_run(NP.N, float(fx[f"{name}_t_end"]),
                                        integrator=INTEGRATOR[name], return_sim=True, **kw)
    return out


@pytest.mark.parametrize("name", list(NP.TRACES))
def test_trace(runs, fx, name):
    traj, sim = runs[name]
    rec = fx[f"{name}_record"]
    assert not sim.diverged and traj.shape == rec.shape and sim.nsteps == len(rec)
    np.testing.assert_allclose(traj[:, 0], rec[:, 0], rtol=1e-15)
    for col, what in ((1, "cx"), (2, "cy"), (3, "minJ"), (4, "maxJ")):
        err = np.abs(traj[:, col] / rec[:, col] - 1).max()
        print(f"{name}, {what}: max relative {err:.3e}")
        np.testing.assert_allclose(traj[:, col], rec[:, col], rtol=1e-9, err_msg=what)
    assert sim.sl_steps == int(fx[f"{name}_sl"].sum())
    s = sim.state()
    for f in ("u", "v", "X1", "X2"):
        err = np.abs(s[f] - fx[f"{name}_final_{f}"]).max()
        print(f"{name}, final {f}: max abs {err:.3e}")
        np.testing.assert_allclose(s[f], fx[f"{name}_final_{f}"], rtol=0, atol=1e-9, err_msg=f)


def test_t_end_is_not_clipped(runs, fx):
    traj, sim = runs["imex_sl"]
    t_end = float(fx["imex_sl_t_end"])
    assert traj[-2, 0] < t_end <= traj[-1, 0] and traj[-1, 0] - t_end < sim.dt
    assert traj[-1, 0] != t_end
    sim.step(3, t_end)          # nothing more to do
    assert sim.nsteps == len(traj)


def test_folded_map_stops_without_a_row(M, fx):
    sim = _sim(M, "elastic")
    st = {f: fx[f"elastic_before12_{f}"].copy() for f in ("u", "v", "X1", "X2")}
    # rows through the disc's centre (y = 0.5), two apart with two between: the central
    # difference across them turns negative (adjacent rows would leave it at +1/2)
    for f in ("X1", "X2"):
        st[f][[14, 17]] = st[f][[17, 14]]
    t0 = float(fx["elastic_record"][10, 0])
    sim.set_state(dict(st, t=t0))
    sim.step(5)
    assert sim.diverged and sim.record == [] and sim.nsteps == 0 and sim.t == t0
    assert sim.get("J").min() < 0.0
    sim.step(5)
    assert sim.record == []
    # set_state clears the stop
    sim.set_state({f: fx[f"elastic_before12_{f}"] for f in ("u", "v", "X1", "X2")})
    sim.step(1)
    assert not sim.diverged and len(sim.record) == 1


def test_state_round_trip_and_set_state_contract(M):
    """state() -> a fresh sim -> set_state -> state() holds every bit; set_state's refusals, its
    copy of what it is given, and its clearing of the `diverged` stop."""
    import torch
    sim = _sim(M, "elastic")
    sim.step(4)
    s = sim.state()
    assert tuple(s) == M.MacSoftDisc.STATE and not sim.diverged
    fresh = _sim(M, "elastic")
    assert not np.array_equal(s["X1"], fresh.state()["X1"]) and s["u"].any()
    fresh.set_state(s)
    s1 = fresh.state()
    for k in M.MacSoftDisc.STATE:
        np.testing.assert_array_equal(s1[k], s[k], err_msg=k)
    assert type(s1["t"]) is float
    # the state is all a step reads: both sims take the same next step
    sim.step(1); fresh.step(1)
    assert fresh.record[-1] == sim.record[-1]
    for k, a in fresh.state().items():
        np.testing.assert_array_equal(a, sim.state()[k], err_msg=k)
    # refusals
    with pytest.raises(KeyError, match="unknown fields"):
        fresh.set_state({"phi": s["X1"]})
    with pytest.raises(ValueError, match="u has shape"):
        fresh.set_state({"u": s["u"][:, :-1]})
    # what it is given is copied, not kept
    u_dev = torch.from_numpy(s["u"]).cuda()
    u_keep = u_dev.clone()
    fresh.set_state({"u": u_dev})
    assert fresh.u.data_ptr() != u_dev.data_ptr()
    fresh.step(1)
    assert torch.equal(u_dev, u_keep)
    # a `diverged` stop (test_folded_map_stops_without_a_row's folded map), cleared by set_state
    bad = {f: s[f].copy() for f in ("X1", "X2")}
    for f in ("X1", "X2"):
        bad[f][[14, 17]] = bad[f][[17, 14]]
    fresh.set_state(dict(s, **bad))
    n = fresh.nsteps
    fresh.step(3)
    assert fresh.diverged and fresh.nsteps == n and fresh.t == s["t"]
    fresh.set_state(s)
    assert not fresh.diverged
    fresh.step(1)
    assert fresh.nsteps == n + 1 and not fresh.diverged and fresh.t > s["t"]


# ---------------------------------------------------------------- physics, N = 48 ----
# The reference's own checks at its own N and dt (the matched, viscous-limited dt of
# test_imex_wall.py:69 and test_elastic_imex_fsi.py:29), rows compared one to one.
PHYS_N, PHYS_T = 48, 0.8
PHYS_DT = 0.2 * (1.0 / PHYS_N) ** 2 / 0.01


@pytest.fixture(scope="module")
def explicit48(M):
    return M.mac_soft_disc_run(PHYS_N, PHYS_T, integrator="explicit", dt=PHYS_DT)


def _drift(te, ti):
    n = min(len(te), len(ti))
    assert n > 5, "trajectory too short (a run diverged)"
    return np.abs(te[:n, 1] - ti[:n, 1]).max(), np.abs(te[:n, 2] - ti[:n, 2]).max()


def test_imex_follows_explicit(M, explicit48):
    """test_imex_wall.py:64-76 (t_end 0.8)."""
    ti = M.mac_soft_disc_run(PHYS_N, PHYS_T, imex=True, dt=PHYS_DT)
    dcx, dcy = _drift(explicit48, ti)
    print(f"imex vs explicit at N = {PHYS_N}: dcx {dcx:.3e}, dcy {dcy:.3e}")
    assert len(ti) == len(explicit48) and dcx < 6e-3 and dcy < 6e-3


def test_imex_elastic_follows_explicit(M, explicit48):
    """test_elastic_imex_fsi.py:25-36."""
    tl = M.mac_soft_disc_run(PHYS_N, PHYS_T, integrator="imex-elastic", dt=PHYS_DT)
    dcx, dcy = _drift(explicit48, tl)
    print(f"imex-elastic vs explicit at N = {PHYS_N}: dcx {dcx:.3e}, dcy {dcy:.3e}")
    assert len(tl) == len(explicit48) and dcx < 5e-3 and dcy < 5e-3


def test_stiff_disc_runs(M):
    """test_elastic_imex_fsi.py:39-46."""
    dx = 1.0 / PHYS_N
    traj, sim = M.mac_soft_disc_run(PHYS_N, 0.5, integrator="imex-elastic", mu_s=8.0,
                                    dt=0.3 * dx / 1.0, return_sim=True)
    assert not sim.diverged and traj[-1, 0] >= 0.5 - 1e-9 and np.isfinite(traj).all()


# ---------------------------------------------------------------- refusals ----
def test_refusals(M):
    with pytest.raises(NotImplementedError, match="FMM"):
        M.MacSoftDisc(NP.N, scheme="conservative")
    with pytest.raises(NotImplementedError, match="FMM"):
        M.MacSoftDisc(NP.N, reinit=True)
    with pytest.raises(NotImplementedError, match="FMM"):
        M.mac_soft_disc_run(NP.N, 0.1, reinit=True)
    with pytest.raises(ValueError, match="unknown integrator"):
        M.MacSoftDisc(NP.N, integrator="rk4")
    with pytest.raises(ValueError, match="not available"):
        M.resolve_integrator("imex-elastic", supports_elastic=False)
    with pytest.raises(ValueError, match="scheme"):
        M.MacSoftDisc(NP.N, scheme="upwind")
