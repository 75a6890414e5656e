"""GPU parity of the free-slip MAC box: pyrmt_amd.mac's momentum_predictor_freeslip and
interfacial_force_faces, and the fused loop with free-slip walls (MacDiscTaylorGreen,
MacTwoDiscContact) against the reference's fixtures (tests/golden/mac_freeslip_*.npz,
gen_mac_freeslip.py).

Bars: bit-exact for the two operators (IEEE arithmetic in the reference's order); the
projection to 1e-12 of its scale (test_mac_projection's bar); the loops' end fields to 1e-9
absolute (test_mac_multi_disc_trace's bar), J range and KE 1e-9, Estrain 1e-7 relative, the
two-disc history 1e-10 relative.  The fixtures hold the reference's own one-ulp noise floor
(noise_*), a tenth of each bar or less (the J range: 0.11 of it at N = 64).
"""
import numpy as np
import pytest

from conftest import golden
import mac_freeslip_np as NP

pytestmark = pytest.mark.gpu

OPTION_SETS = ({"mac_boxes": 0}, {"mac_boxes": 1}, {"mac_boxes": 1, "mac_noop_host": 0},
               {"mac_boxes": 1, "mac_face_sl": 0}, {"mac_boxes": 0, "mac_face_sl": 0},
               {"mac_boxes": 1, "mac_m2_bound": 0})


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


# ------------------------------------------------------------------ operators --------
@pytest.mark.parametrize("N", [4, 5, 33, 64])
def test_freeslip_operators_bitwise(M, N):
    g = NP.ops_fixture(golden, N)
    dx = dy = 1.0 / N
    us, vs = M.momentum_predictor_freeslip(g["u"], g["v"], g["nu"], dx, dy, g["dt"], fu=g["fu"],
                                           fv=g["fv"], rho=g["rho"])
    np.testing.assert_array_equal(us, g["us"])
    np.testing.assert_array_equal(vs, g["vs"])
    us0, vs0 = M.momentum_predictor_freeslip(g["u"], g["v"], g["nu"], dx, dy, g["dt"])
    np.testing.assert_array_equal(us0, g["us0"])
    np.testing.assert_array_equal(vs0, g["vs0"])
    gu, gv = M.interfacial_force_faces(g["kappa"], g["H"], g["gamma"], dx, dy)
    np.testing.assert_array_equal(gu, g["gu"])
    np.testing.assert_array_equal(gv, g["gv"])


@pytest.mark.parametrize("N", [256, 1023])
def test_freeslip_operators_against_numpy(M, N):
    rng = np.random.default_rng(4400 + N)
    dx = dy = 1.0 / N
    u, fu = rng.standard_normal((2, N, N + 1))
    v, fv = rng.standard_normal((2, N + 1, N))
    kappa, H = rng.standard_normal((2, N, N))
    for kw in ({"fu": fu, "fv": fv, "rho": 1.3}, {}):
        us, vs = M.momentum_predictor_freeslip(u, v, 0.01, dx, dy, 1e-3, **kw)
        eu, ev = NP.momentum_predictor_freeslip(u, v, 0.01, dx, dy, 1e-3, **kw)
        np.testing.assert_array_equal(us, eu)
        np.testing.assert_array_equal(vs, ev)
    gu, gv = M.interfacial_force_faces(kappa, H, 0.07, dx, dy)
    eu, ev = NP.interfacial_force_faces(kappa, H, 0.07, dx, dy)
    np.testing.assert_array_equal(gu, eu)
    np.testing.assert_array_equal(gv, ev)


def test_freeslip_operators_keep_device_tensors(M):
    import torch
    g = NP.ops_fixture(golden, 33)
    dx = 1.0 / 33
    t = {k: torch.from_numpy(g[k]).cuda() for k in ("u", "v", "fu", "fv", "kappa", "H")}
    us, vs = M.momentum_predictor_freeslip(t["u"], t["v"], g["nu"], dx, dx, g["dt"], fu=t["fu"],
                                           fv=t["fv"], rho=g["rho"])
    gu, gv = M.interfacial_force_faces(t["kappa"], t["H"], g["gamma"], dx, dx)
    for a, name in ((us, "us"), (vs, "vs"), (gu, "gu"), (gv, "gv")):
        assert isinstance(a, torch.Tensor) and a.is_cuda
        np.testing.assert_array_equal(a.cpu().numpy(), g[name])


def test_freeslip_operators_refuse_bad_shapes(M):
    z = np.zeros
    with pytest.raises(NotImplementedError):
        M.momentum_predictor_freeslip(z((8, 11)), z((9, 10)), 0.01, 0.1, 0.125, 1e-3)
    with pytest.raises(NotImplementedError):
        M.interfacial_force_faces(z((8, 10)), z((8, 10)), 0.1, 0.1, 0.125)
    with pytest.raises(NotImplementedError):
        M.momentum_predictor_freeslip(z((8, 9)), z((9, 8)), 0.01, 0.125, 0.125, 1e-3,
                                      fu=z((8, 9)))


def test_freeslip_differs_from_lid_in_the_ghosts_only(M):
    """On a Taylor-Green field the free-slip predictor and the lid one at U_lid = 0 differ on
    the wall-adjacent tangential faces (u rows 0, N-1; v columns 0, N-1: the ghosts) and are
    the same bits everywhere else."""
    N = 48
    dx = 1.0 / N
    xc = (np.arange(N) + 0.5) * dx; xf = np.arange(N + 1) * dx
    Xu, Yu = np.meshgrid(xf, xc)
    Xv, Yv = np.meshgrid(xc, xf)
    u = 0.3 * np.pi * np.sin(np.pi * Xu) * np.cos(np.pi * Yu)
    v = -0.3 * np.pi * np.cos(np.pi * Xv) * np.sin(np.pi * Yv)
    fs_u, fs_v = M.momentum_predictor_freeslip(u, v, 0.01, dx, dx, 1e-3)
    ld_u, ld_v = M.momentum_predictor(u, v, 0.01, dx, dx, 1e-3, 0.0)
    np.testing.assert_array_equal(fs_u[1:-1], ld_u[1:-1])
    np.testing.assert_array_equal(fs_v[:, 1:-1], ld_v[:, 1:-1])
    np.testing.assert_array_equal(fs_u[:, [0, -1]], ld_u[:, [0, -1]])
    np.testing.assert_array_equal(fs_v[[0, -1], :], ld_v[[0, -1], :])
    assert np.all(fs_u[[0, -1], 1:-1] != ld_u[[0, -1], 1:-1])
    assert np.all(fs_v[1:-1, [0, -1]] != ld_v[1:-1, [0, -1]])


def test_interfacial_force_is_balanced_for_constant_curvature(M):
    """The reference's tests/test_mac.py:115-131: with constant curvature the face force is
    the discrete face gradient of -gamma * kappa * H."""
    N = 40
    dx, dy = M.mac_grid(N, N)
    xc = (np.arange(N) + 0.5) * dx
    Xc, Yc = np.meshgrid(xc, xc)
    H = 0.5 * (1 + np.tanh((np.sqrt((Xc - .5)**2 + (Yc - .5)**2) - .25) / (2 * dx)))
    gamma, kR = 0.1, 4.0
    fu, fv = M.interfacial_force_faces(np.full((N, N), kR), H, gamma, dx, dy)
    phi = -gamma * kR * H
    np.testing.assert_allclose(fu, M.gradient_p_u(phi, dx), rtol=0, atol=1e-12)
    np.testing.assert_allclose(fv, M.gradient_p_v(phi, dy), rtol=0, atol=1e-12)


def test_static_drop_composed_step(M, gpu):
    """circle phi -> curvature -> H -> face force -> free-slip predictor from rest ->
    projection.  The two new operators are bit-exact on the fixture's inputs of their stage;
    the chain composed on the device (its H from the device's sin, within 4e-16 of the
    reference's) ends within 1e-12 of scale: max |u*| for u, v, max |p| for p (the
    projection's rounding error is relative to its input, test_mac_projection's bar)."""
    g = golden("mac_freeslip_drop")
    N = int(g["N"])
    dx = dy = 1.0 / N
    gamma, nu, rho, dt = (float(g[k]) for k in ("gamma", "nu", "rho", "dt"))
    fu, fv = M.interfacial_force_faces(g["kappa"], g["H"], gamma, dx, dy)
    np.testing.assert_array_equal(fu, g["fu"])
    np.testing.assert_array_equal(fv, g["fv"])
    z = np.zeros
    us, vs = M.momentum_predictor_freeslip(z((N, N + 1)), z((N + 1, N)), nu, dx, dy, dt,
                                           fu=g["fu"], fv=g["fv"], rho=rho)
    np.testing.assert_array_equal(us, g["us"])
    np.testing.assert_array_equal(vs, g["vs"])
    # the chain
    kappa = gpu.compute_curvature(g["phi"], dx, dy)
    np.testing.assert_array_equal(kappa, g["kappa"])
    H = gpu.smoothed_heaviside(g["phi"], 2.0 * dx)
    np.testing.assert_allclose(H, g["H"], rtol=0, atol=4e-16)
    fu, fv = M.interfacial_force_faces(kappa, H, gamma, dx, dy)
    us, vs = M.momentum_predictor_freeslip(z((N, N + 1)), z((N + 1, N)), nu, dx, dy, dt, fu=fu,
                                           fv=fv, rho=rho)
    u, v, p = M.project(us, vs, dx, dy, dt, rho, M.poisson_eigs_neumann(N, N, dx, dy))
    su = max(np.abs(g["us"]).max(), np.abs(g["vs"]).max())
    np.testing.assert_allclose(u, g["u"], rtol=0, atol=1e-12 * su)
    np.testing.assert_allclose(v, g["v"], rtol=0, atol=1e-12 * su)
    np.testing.assert_allclose(p, g["p"], rtol=0, atol=1e-12 * np.abs(g["p"]).max())


# ------------------------------------------------------------------ disc in vortex ---
@pytest.mark.parametrize("N,n", [(32, 24), (33, 24), (64, 40)])
def test_disc_in_vortex(M, N, n):
    """mac_disc_in_tg_convergence.py run_one(N, (n + 0.5) dt): n full steps and a truncated
    one."""
    g = golden("mac_freeslip_tg")
    f = {k[len(f"n{N}_"):]: g[k] for k in g.files if k.startswith(f"n{N}_")}
    assert int(f["n"]) == n
    dt = M.disc_in_tg_dt(N)
    assert dt == float(f["dt"])
    sim, r = M._disc_in_tg_run(N, (n + 0.5) * dt)
    d = sim.diagnostics()
    print(f"N={N}: |du| {np.abs(sim.get('u') - f['u']).max():.3g} |dv| "
          f"{np.abs(sim.get('v') - f['v']).max():.3g} |dp| {np.abs(r['p'] - f['p']).max():.3g} "
          f"|dX1| {np.abs(sim.get('X1') - f['X1']).max():.3g} |dX2| "
          f"{np.abs(sim.get('X2') - f['X2']).max():.3g} KE {r['KE'] / float(f['KE']) - 1:.3g} "
          f"Estrain {r['Estrain'] / float(f['Estrain']) - 1:.3g} divmax {r['divmax']:.3g}")
    assert len(d["t"]) == n + 1
    assert d["dt"][-1] == float(f["dt_last"]) and d["dt"][-1] < dt and np.all(d["dt"][:-1] == dt)
    for name in ("u", "v", "p", "X1", "X2", "phi"):
        np.testing.assert_allclose(sim.get(name), f[name], rtol=0, atol=1e-9, err_msg=name)
    np.testing.assert_allclose(d["minJ"], f["J"][:, 0], rtol=1e-9)
    np.testing.assert_allclose(d["maxJ"], f["J"][:, 1], rtol=1e-9)
    np.testing.assert_allclose(r["KE"], float(f["KE"]), rtol=1e-9)
    np.testing.assert_allclose(r["Estrain"], float(f["Estrain"]), rtol=1e-7)
    assert r["divmax"] < 1e-9
    np.testing.assert_array_equal(r["p"], sim.get("p"))
    assert r["N"] == N and r["dx"] == 1.0 / N and r["speed"].shape == (N, N)
    np.testing.assert_array_equal(r["xc"], (np.arange(N) + 0.5) * (1.0 / N))


def test_disc_in_tg_run_one_returns_the_reference_dict(M):
    g = golden("mac_freeslip_tg")
    dt = M.disc_in_tg_dt(32)
    r = M.disc_in_tg_run_one(32, 24.5 * dt, w_cut_fac=7.0)
    assert sorted(r) == sorted(["N", "dx", "xc", "speed", "p", "KE", "Estrain", "divmax"])
    np.testing.assert_allclose(r["KE"], float(g["n32_KE"]), rtol=1e-9)
    np.testing.assert_allclose(r["p"], g["n32_p"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ two discs --------
@pytest.fixture(scope="module")
def two_disc_runs(M):
    c = golden("mac_freeslip_contact")
    runs = {}
    for tag, eta in (("eta2", 2.0), ("eta0", 0.0)):
        sim = M.MacTwoDiscContact(N=int(c["N"]), V0=float(c["V0"]), eta=eta)
        sim.step(2**31 - 1, float(c["t_end"]))
        runs[tag] = (sim.history(), sim.get("u"), sim.get("v"))
    return c, runs


@pytest.mark.parametrize("tag", ["eta2", "eta0"])
def test_two_disc_contact(two_disc_runs, tag):
    c, runs = two_disc_runs
    h, u, v = runs[tag]
    ref = c[f"{tag}_hist"]
    print(f"{tag}: |du| {np.abs(u - c[tag + '_u']).max():.3g} |dv| "
          f"{np.abs(v - c[tag + '_v']).max():.3g} hist {np.abs(h / ref - 1).max():.3g}")
    assert h.shape == ref.shape
    np.testing.assert_array_equal(h[:, 0], ref[:, 0])
    np.testing.assert_allclose(h, ref, rtol=1e-10)
    np.testing.assert_allclose(u, c[f"{tag}_u"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(v, c[f"{tag}_v"], rtol=0, atol=1e-9)


def test_two_disc_contact_term_acts(two_disc_runs):
    """eta = 0 and eta = 2 differ by more than 1e-3 in u: a dropped contact term cannot pass."""
    _, runs = two_disc_runs
    assert np.abs(runs["eta2"][1] - runs["eta0"][1]).max() > 1e-3


def test_loop_goes_on_past_divergence_when_told_to(M):
    """test_mac_sim_stops_on_divergence's construction (a mirrored map: J < 0): the default
    stops after the flagged record, stop_on_divergence=False goes on stepping."""
    counts = {}
    for stop in (True, False):
        sim = M.MacMultiDisc(64, n_discs=3, seed=3, stop_on_divergence=stop)
        R, cx, cy = sim.specs[0]
        X1 = sim.get("X1", 0)
        sim.field("X1", 0).copy_(sim.torch.as_tensor(2 * cx - X1))
        sim.step(2)
        d = sim.diagnostics()
        assert d["diverged"][0] == 1 and d["minJ"][0] < 0
        sim.step(1)
        counts[stop] = len(sim.diagnostics()["t"])
    assert counts == {True: 1, False: 3}


# ------------------------------------------------------------------ mode switch ------
def test_set_mode_after_a_step_raises(M):
    sim = M.MacMultiDisc(16, specs=[(0.2, 0.5, 0.5)])
    sim.set_mode("freeslip", False)
    sim.set_mode("lid", True)
    sim.step(1)
    with pytest.raises(ValueError, match="before the first step"):
        sim.set_mode("freeslip", True)
    from pyrmt_amd import _lib as L
    fresh = M.MacMultiDisc(16, specs=[(0.2, 0.5, 0.5)])
    with pytest.raises(ValueError, match="unknown wall kind"):
        L.check(L.lib().rmt_mac_sim_set_mode(fresh.h, 2, 1), "rmt_mac_sim_set_mode")


def test_lid_keyword_is_todays_loop(M):
    """walls="lid" through the new keyword and through set_mode: the same bits as the plain
    MacMultiDisc on the mac_trace case, and the reference's trace to its bar."""
    g = golden("mac_trace")
    N, K = int(g["N"]), int(g["nsteps"])
    sims = [M.MacMultiDisc(N, n_discs=3, seed=3),
            M.MacMultiDisc(N, n_discs=3, seed=3, walls="lid", stop_on_divergence=True),
            M.MacMultiDisc(N, n_discs=3, seed=3, walls="lid", stop_on_divergence=False)]
    for s in sims:
        s.step(K)
    d0 = sims[0].diagnostics()
    for s in sims[1:]:
        d = s.diagnostics()
        for k in d0:
            np.testing.assert_array_equal(d[k], d0[k], err_msg=k)
        for name in ("u", "v", "p"):
            np.testing.assert_array_equal(s.get(name), sims[0].get(name))
        for k in range(3):
            for name in ("X1", "X2", "phi"):
                np.testing.assert_array_equal(s.get(name, k), sims[0].get(name, k))
    np.testing.assert_allclose(sims[1].get("u"), g["u"], rtol=0, atol=1e-9)
    # free-slip walls on the same case are another flow
    fs = M.MacMultiDisc(N, n_discs=3, seed=3, walls="freeslip")
    fs.step(K)
    assert np.abs(fs.get("u") - sims[0].get("u")).max() > 1e-3


# ------------------------------------------------------------------ switches ---------
@pytest.mark.parametrize("N", [64, 256])
def test_freeslip_loop_is_bit_identical_across_switches(M, N):
    """test_mac_box_mode_is_bit_identical's option sets on the disc-in-vortex loop, over calls
    of (3, 1, 4) steps: every field and record bit for bit."""
    out = []
    for opts in OPTION_SETS:
        sim = M.MacDiscTaylorGreen(N, options=opts)
        for c in (3, 1, 4):
            sim.step(c)
        f = {n: sim.get(n) for n in ("u", "v", "p", "X1", "X2", "phi")}
        out.append((sim.diagnostics(), f))
    d0, f0 = out[0]
    assert len(d0["t"]) == 8 and np.abs(f0["X1"]).max() > 0
    for d1, f1 in out[1:]:
        for k in d0:
            np.testing.assert_array_equal(d1[k], d0[k], err_msg=k)
        for k in f0:
            np.testing.assert_array_equal(f1[k], f0[k], err_msg=k)
