"""GPU parity of the four-roll-mill viscoelastic driver (mac_ve.hip, pyrmt_amd.mac:
ve_centre_kinematics, ve_face_force, momentum_predictor_periodic_imex_elastic, ve_lock, ve_record,
MacViscoelasticExtension) against the reference's benchmarks/mac_viscoelastic_extension.py and
pyRMT/mac.py:560-584 (tests/golden/mac_ve_extension_ops.npz, mac_ve_extension_runs.npz, which
test_mac_ve_extension_cpu.py pins to the NumPy restatement tests/mac_ve_extension_np.py).

Bars: == for the centre kinematics, the elastic IMEX right-hand side, the explicit lock, the
record reduction, step counts, t and dt (arithmetic, sqrt and comparisons only); bit for bit
against this package's own operators composed for the kinematics and the face force; 1e-12 of
max-abs for what one FFT pair separates from the reference (the predictor's u*, v*: the project's
bar for rocFFT against pocketfft); everything behind sin / exp / log / cos / atan2 and several
solves within mac_ve_extension_np.bar(case) = 4 x its measured noise floor
(profiles/ve_extension/floor.json), printed before it is asserted.  The reference's five checks
at N = 40 keep the reference's own bars, and the device's final b_xx lies within a tenth of each
bar of the reference's recorded value.
"""
import ctypes
import math

import numpy as np
import pytest

from conftest import golden
import mac_ve_extension_np as E

pytestmark = pytest.mark.gpu

NP, same_bits, close = E.NP, E.same_bits, E.assert_close
eq = np.testing.assert_array_equal
FULL = [s for s in E.SHAPES if s != E.ARITH_ONLY]


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


@pytest.fixture(scope="module")
def ops():
    return golden("mac_ve_extension_ops")


@pytest.fixture(scope="module")
def runs():
    return golden("mac_ve_extension_runs")


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _host(ts):
    return np.stack([t.cpu().numpy() for t in ts])


def _ref(ops, shape, name, compute):
    k = f"{E.key(shape)}_{name}"
    return ops[k] if k in ops.files else np.stack(compute())


# --------------------------------------------------- centre kinematics, face force --
@pytest.mark.parametrize("shape", E.SHAPES, ids=E.key)
def test_centre_kinematics_bitwise(M, ops, shape):
    """== the reference; from 5 x 5 (the collocated operators' smallest grid) also the bits of
    grad_central_*_2nd and torch.roll composed.  (3, 3) is the smallest grid the one-sided rule
    admits, (5, 7) lies below a tile, (33, 70) crosses the launch's workgroup edge."""
    import torch
    from pyrmt_amd import functions as F
    g = E.op_inputs(shape)
    got = M.ve_centre_kinematics(g["u"], g["v"], E.DX, E.DY)
    assert isinstance(got[0], np.ndarray) and got[0].shape == tuple(shape)
    assert same_bits(np.stack(got), ops[E.key(shape) + "_kin"])
    if min(shape) >= 5:
        u, v = _dev(g["u"], g["v"])
        u_c = 0.5 * (u + torch.roll(u, -1, 1)); v_c = 0.5 * (v + torch.roll(v, -1, 0))
        comp = [u_c, v_c, F.grad_central_x_2nd(u_c, E.DX), F.grad_central_y_2nd(u_c, E.DY),
                F.grad_central_x_2nd(v_c, E.DX), F.grad_central_y_2nd(v_c, E.DY)]
        dgot = M.ve_centre_kinematics(u, v, E.DX, E.DY)
        assert all(t.is_cuda for t in dgot)
        assert same_bits(_host(dgot), _host(comp))


@pytest.mark.parametrize("shape", E.SHAPES, ids=E.key)
def test_face_force(M, ops, shape):
    """4 x floor against the reference (through sin alone); from 5 x 5 the bits of
    smoothed_heaviside, grad_central_*_2nd and torch.roll composed.  At (33, 70) the wrap lies
    inside a partial tile in both directions."""
    import torch
    from pyrmt_amd import functions as F
    g = E.op_inputs(shape)
    b = (g["be11"], g["be12"], g["be22"])
    got = M.ve_face_force(*b, g["phi"], E.G, E.W_T, E.DX, E.DY)
    ref = _ref(ops, shape, "force", lambda: NP.face_force(*b, g["phi"], E.G, E.W_T, E.DX, E.DY))
    close(np.stack(got), ref, "force", f"face force {shape}")
    # chi = 1 - H, Hu, Hv: the clamps are exact
    assert np.array_equal(got[4] == 0.0, ref[4] == 0.0) and np.array_equal(got[4] == 1.0,
                                                                          ref[4] == 1.0)
    if min(shape) >= 5:
        b11, b12, b22, phi = _dev(*b, g["phi"])
        H = F.smoothed_heaviside(phi, E.W_T)
        Sxx = (1 - H) * E.G * b11; Sxy = (1 - H) * E.G * b12; Syy = (1 - H) * E.G * b22
        divx = F.grad_central_x_2nd(Sxx, E.DX) + F.grad_central_y_2nd(Sxy, E.DY)
        divy = F.grad_central_x_2nd(Sxy, E.DX) + F.grad_central_y_2nd(Syy, E.DY)
        comp = [0.5 * (divx + torch.roll(divx, 1, 1)), 0.5 * (divy + torch.roll(divy, 1, 0)),
                0.5 * (H + torch.roll(H, 1, 1)), 0.5 * (H + torch.roll(H, 1, 0)), 1.0 - H]
        dgot = M.ve_face_force(b11, b12, b22, phi, E.G, E.W_T, E.DX, E.DY)
        assert same_bits(_host(dgot), _host(comp))


MUT_SHAPE = (33, 70)
MUT_CELLS = [(0, 0), (0, 69), (32, 0), (32, 69), (0, 35), (32, 35), (16, 0), (16, 69), (15, 31),
             (16, 32), (1, 1), (31, 68)]


def _changed(a, b):
    a, b = np.stack(a), np.stack(b)
    return a.view(np.int64) != b.view(np.int64)


@pytest.mark.parametrize("cell", MUT_CELLS, ids=lambda c: f"{c[0]}_{c[1]}")
def test_mutation_centre_kinematics(M, cell):
    """One changed cell of u, then of v -- at each corner, on each edge, beside them and on both
    sides of a workgroup edge -- moves exactly the outputs the stencil says (the restatement's
    set: the wrapping averages, the one-sided gradients) and no others."""
    g = E.op_inputs(MUT_SHAPE)
    base = M.ve_centre_kinematics(g["u"], g["v"], E.DX, E.DY)
    ref0 = NP.centre_kinematics(g["u"], g["v"], E.DX, E.DY)
    for name in ("u", "v"):
        h = {k: g[k].copy() for k in ("u", "v")}
        h[name][cell] += 1.0
        got = _changed(M.ve_centre_kinematics(h["u"], h["v"], E.DX, E.DY), base)
        want = _changed(NP.centre_kinematics(h["u"], h["v"], E.DX, E.DY), ref0)
        assert want.sum() >= 6
        eq(got, want)


@pytest.mark.parametrize("cell", MUT_CELLS, ids=lambda c: f"{c[0]}_{c[1]}")
def test_mutation_face_force(M, cell):
    """The same for the face force, with phi inside the band everywhere (every cell carries
    stress): a changed cell of be12 moves both force components two cells along and one across,
    a changed cell of phi moves H's three outputs as well."""
    g = E.op_inputs(MUT_SHAPE)
    j, i = np.meshgrid(np.arange(MUT_SHAPE[0]), np.arange(MUT_SHAPE[1]), indexing="ij")
    phi = E.W_T * (0.25 + 0.125 * (((3 * i + 5 * j) % 7) - 3) / 3.0)
    args = dict(be11=g["be11"], be12=g["be12"], be22=g["be22"], phi=phi)
    call = lambda f, a: f(a["be11"], a["be12"], a["be22"], a["phi"], E.G, E.W_T, E.DX, E.DY)
    base, ref0 = call(M.ve_face_force, args), call(NP.face_force, args)
    for name, delta in (("be12", 1.0), ("phi", 0.25 * E.W_T)):
        h = dict(args)
        h[name] = args[name].copy()
        h[name][cell] += delta
        got = _changed(call(M.ve_face_force, h), base)
        want = _changed(call(NP.face_force, h), ref0)
        assert want[:2].sum() >= 8 and (name == "be12" or want[2:].sum() == 5)
        eq(got, want)


def test_output_planes_must_be_their_own(M):
    """Aliasing that is not allowed: an output plane that is an input plane is refused."""
    import torch
    from pyrmt_amd import _lib as L
    from pyrmt_amd.functions import _p, _plane_ptrs, ctx_for
    z = [torch.zeros((8, 8), dtype=torch.float64, device="cuda") for _ in range(8)]
    c = ctx_for(8, 8).bind()
    with pytest.raises(ValueError, match="of their own"):
        L.check(L.lib().rmt_mac_ve_centre_kinematics(c, _p(z[0]), _p(z[1]), 0.1, 0.1, _p(z[0]),
                                                     _p(z[2]), _plane_ptrs(z[3:7])))
    with pytest.raises(ValueError, match="of their own"):
        L.check(L.lib().rmt_mac_ve_face_force(c, _plane_ptrs(z[0:3]), _p(z[3]), 0.3, 0.1, 0.1, 0.1,
                                              _p(z[4]), _p(z[5]), _p(z[6]), _p(z[7]), _p(z[3])))
    with pytest.raises(ValueError, match="not in place"):
        L.check(L.lib().rmt_mac_per_imex_elastic_rhs(c, _p(z[0]), _p(z[1]), 0.2, 0.2, 0.01, 0.01,
                                                     0.1, 0.003, 1.0, _p(z[2]), _p(z[3]), _p(z[4]),
                                                     _p(z[0]), _p(z[5])))


# ------------------------------------------------------------- elastic IMEX predictor --
@pytest.mark.parametrize("shape", E.SHAPES, ids=E.key)
def test_imex_elastic_rhs_and_predictor(M, ops, shape):
    g, k = E.op_inputs(shape), E.key(shape)
    chi = NP.face_force(g["be11"], g["be12"], g["be22"], g["phi"], E.G, E.W_T, E.DX, E.DY)[4]
    rhs = M.imex_elastic_rhs(g["u"], g["v"], E.DX, E.DY, E.DT, E.CS2, chi, g["fu"], g["fv"], E.RHO)
    assert same_bits(np.stack(rhs), ops[k + "_rhs"])
    ny, nx = shape
    le = M.lap_eigs_periodic(nx, ny, E.DX, E.DY)
    got = np.stack(M.momentum_predictor_periodic_imex_elastic(
        g["u"], g["v"], E.NU, E.DX, E.DY, E.DT, le, E.CS2, chi, g["fu"], g["fv"], E.RHO))
    ref = _ref(ops, shape, "pred", lambda: NP.predictor_imex_elastic(
        g["u"], g["v"], E.NU, E.DX, E.DY, E.DT, le, E.CS2, chi, g["fu"], g["fv"], E.RHO))
    for c, name in enumerate(("u*", "v*")):
        d = np.abs(got[c] - ref[c]).max() / np.abs(ref[c]).max()
        print(f"elastic IMEX predictor {shape} {name}: {d:.3e} of max-abs (bar {E.FFT_REL:g})")
        assert d <= E.FFT_REL


@pytest.mark.parametrize("shape", [(5, 7), (33, 70)], ids=E.key)
def test_chi_one_no_force_is_the_imex_predictor(M, shape):
    """chi = 1, fu = fv = 0: the bits of momentum_predictor_periodic_imex's entry at
    coef = dt nu + c_el."""
    import torch
    from pyrmt_amd import _lib as L
    from pyrmt_amd.functions import _p
    g = E.op_inputs(shape)
    ny, nx = shape
    le = M.lap_eigs_periodic(nx, ny, E.DX, E.DY)
    one, zero = np.ones(shape), np.zeros(shape)
    got = M.momentum_predictor_periodic_imex_elastic(g["u"], g["v"], E.NU, E.DX, E.DY, E.DT, le,
                                                     E.CS2, one, zero, zero, E.RHO)
    lx, ly = M._axis_eigs_per(le, False)
    u, v = _dev(g["u"], g["v"])
    us, vs = torch.empty_like(u), torch.empty_like(v)
    coef = E.DT * E.NU + E.DT * E.DT * E.CS2
    L.check(L.lib().rmt_mac_per_predictor_imex(M._pctx(shape, True), _p(u), _p(v), 2 * E.DX,
                                               2 * E.DY, E.DT, coef, M._hp(lx), M._hp(ly), _p(us),
                                               _p(vs)))
    assert same_bits(np.stack(got), _host([us, vs]))


# -------------------------------------------------------------------------- lock --
@pytest.mark.parametrize("shape", E.SHAPES, ids=E.key)
def test_lock(M, ops, shape):
    g, k = E.op_inputs(shape), E.key(shape)
    ff = NP.face_force(g["be11"], g["be12"], g["be22"], g["phi"], E.G, E.W_T, E.DX, E.DY)
    comp = ((g["us"], g["u"], g["fu"], ff[2], g["um"]), (g["vs"], g["v"], g["fv"], ff[3], g["vm"]))
    lock = lambda mode, beta=E.BETA: np.stack([M.ve_lock(*c, E.DT, beta, E.RHO, mode)
                                               for c in comp])
    assert same_bits(lock("explicit"), ops[k + "_lock_explicit"])
    for mode in ("imex", "imex-elastic"):
        ref = _ref(ops, shape, "lock_" + mode, lambda: [
            NP.lock(*c, E.DT, E.BETA, E.RHO, mode) for c in comp])
        close(lock(mode), ref, "lock_" + mode, f"lock {mode} {shape}")
    # beta = 0: the explicit lock is u* + dt f / rho exactly; the exact one multiplies by
    # exp(-0.0) = 1
    want = np.stack([c[0] + E.DT * c[2] / E.RHO for c in comp])
    assert same_bits(lock("explicit", 0.0), want)
    assert same_bits(lock("imex", 0.0), np.stack([c[4] + (w - c[4]) for c, w in zip(comp, want)]))
    assert same_bits(lock("imex-elastic", 0.0),
                     np.stack([c[4] + (c[0] - c[4]) for c in comp]))


# ------------------------------------------------------------------------ record --
TRIP = 256 * 256      # the reduction's constant launch (mac_ve.hip VR_RB x VR_T)


def _record_case(name):
    if name == "trip2":     # the last cell is read on a workgroup's second trip
        shape = (TRIP + 1,)
        k = np.arange(TRIP + 1, dtype=np.float64)
        g = dict(be11=1.0 + (k % 13) * 0.125, be12=(k % 7) * 0.0625, be22=1.0 + (k % 5) * 0.25,
                 phi=np.where(k % 3 == 0, -0.5, 0.5), u=((k % 17) - 8.0) * 0.125)
        g["be11"][-1] = 40.0; g["phi"][-1] = -1.0; g["u"][-1] = -77.0
        return g, TRIP
    g = {k: v.copy() for k, v in E.op_inputs((33, 70)).items()
         if k in ("be11", "be12", "be22", "phi", "u")}
    if name == "nan_u":
        g["u"][32, 69] = np.nan
    elif name == "inf_u":
        g["u"][0, 0] = -np.inf
    elif name == "inf_be":
        g["be22"][0, 0] = np.inf         # a solid cell
    elif name == "nan_be_fluid":
        g["be11"][32, 69] = np.nan       # a fluid cell: not in the maximum
    elif name == "nan_be_solid":
        g["be12"][0, 1] = np.nan
    elif name == "no_solid":
        g["phi"] = np.abs(g["phi"]) + 0.125
    return g, 16 * 70 + 35


@pytest.mark.parametrize("name", ["plain", "nan_u", "inf_u", "inf_be", "nan_be_fluid",
                                  "nan_be_solid", "no_solid", "trip2"])
def test_record_reduction_bitwise(M, ops, name):
    g, at = _record_case(name)
    got = M.ve_record(g["be11"], g["be12"], g["be22"], g["phi"], g["u"], at)
    ref = NP.record(g["be11"], g["be12"], g["be22"], g["phi"], g["u"], at)
    print(f"record {name}: {got}")
    assert got.shape == (5,)
    eq(got, ref)                      # (NaN == NaN here; the bits of a NaN are not pinned)
    if name == "plain":
        eq(got, ops["33x70_record"])
    if name == "no_solid":
        assert got[0] == -np.inf and got[1] == 0.0
    if name in ("nan_u", "inf_u"):
        assert got[4] == 0.0 and (np.isnan(got[3]) if name == "nan_u" else got[3] == np.inf)
    if name == "trip2":
        assert got[0] >= 40.0 and got[3] == 77.0


# -------------------------------------------------------------------- short runs --
def _cases():
    return [(E.short_key(*c), E.short_kwargs(*c), E.SHORT_STEPS) for c in E.short_cases()] + [
        (E.LARGE["key"], E.large_kwargs(), E.LARGE["steps"])]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_short_runs(M, runs, case):
    """Step count, t and dt ==; the per-step record and the final planes within 4 x floor."""
    k, kw, nsteps = case
    kw = dict(kw)
    t_end = kw.pop("t_end")
    t, hist, sim = M.mac_ve_extension_run(t_end=t_end, return_sim=True, **kw)
    rec, ref = np.array(sim.record), runs[k + "_record"]
    assert sim.nsteps == nsteps == len(ref) and not sim.stopped
    assert type(t) is float and t == ref[-1, 0]
    eq(rec[:, 0], ref[:, 0]); eq(np.array(sim.dts), runs[k + "_dts"])
    assert len(hist) == 1 and hist[0] == sim.record[-1]
    for c, q in ((1, "lam"), (2, "bxx"), (3, "umax")):
        close(rec[:, c], ref[:, c], f"{k}_{q}")
    state = dict(u=sim.get("u"), v=sim.get("v"), X1=sim.get("X1"), X2=sim.get("X2"),
                 phi=sim.get("phi"), psi=np.stack([sim.get(n) for n in ("p11", "p12", "p22")]),
                 be=np.stack([sim.get(n) for n in ("be11", "be12", "be22")]))
    assert int((state["phi"] <= 0).sum()) == runs[k + "_cells"][-1]
    for name in E.STATE:
        close(state[name], runs[f"{k}_{name}"], f"{k}_{name}")


def test_strang_without_relaxation_is_the_explicit_stepper(M):
    """tau = 0 (inf) under "imex": the Strang path has no relaxation to do and gives the bits of
    the explicit stepper on the same inputs -- the planes of a driver mid-run."""
    from pyrmt_amd import viscoelastic as VE
    kw = dict(E.short_kwargs(24, "imex", 0.0))
    t_end = kw.pop("t_end")
    sim = M.MacViscoelasticExtension(**kw).step(5, t_end)
    assert sim.tau == math.inf and sim.imex and sim.nsteps == 5
    psi = sim.psi
    Lc = [sim.kin[c] for c in (2, 3, 4, 5)]
    a = VE.logconf_local_step_strang(*psi, *Lc, sim.tau, sim.dt)
    b = VE.logconf_local_step(*psi, *Lc, sim.tau, sim.dt)
    assert same_bits(_host(a), _host(b)) and float(abs(a[0]).max()) > 0.0


# ------------------------------------------- the reference's five checks at N = 40 --
_long = {}


def _long_run(M, name):
    if name not in _long:
        kw = dict(E.LONG_CFG, **E.LONG[name]) if name in E.LONG else dict(E.SAT_CFG,
                                                                           **E.SAT[name])
        t, hist, sim = M.mac_ve_extension_run(return_sim=True, **kw)
        _long[name] = (t, hist, sim, kw["t_end"])
        print(f"{name}: {sim.nsteps} steps, t = {t!r}, stopped = {sim.stopped} "
              f"({sim.clause}), last {hist[-1] if hist else None}")
    return _long[name]


def _bxx(M, runs, name, bar):
    """The device's final b_xx of a run that reaches the end: within a tenth of the check's bar
    of the reference's recorded value (the port may not use up the slack the reference's test
    leaves for the method), with the reference's step count and t."""
    t, hist, sim, t_end = _long_run(M, name)
    r = runs["long_" + name]
    assert E.reached(hist, t_end) and r[0] == 1.0
    assert sim.nsteps == r[1] and t == r[2]
    b, d = hist[-1][2], abs(hist[-1][2] - r[5]) / r[5]
    print(f"{name}: b_xx(centre) {b!r}, reference {r[5]!r}, relative distance {d:.3e} "
          f"(bar {0.1 * bar:g})")
    assert d <= 0.1 * bar
    return b


def _diverges(M, runs, name):
    """A run that blows up: it ends by the loop's own stop test, not at t_end, as the CPU
    restatement predicts (tests/test_mac_ve_extension_cpu.py: step and clause)."""
    t, hist, sim, t_end = _long_run(M, name)
    r = runs["long_" + name]
    print(f"{name}: stopped at step {sim.nsteps} by {sim.clause!r}; the reference at step "
          f"{int(r[1])}, the restatement by {E.DIVERGING[name]!r}")
    assert sim.stopped and not E.reached(hist, t_end) and r[0] == 0.0
    assert sim.clause in ("non-finite u", "lam_max > 1e4", "no solid cell")


def test_imex_fsi_reproduces_explicit_at_matched_dt(M, runs):
    be, bi = _bxx(M, runs, "fsi_explicit", 0.03), _bxx(M, runs, "fsi_imex", 0.03)
    print(f"IMEX vs explicit rel diff {abs(bi - be) / be:.3e} (bar 0.03)")
    assert abs(bi - be) / be < 0.03


def test_imex_fsi_stable_where_explicit_diverges(M, runs):
    br = _bxx(M, runs, "fsi_explicit", 0.03)
    _diverges(M, runs, "fsi_explicit_3x")
    bi = _bxx(M, runs, "fsi_imex_3x", 0.06)
    print(f"IMEX at 3 x the viscous step vs explicit rel diff {abs(bi - br) / br:.3e} (bar 0.06)")
    assert np.isfinite(bi) and abs(bi - br) / br < 0.06


def test_elastic_imex_consistent_at_small_dt(M, runs):
    br, be = _bxx(M, runs, "el_explicit", 0.025), _bxx(M, runs, "el_elastic_small", 0.025)
    print(f"elastic IMEX vs explicit rel diff {abs(be - br) / br:.3e} (bar 0.025)")
    assert abs(be - br) / br < 0.025


def test_elastic_imex_lifts_elastic_cfl(M, runs):
    _diverges(M, runs, "el_imex_8x")
    t, hist, sim, t_end = _long_run(M, "el_elastic_8x")
    r = runs["long_el_elastic_8x"]
    assert E.reached(hist, t_end) and np.isfinite(hist[-1][2])
    assert sim.nsteps == r[1] and t == r[2]
    print(f"el_elastic_8x: b_xx(centre) {hist[-1][2]!r}, reference {r[5]!r}, relative distance "
          f"{abs(hist[-1][2] - r[5]) / r[5]:.3e}")


def test_compare_integrators_table(M, runs):
    """compare_integrators at a short horizon: the table's shape, and the regression row equal
    to two plain runs."""
    tab = M.compare_integrators(N=24, t_end=0.05)
    assert sorted(tab) == ["dt_elastic", "dt_visc", "explicit_bxx", "imex_bxx", "rel", "rows"]
    assert tab["dt_visc"] == 0.2 * (1.0 / 24) * (1.0 / 24) / 0.05
    assert [r[0] for r in tab["rows"]] == [2, 3, 4] and all(len(r) == 5 for r in tab["rows"])
    _, h = M.mac_ve_extension_run(N=24, t_end=0.05, dt=tab["dt_visc"])
    assert h[-1][2] == tab["explicit_bxx"] and tab["rel"] < 0.03


# -------------------------------------------------------------------- saturation --
def test_saturation(M, runs):
    """N = 32, tau = 0.5 (Wi = 0.25): b_xx(centre) against 1 / (1 - 2 Wi) = 2.  t_end and the
    bar are the reference's own: under "imex" at t_end = 4 (mac_ve_extension_np.SAT: with the
    default explicit integrator the reference's run ends at t = 0.5) its b_xx(centre) lies
    a relative e_ref from the analytic value; the device's distance may exceed e_ref by a tenth
    of it at most."""
    t, hist, sim, t_end = _long_run(M, "sat_imex")
    r = runs["long_sat_imex"]
    assert sim.Wi == 0.25 and sim.bxx_analytic == 2.0
    assert E.reached(hist, t_end) and r[0] == 1.0 and sim.nsteps == r[1] and t == r[2]
    e_ref = abs(r[5] - 2.0) / 2.0
    e = abs(hist[-1][2] - 2.0) / 2.0
    print(f"saturation: b_xx(centre) {hist[-1][2]!r} (reference {r[5]!r}), distance from "
          f"1 / (1 - 2 Wi): {e:.4f}, the reference's {e_ref:.4f}")
    assert e <= 1.1 * e_ref
    t, hist, sim, t_end = _long_run(M, "sat_explicit")
    assert sim.stopped and not E.reached(hist, t_end) and runs["long_sat_explicit"][0] == 0.0
