"""The oracle at dx != dy (no GPU): oracle/mac_oracle.py and tests/mac_freeslip_np.py against the
reference's own results on square grids over non-square boxes (tests/golden/mac_lid_aniso.npz,
made by tests/golden/gen_mac_lid_aniso.py), bit for bit -- the bars tests/test_oracle_golden.py
holds the same functions to at dx == dy.  That lets tests/test_gpu_mac_lid_aniso.py use the
oracle at sizes the fixture does not hold.

The second half checks the cases that GPU file runs against the oracle (tables in
tests/mac_lid_aniso_np.py), on the CPU: every CG / PCG solve's stopping test is decided with a
margin (||r|| / atol >= 1.05 on the trips that run, <= 0.95 where it stops, from a
residual-recording copy of the oracle's cg_x0), so that an equal iteration count is a fair
demand of the kernels; and the oracle's response to a one-ulp change of one input value stays a
tenth below the bar each case is held to.
"""
import numpy as np
import pytest

import mac_freeslip_np as FS
import mac_lid_aniso_np as A
from conftest import golden


@pytest.fixture(scope="module")
def MO():
    from oracle import mac_oracle
    return mac_oracle


_eq = np.testing.assert_array_equal
GRIDS = [g[0] for g in A.FIXTURE_GRIDS]


@pytest.mark.parametrize("N, box", A.FIXTURE_GRIDS)
def test_fixture_grid(N, box):
    g = A.fixture(golden, N)
    assert (g["dx"], g["dy"]) == A.spacing(N, box) and g["dx"] != g["dy"]
    for k in ("noise_pu", "noise_pv", "noise_pp", "noise_cg_u", "noise_cg_v", "noise_pcg_u",
              "noise_pcg_v", "noise_ix0", "noise_ix1", "noise_ixfu", "noise_ixfv", "noise_sl0",
              "noise_sl1"):
        assert 0.0 <= g[k] <= 0.1 * A.BAR_FIXTURE, (k, g[k])
    nz = g["txx"] != 0
    assert nz[1:-1, 1:-1].any() and nz[0].any() and nz[:, 0].any()


@pytest.mark.parametrize("N", GRIDS)
def test_operators_bitwise(MO, N):
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    _eq(MO.divergence(g["u"], g["v"], dx, dy), g["div"])
    _eq(MO.gradient_p_u(g["p"], dx), g["gpu"])
    _eq(MO.gradient_p_v(g["p"], dy), g["gpv"])
    base = (g["u"], g["v"], A.NU, dx, dy, A.DT)
    forces = dict(fu=g["fu"], fv=g["fv"], rho=A.RHO)
    for tag, kw in (("0", {}), ("1", forces)):
        us, vs = MO.momentum_predictor(*base, A.U_LID, **kw)
        _eq(us, g["mp_us" + tag]); _eq(vs, g["mp_vs" + tag])
        us, vs = FS.momentum_predictor_freeslip(*base, **kw)
        _eq(us, g["fs_us" + tag]); _eq(vs, g["fs_vs" + tag])
    gu, gv = FS.interfacial_force_faces(g["kappa"], g["H"], A.GAMMA, dx, dy)
    _eq(gu, g["gu"]); _eq(gv, g["gv"])
    pa, pb = A.discs(N, dx, dy)
    _eq(pa, g["pa"]); _eq(pb, g["pb"])
    assert g["eps"] == 3 * max(dx, dy)
    for a, k in zip(MO.contact_stress(pa, pb, A.ETA, A.GSUM, g["eps"], dx, dy),
                    ("txx", "txy", "tyy")):
        _eq(a, g[k])
    _eq(MO.lap_u_lid_hom(g["u"], dx, dy), g["lap_u"])
    _eq(MO.lap_v_lid_hom(g["v"], dx, dy), g["lap_v"])
    _eq(MO.dst_helmholtz_eigs((N, N - 1), dx, dy), g["eig_u"])
    _eq(MO.dst_helmholtz_eigs((N - 1, N), dx, dy), g["eig_v"])


@pytest.mark.parametrize("N", GRIDS)
def test_projection_bitwise(MO, N):
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    eig = MO.poisson_eigs_neumann(N, N, dx, dy)
    u, v, p = MO.project(g["mp_us1"], g["mp_vs1"], dx, dy, A.DT, A.RHO, eig)
    _eq(u, g["pu"]); _eq(v, g["pv"]); _eq(p, g["pp"])
    rhs = (A.RHO / A.DT) * MO.divergence(g["mp_us1"], g["mp_vs1"], dx, dy)
    _eq(MO.solve_poisson_neumann(rhs - rhs.mean(), eig), g["pp"])


@pytest.mark.parametrize("N", GRIDS)
def test_helmholtz_bitwise(MO, N):
    g = A.fixture(golden, N)
    dx, dy, coef = g["dx"], g["dy"], float(golden("mac_lid_aniso")["coef"])
    for kind, tag in ((0, "u"), (1, "v")):
        x, _ = MO.helmholtz(g["rhs_" + tag], kind, coef, dx, dy, 1e-10, precond=False)
        _eq(x, g["cg_" + tag])
        x, it = MO.helmholtz(g["rhs_" + tag], kind, coef, dx, dy, 1e-8)
        _eq(x, g["pcg_" + tag])
        assert it == g["cnt_" + tag]


@pytest.mark.parametrize("N", GRIDS)
def test_predictors_bitwise(MO, N):
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    forces = dict(fu=g["fu"], fv=g["fv"], rho=A.RHO, cs2=A.CS2)
    lid = (g["u"], g["v"], A.NU, dx, dy, A.DT, A.U_LID)
    for tag, kw in (("0", {}), ("1", forces), ("fu", dict(fu=g["fu"], rho=A.RHO)),
                    ("fv", dict(fv=g["fv"], rho=A.RHO))):
        us, vs = MO.momentum_predictor_lid_imex(*lid, **kw)
        _eq(us, g["ix_us" + tag]); _eq(vs, g["ix_vs" + tag])
    assert g["dt_sl"] == A.semilag_dt(g["u"], g["v"], dx, dy, 3.0)
    sl = (g["u"], g["v"], A.NU, dx, dy, g["dt_sl"], A.U_LID)
    for tag, kw in (("0", {}), ("1", forces)):
        us, vs = MO.momentum_predictor_lid_semilag(*sl, **kw)
        _eq(us, g["sl_us" + tag]); _eq(vs, g["sl_vs" + tag])


# ------------------------------------------------ the oracle cases of the GPU file ----
def test_recording_cg_is_the_oracles(MO):
    """cg_x0_rec is cg_x0 with the ratios kept: same iterate, same count."""
    case = (33, "wide", 0.05, 0, 1)
    dx, dy = A.spacing(33, "wide")
    rhs = A.helm_rhs(case)
    x, it = MO.helmholtz(rhs, 0, 0.05, dx, dy, 1e-8)
    with A.Recorded(MO) as R:
        xr, itr = MO.helmholtz(rhs, 0, 0.05, dx, dy, 1e-8)
    assert MO.cg_x0 is R.orig
    _eq(x, xr)
    assert it == itr == R.solves[0][0] and len(R.solves[0][1]) == it + 1


def _helm_checked(MO, case, maxiter=500):
    N, box, coef, kind, precond = case
    dx, dy = A.spacing(N, box)
    with A.Recorded(MO) as R:
        _, nz = A.with_noise(
            lambda r: MO.helmholtz(r, kind, coef, dx, dy, A.RTOL[precond], maxiter=maxiter,
                                   precond=bool(precond)), (A.helm_rhs(case),), 0)
    for it, ratios, mx in R.solves:
        assert A.margin_ok(ratios, it, mx), (A.helm_id(case), it, ratios[max(0, it - 1):])
    assert R.solves[0][0] == R.solves[1][0]
    assert nz <= 0.1 * A.helm_bar(case), (A.helm_id(case), nz)
    return R.solves[0][0]


@pytest.mark.parametrize("N", A.HELM_N + (516,))
def test_helmholtz_cases_margin_and_noise(MO, N):
    cases = [c for c in A.helm_cases() + A.HELM_BIG if c[0] == N]
    assert len(cases) == (2 if N == 516 else 24)
    for case in cases:
        it = _helm_checked(MO, case)
        assert 0 < it < 500


def test_plan_cache_and_early_exit_cases(MO):
    for kind in (0, 1):
        for N, dx, dy, coef, rhs, _ in A.cache_sequence(kind):
            with A.Recorded(MO) as R:
                _, nz = A.with_noise(lambda r: MO.helmholtz(r, kind, coef, dx, dy, 1e-8), (rhs,), 0)
            assert R.all_ok() and nz <= 0.1 * A.BAR_ORACLE
        # a capped maxiter: the loop must still be running where it is cut (ratios far above 1)
        dx, dy = A.spacing(A.EXIT_N, A.EXIT_BOX)
        for precond in (0, 1):
            for cap in (1, 2, 3):
                with A.Recorded(MO) as R:
                    _, nz = A.with_noise(
                        lambda r: MO.helmholtz(r, kind, A.EXIT_COEF, dx, dy, A.RTOL[precond],
                                               maxiter=cap, precond=bool(precond)),
                        (A.exit_rhs(kind),), 0)
                assert all(it == cap and min(ratios) > 100 for it, ratios, _ in R.solves)
                assert nz <= 0.1 * A.BAR_ORACLE
    # the two exits that run no trip
    z, it = MO.helmholtz(np.zeros((33, 32)), 0, 0.05, dx, dy, 1e-8)
    assert it == 0 and not z.any()
    x, it = MO.helmholtz(A.exit_rhs(0), 0, 0.05, dx, dy, 1e-8, maxiter=0)
    assert it == 0
    _eq(x, A.exit_rhs(0))


@pytest.mark.parametrize("which", ["imex", "semilag"])
def test_predictor_cases_margin_and_noise(MO, which):
    if which == "imex":
        cases, inputs, fn = A.pred_cases(), A.imex_inputs, MO.momentum_predictor_lid_imex
    else:
        cases, inputs, fn = A.semilag_cases(), A.semilag_inputs, MO.momentum_predictor_lid_semilag
    for case in cases:
        args, kw = inputs(case)
        u, v, dx, dy, dt = args[0], args[1], args[3], args[4], args[5]
        cfl = dt * max(np.abs(u).max() / dx, np.abs(v).max() / dy)
        if which == "semilag":
            assert abs(cfl - case[3]) < 1e-12 and (cfl > 0.9) == (case[3] == 4.0)
        with A.Recorded(MO) as R:
            _, nz = A.with_noise(fn, args, 0, kw)
        assert len(R.solves) == 4 and R.all_ok(), (which, case)
        assert [s[0] for s in R.solves[:2]] == [s[0] for s in R.solves[2:]]
        assert nz <= 0.1 * A.pred_bar(which, case[:3]), (which, case, nz)


@pytest.mark.parametrize("N", A.PROJ_N)
def test_projection_cases_noise(MO, N):
    for box in A.BOXES:
        dx, dy = A.spacing(N, box)
        us, vs = A.project_inputs(MO, N, box)
        for ddx, ddy in ((dx, dy), (dy, dx)):
            (u, v, p), nz = A.with_noise(
                MO.project, (us, vs, ddx, ddy, A.DT, A.RHO,
                             MO.poisson_eigs_neumann(N, N, ddx, ddy)), 0)
            assert nz <= 0.1 * A.BAR_PROJECT, (N, box, nz)
            assert np.abs(MO.divergence(u, v, ddx, ddy)).max() < 1e-9
