"""GPU parity of the lid-tier MAC operators (mac.hip) and the IMEX tier (imex.hip) at dx != dy:
square grids over non-square boxes, dx, dy = mac_grid(N, N, Lx, Ly), which _lid_n accepts and
every other lid-tier test leaves out (they all run dx == dy).  A dx taken for a dy (or dx**2 for
dy**2) at a host call site, in imex_plan's eigenvalues, in the lid term, in the backtrace or in
the projection's correction passes every one of those; it fails here.

Against the reference's fixture (tests/golden/mac_lid_aniso.npz: N = 5, 6, 33) and, at N = 64
and 97 (and 516 once, where the grid-stride loops of k_im_apply / k_cg_dot / k_cg_xr take their
second trip), against the oracle, which tests/test_mac_lid_aniso_cpu.py pins to that fixture
bit for bit.  The projection's oracle sizes are 64 and 99: the DCT-II solve refuses the prime
97 (radices <= 23), which is asserted.

The stencil operators are bit-exact.  The solves and the implicit predictors are held to 1e-12
of the solution's scale against the fixture and 1e-11 against the oracle (the projection: 1e-12
everywhere), each bar only where the reference's own response to a one-ulp input change is a
tenth of it -- stored in the fixture as noise_*, measured here for the oracle cases (and
asserted: a larger floor would have its own bar in tests/mac_lid_aniso_np.py).  CG and PCG
iteration counts are equal: the CPU file checks that every case's stopping test is decided
with a 5 % margin.  Also here: imex_plan's cache paths and the DCT-II plan's on a changing
(dx, dy, coef), and the early exits of the CG (zero right-hand side, maxiter 0, a capped
maxiter).
"""
import numpy as np
import pytest

import mac_freeslip_np as FS
import mac_lid_aniso_np as A
from conftest import golden

pytestmark = pytest.mark.gpu
_eq = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def M(gpu):
    from pyrmt_amd import mac
    return mac


@pytest.fixture(scope="module")
def MO():
    from oracle import mac_oracle
    return mac_oracle


def _close(a, b, bar, floor=0.0):
    """max|a - b| <= bar * max(floor, max|b|)."""
    a, b = np.asarray(a), np.asarray(b)
    scale = max(np.abs(b).max(), floor, 1e-300)
    assert np.abs(a - b).max() <= bar * scale, (np.abs(a - b).max() / scale, bar)


def _fixture_bar(g, *names):
    """1e-12 where the stored noise floor is a tenth of it, else ten times the floor."""
    nz = max(g["noise_" + n] for n in names)
    return A.BAR_FIXTURE if nz <= 0.1 * A.BAR_FIXTURE else 10.0 * nz


def _oracle(fn, args, kw, bar):
    """The oracle's result, with its one-ulp response (args[0] nudged) a tenth below bar."""
    ref, nz = A.with_noise(fn, args, 0, kw)
    assert nz <= 0.1 * bar, (nz, bar)
    return ref


# ---------------------------------------------------------------- bit-exact operators ----
OPS = ("div", "gpu", "gpv", "mp_us0", "mp_vs0", "mp_us1", "mp_vs1", "fs_us0", "fs_vs0", "fs_us1",
       "fs_vs1", "gu", "gv", "txx", "txy", "tyy", "lap_u", "lap_v", "eig_u", "eig_v")


def _ops(m, fs, d, N, dx, dy, names):
    """Every stencil operator of module m (free-slip pair: fs) on the inputs d."""
    o = {}
    o["div"] = m.divergence(d["u"], d["v"], dx, dy)
    o["gpu"] = m.gradient_p_u(d["p"], dx)
    o["gpv"] = m.gradient_p_v(d["p"], dy)
    base = (d["u"], d["v"], A.NU, dx, dy, A.DT)
    forces = dict(fu=d["fu"], fv=d["fv"], rho=A.RHO)
    for tag, kw in (("0", {}), ("1", forces)):
        o["mp_us" + tag], o["mp_vs" + tag] = m.momentum_predictor(*base, A.U_LID, **kw)
        o["fs_us" + tag], o["fs_vs" + tag] = fs.momentum_predictor_freeslip(*base, **kw)
    o["gu"], o["gv"] = fs.interfacial_force_faces(d["kappa"], d["H"], A.GAMMA, dx, dy)
    pa, pb = A.discs(N, dx, dy)
    o["txx"], o["txy"], o["tyy"] = m.contact_stress(pa, pb, A.ETA, A.GSUM, 3 * max(dx, dy), dx, dy)
    o["lap_u"] = getattr(m, names[0])(d["u"], dx, dy)
    o["lap_v"] = getattr(m, names[1])(d["v"], dx, dy)
    o["eig_u"] = getattr(m, names[2])((N, N - 1), dx, dy)
    o["eig_v"] = getattr(m, names[2])((N - 1, N), dx, dy)
    return o


GPU_NAMES = ("_lap_u_lid_hom", "_lap_v_lid_hom", "_dst_helmholtz_eigs")
ORACLE_NAMES = ("lap_u_lid_hom", "lap_v_lid_hom", "dst_helmholtz_eigs")


def _walls_zero(us, vs):
    assert not us[:, 0].any() and not us[:, -1].any() and not vs[0].any() and not vs[-1].any()


@pytest.mark.parametrize("N, box", A.FIXTURE_GRIDS)
def test_operators_bitwise_vs_reference(M, N, box):
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    assert (dx, dy) == M.mac_grid(N, N, *A.BOXES[box]) and dx != dy
    o = _ops(M, M, g, N, dx, dy, GPU_NAMES)
    for k in OPS:
        _eq(o[k], g[k], err_msg=k)
    for a, b in (("mp_us0", "mp_vs0"), ("mp_us1", "mp_vs1"), ("fs_us0", "fs_vs0"),
                 ("fs_us1", "fs_vs1"), ("gu", "gv")):
        _walls_zero(o[a], o[b])
    assert np.count_nonzero(o["txx"]) > 0


@pytest.mark.parametrize("box", list(A.BOXES))
@pytest.mark.parametrize("N", A.ORACLE_N)
def test_operators_bitwise_vs_oracle_and_swap(M, MO, N, box):
    """The same operators at N = 64, 97 against the oracle, then once more with the two
    spacings exchanged on the same inputs: every output changes (the case is sensitive to the
    swap) and equals the oracle's at the exchanged spacings."""
    d = A.op_inputs(N, A.op_seed(N, box))
    dx, dy = A.spacing(N, box)
    first = _ops(M, M, d, N, dx, dy, GPU_NAMES)
    ref = _ops(MO, FS, d, N, dx, dy, ORACLE_NAMES)
    for k in OPS:
        _eq(first[k], ref[k], err_msg=k)
    nz = ref["txx"] != 0
    assert nz[1:-1, 1:-1].any() and nz[0].any() and nz[:, 0].any()
    swapped = _ops(M, M, d, N, dy, dx, GPU_NAMES)
    ref = _ops(MO, FS, d, N, dy, dx, ORACLE_NAMES)
    for k in OPS:
        assert not np.array_equal(swapped[k], first[k]), k
        _eq(swapped[k], ref[k], err_msg=k)


def test_device_tensors_in_device_tensors_out(M):
    import torch
    g = A.fixture(golden, 33)
    dx, dy = g["dx"], g["dy"]
    dev = {k: torch.from_numpy(g[k]).cuda() for k in ("u", "v", "fu", "fv", "p")}
    us, vs = M.momentum_predictor(dev["u"], dev["v"], A.NU, dx, dy, A.DT, A.U_LID, fu=dev["fu"],
                                  fv=dev["fv"], rho=A.RHO)
    div = M.divergence(dev["u"], dev["v"], dx, dy)
    ix, iv = M.momentum_predictor_lid_imex(dev["u"], dev["v"], A.NU, dx, dy, A.DT, A.U_LID)
    for t in (us, vs, div, ix, iv):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
    _eq(us.cpu().numpy(), g["mp_us1"]); _eq(vs.cpu().numpy(), g["mp_vs1"])
    _eq(div.cpu().numpy(), g["div"])
    _close(ix.cpu().numpy(), g["ix_us0"], _fixture_bar(g, "ix0"))
    _close(iv.cpu().numpy(), g["ix_vs0"], _fixture_bar(g, "ix0"))


# ---------------------------------------------------------------- projection ----
def _check_projection(M, got, ref, dx, dy):
    u, v, phi = got
    _close(phi, ref[2], A.BAR_PROJECT)
    _close(u, ref[0], A.BAR_PROJECT, 1.0)
    _close(v, ref[1], A.BAR_PROJECT, 1.0)
    assert np.abs(M.divergence(u, v, dx, dy)).max() < 1e-9


def test_projection_vs_reference(M):
    N = 33
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    assert max(g["noise_pu"], g["noise_pv"], g["noise_pp"]) <= 0.1 * A.BAR_PROJECT
    got = M.project(g["mp_us1"], g["mp_vs1"], dx, dy, A.DT, A.RHO,
                    M.poisson_eigs_neumann(N, N, dx, dy))
    _check_projection(M, got, (g["pu"], g["pv"], g["pp"]), dx, dy)


def test_projection_refuses_prime_97(M, MO):
    """N = 97, the odd size of the other oracle cases, is outside the DCT-II solve's domain (a
    prime factor above 23): project and solve_poisson_neumann say so, they do not fall back."""
    N = 97
    dx, dy = A.spacing(N, "wide")
    us, vs = A.project_inputs(MO, N, "wide")
    eig = M.poisson_eigs_neumann(N, N, dx, dy)
    with pytest.raises(NotImplementedError, match="radices <= 23"):
        M.project(us, vs, dx, dy, A.DT, A.RHO, eig)
    with pytest.raises(NotImplementedError, match="radices <= 23"):
        M.solve_poisson_neumann(us[:, 1:], eig)


@pytest.mark.parametrize("box", list(A.BOXES))
@pytest.mark.parametrize("N", A.PROJ_N)
def test_projection_vs_oracle_and_plan_cache(M, MO, N, box):
    """project at (dx, dy), at (dy, dx) and at (dx, dy) again on one context: each against the
    oracle (a stale lamx / lamy of the DCT-II plan would show), the third the first's bits; then
    the same three calls through solve_poisson_neumann."""
    dx, dy = A.spacing(N, box)
    us, vs = A.project_inputs(MO, N, box)
    got = []
    for ddx, ddy in ((dx, dy), (dy, dx), (dx, dy)):
        ref = _oracle(MO.project, (us, vs, ddx, ddy, A.DT, A.RHO,
                                   MO.poisson_eigs_neumann(N, N, ddx, ddy)), None, A.BAR_PROJECT)
        got.append(M.project(us, vs, ddx, ddy, A.DT, A.RHO, M.poisson_eigs_neumann(N, N, ddx, ddy)))
        _check_projection(M, got[-1], ref, ddx, ddy)
    assert not np.array_equal(got[1][2], got[0][2])
    for a, b in zip(got[0], got[2]):
        _eq(a, b)
    rhs = np.random.default_rng(A.op_seed(N, box) + 1).standard_normal((N, N))
    rhs -= rhs.mean()
    sol = []
    for ddx, ddy in ((dx, dy), (dy, dx), (dx, dy)):
        (ref,) = _oracle(MO.solve_poisson_neumann,
                         (rhs, MO.poisson_eigs_neumann(N, N, ddx, ddy)), None, A.BAR_PROJECT)
        sol.append(M.solve_poisson_neumann(rhs, M.poisson_eigs_neumann(N, N, ddx, ddy)))
        _close(sol[-1], ref, A.BAR_PROJECT)
    assert not np.array_equal(sol[1], sol[0])
    _eq(sol[0], sol[2])


# ---------------------------------------------------------------- Helmholtz ----
def _embed_lap(M, kind, dx, dy):
    if kind == 0:
        return (lambda w: M._lap_u_lid_hom(w, dx, dy)), (lambda x: np.pad(x, ((0, 0), (1, 1))))
    return (lambda w: M._lap_v_lid_hom(w, dx, dy)), (lambda x: np.pad(x, ((1, 1), (0, 0))))


@pytest.mark.parametrize("N", [g[0] for g in A.FIXTURE_GRIDS])
def test_cg_pcg_vs_reference(M, N):
    """The public _cg_helmholtz / _pcg_helmholtz (the operator handed over as the reference's
    lambdas) against the reference's own solves, the PCG counts equal."""
    g = A.fixture(golden, N)
    dx, dy, coef = g["dx"], g["dy"], float(golden("mac_lid_aniso")["coef"])
    for kind, tag in ((0, "u"), (1, "v")):
        lap, emb = _embed_lap(M, kind, dx, dy)
        _close(M._cg_helmholtz(g["rhs_" + tag], lap, emb, coef), g["cg_" + tag],
               _fixture_bar(g, "cg_" + tag))
        cnt = []
        x = M._pcg_helmholtz(g["rhs_" + tag], lap, emb, coef, dx, dy, rtol=1e-8, count=cnt)
        _close(x, g["pcg_" + tag], _fixture_bar(g, "pcg_" + tag))
        assert cnt[0] == g["cnt_" + tag]


def _helm_case(M, MO, case):
    N, box, coef, kind, precond = case
    dx, dy = A.spacing(N, box)
    rhs = A.helm_rhs(case)
    bar = A.helm_bar(case)
    oracle = lambda r: MO.helmholtz(r, kind, coef, dx, dy, A.RTOL[precond], precond=bool(precond))
    (xo,) = _oracle(oracle, (rhs,), None, bar)
    _, ito = oracle(rhs)
    x, it = M._solve_helmholtz(rhs, kind, coef, dx, dy, A.RTOL[precond], 500, precond)
    print(f"{A.helm_id(case)}: {it} iterations (oracle {ito}), rel {A.rel(x, xo):.3g}")
    assert it == ito, A.helm_id(case)
    _close(x, xo, bar)


@pytest.mark.parametrize("box", list(A.BOXES))
@pytest.mark.parametrize("N", A.HELM_N)
def test_helmholtz_vs_oracle(M, MO, N, box):
    """CG and PCG, both face kinds, coef 2e-5, 0.5e-3, 0.05: solution and iteration count."""
    cases = [c for c in A.helm_cases() if c[:2] == (N, box)]
    assert len(cases) == 12
    for case in cases:
        _helm_case(M, MO, case)


def test_helmholtz_grid_stride_second_trip(M, MO):
    """N = 516: 516 * 515 interior values against the 262144 threads of k_im_apply, k_cg_dot and
    k_cg_xr, so their loops run a second trip."""
    for case in A.HELM_BIG:
        assert case[0] * (case[0] - 1) > 1024 * 256
        _helm_case(M, MO, case)


@pytest.mark.parametrize("kind", [0, 1])
def test_imex_plan_cache_paths(M, MO, kind):
    """One context per N, one plan per kind: cold, exact hit, new coef and exchanged spacings on
    the kept plan, another N in between, and back -- a stale denom would show against the
    oracle; what repeats, repeats bit for bit."""
    got = []
    for N, dx, dy, coef, rhs, same in A.cache_sequence(kind):
        oracle = lambda r: MO.helmholtz(r, kind, coef, dx, dy, 1e-8)
        (xo,) = _oracle(oracle, (rhs,), None, A.BAR_ORACLE)
        x, it = M._solve_helmholtz(rhs, kind, coef, dx, dy, 1e-8, 500, 1)
        assert it == oracle(rhs)[1]
        _close(x, xo, A.BAR_ORACLE)
        if same is not None:
            _eq(x, got[same])
        got.append(x)
    assert not np.array_equal(got[2], got[3])


@pytest.mark.parametrize("kind", [0, 1])
def test_helmholtz_early_exits(M, MO, kind):
    dx, dy = A.spacing(A.EXIT_N, A.EXIT_BOX)
    rhs = A.exit_rhs(kind)
    for precond in (0, 1):
        x, it = M._solve_helmholtz(np.zeros_like(rhs), kind, A.EXIT_COEF, dx, dy, 1e-8, 500, precond)
        assert it == 0 and not x.any()
        x, it = M._solve_helmholtz(rhs, kind, A.EXIT_COEF, dx, dy, 1e-8, 0, precond)
        assert it == 0
        _eq(x, rhs)
        for cap in (1, 2, 3):
            oracle = lambda r: MO.helmholtz(r, kind, A.EXIT_COEF, dx, dy, A.RTOL[precond],
                                            maxiter=cap, precond=bool(precond))
            (xo,) = _oracle(oracle, (rhs,), None, A.BAR_ORACLE)
            assert oracle(rhs)[1] == cap
            x, it = M._solve_helmholtz(rhs, kind, A.EXIT_COEF, dx, dy, A.RTOL[precond], cap,
                                       precond)
            assert it == cap
            _close(x, xo, A.BAR_ORACLE)
            assert not np.array_equal(x, rhs)


# ---------------------------------------------------------------- implicit predictors ----
@pytest.mark.parametrize("N", [g[0] for g in A.FIXTURE_GRIDS])
def test_predictors_vs_reference(M, N):
    g = A.fixture(golden, N)
    dx, dy = g["dx"], g["dy"]
    forces = dict(fu=g["fu"], fv=g["fv"], rho=A.RHO, cs2=A.CS2)
    lid = (g["u"], g["v"], A.NU, dx, dy, A.DT, A.U_LID)
    for tag, kw in (("0", {}), ("1", forces), ("fu", dict(fu=g["fu"], rho=A.RHO)),
                    ("fv", dict(fv=g["fv"], rho=A.RHO))):
        us, vs = M.momentum_predictor_lid_imex(*lid, **kw)
        bar = _fixture_bar(g, "ix" + tag)
        _close(us, g["ix_us" + tag], bar); _close(vs, g["ix_vs" + tag], bar)
        _walls_zero(us, vs)
    sl = (g["u"], g["v"], A.NU, dx, dy, g["dt_sl"], A.U_LID)
    for tag, kw in (("0", {}), ("1", forces)):
        us, vs = M.momentum_predictor_lid_semilag(*sl, **kw)
        bar = _fixture_bar(g, "sl" + tag)
        _close(us, g["sl_us" + tag], bar); _close(vs, g["sl_vs" + tag], bar)
        _walls_zero(us, vs)


@pytest.mark.parametrize("box", list(A.BOXES))
@pytest.mark.parametrize("N", A.ORACLE_N)
def test_imex_predictor_vs_oracle(M, MO, N, box):
    """Plain, with fu + fv + rho + cs2, and with one face force only."""
    for case in A.pred_cases():
        if case[:2] != (N, box):
            continue
        args, kw = A.imex_inputs(case)
        bar = A.pred_bar("imex", case)
        uo, vo = _oracle(MO.momentum_predictor_lid_imex, args, kw, bar)
        us, vs = M.momentum_predictor_lid_imex(*args, **kw)
        print(f"imex {A.pred_id(case)}: rel {A.rel(us, uo):.3g}, {A.rel(vs, vo):.3g}")
        _close(us, uo, bar); _close(vs, vo, bar)
        _walls_zero(us, vs)


@pytest.mark.parametrize("box", list(A.BOXES))
@pytest.mark.parametrize("N", A.ORACLE_N)
def test_semilag_predictor_vs_oracle(M, MO, N, box):
    """The semi-Lagrangian branch at CFL 4 (backtraces leave the box) in every variant, and
    the branch below cfl_switch, which is the IMEX predictor bit for bit."""
    for case in A.semilag_cases():
        if case[:2] != (N, box):
            continue
        args, kw = A.semilag_inputs(case)
        bar = A.pred_bar("semilag", case[:3])
        uo, vo = _oracle(MO.momentum_predictor_lid_semilag, args, kw, bar)
        us, vs = M.momentum_predictor_lid_semilag(*args, **kw)
        print(f"semilag {A.pred_id(case)} CFL {case[3]}: rel {A.rel(us, uo):.3g}, "
              f"{A.rel(vs, vo):.3g}")
        _close(us, uo, bar); _close(vs, vo, bar)
        _walls_zero(us, vs)
        if case[3] < 0.9:
            ui, vi = M.momentum_predictor_lid_imex(*args, **kw)
            _eq(us, ui); _eq(vs, vi)
        else:
            ui, vi = MO.momentum_predictor_lid_imex(*args, **kw)
            assert A.rel(uo, ui) > 1e-3     # the other branch: a different result
