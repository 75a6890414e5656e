"""The variable-density projection (pyrmt_amd/csrc/varrho.hip: k_vr_apply, k_vr_div_rc,
k_vr_correct on the solver of cg.hpp) off the square and at its launch edges, against the
reference's own results (tests/golden/varrho_rect.npz) and the oracle that
tests/test_varrho_rect_cpu.py holds to them bit for bit.  tests/varrho_np.py builds the cases:
nx != ny on every grid, dx != dy on half of them, a density that varies along the walls (the
disc crosses the west wall and the lid, times a rough factor per cell), the three velocity BCs.

Bars:
  * the matrix-free operator and the per-face Rhie-Chow divergence: bit-exact;
  * the projection: tests/test_gpu_varrho.py's bar, atol = 1e-10 max(|ref|.max(), 1), and the
    iteration count equal.  The solves differ from the oracle's in rounding only (the dot
    products fold in another order, the preconditioner's DCT is the LDS FFT or rocFFT against
    pocketfft); noise of 1e-15 of max-abs in every preconditioner application of the oracle
    moves a, b, p by at most 1.3e-13 max(|ref|, 1) on these shapes;
  * the near-constant density path: the 1e-12 bar of test_projection_near_constant_density.

Every test prints its worst distance over the bar before it asserts.  The largest seen on an
MI355X, as fractions of the bar: 2.0e-4 of the 1e-10 bar ((131, 5) aniso, one iteration, every
BC; 1.5e-4 on the (263, 1001) grid, 1.2e-5 at ptp(rho) = 2e-10), 2.4e-3 of the 1e-12 bar of the
near-constant path; no cell differs in any bit-exact case.
"""
import functools

import numpy as np
import pytest

import varrho_np as V
from conftest import golden

# the shared inputs are read-only arrays; the wrappers copy them to the device at once
pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

_eq = np.testing.assert_array_equal
_id = lambda s, k: "%s-%s" % (V.sid(s), k)
FIX = [pytest.param(s, k, id=_id(s, k)) for s, k in V.FIXTURE_GRIDS]
KINDS = ("aniso", "iso")


def _bc(name):
    from pyrmt_amd.bc import FreeSlipBox, NoSlipLid
    return {"freeslip": FreeSlipBox(), "lid": NoSlipLid(1.0), "identity": lambda u, v: (u, v)}[name]


def _eig(c):
    from oracle import oracle as O
    if "eig" not in c:
        ny, nx = c["a"].shape
        return O._precompute_poisson_eigenvalues(nx, ny, c["dx"], c["dy"])
    return c["eig"]


def _gpu_project(monkeypatch, c, bc, maxiter, with_prev=True, rtol=None):
    """(a, b, p, last_cg_iterations) of one pressure_projection_amg call."""
    from pyrmt_amd import functions as F
    monkeypatch.setattr(F, "CG_MAXITER", maxiter)
    if rtol is not None:
        monkeypatch.setattr(F, "CG_RTOL", rtol)
    monkeypatch.setattr(F, "last_cg_iterations", None)
    a, b, p, _, _ = F.pressure_projection_amg(
        c["a"], c["b"], c["dx"], c["dy"], c["dt"], c["rho"], _bc(bc),
        p_prev=c["p_prev"] if with_prev else None, eigenvalues=_eig(c))
    return a, b, p, F.last_cg_iterations


@functools.lru_cache(maxsize=None)
def _oracle_project(shape, kind, bc, maxiter, with_prev=True, rtol=1e-6):
    """The oracle's (a, b, p, iterations) of a case of varrho_np.case: computed once."""
    from oracle import oracle as O
    c = V.case(shape, kind)
    ref = O.pressure_projection_variable(c["a"], c["b"], c["dx"], c["dy"], c["dt"], c["rho"],
                                         *V.BCS[bc], c["p_prev"] if with_prev else None,
                                         _eig(c), rtol=rtol, maxiter=maxiter)
    for x in ref[:3]:
        x.setflags(write=False)
    return ref


def _held(got, ref, what, bar=V.BAR):
    """Print the worst distance of a, b, p over the bar, then assert each field to it."""
    print("%s: worst |got - ref| / bar = %.3g" % (what, V.worst(got[:3], ref[:3], bar)))
    for g, r in zip(got[:3], ref[:3]):
        np.testing.assert_allclose(g, r, rtol=0, atol=bar * max(np.abs(r).max(), 1.0),
                                   err_msg=what)


def _walls_equal(got, ref):
    """Under the lid BC the wall rows and columns of a and b are constants: exactly equal."""
    for g, r in zip(got[:2], ref[:2]):
        for sl in (np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1]):
            _eq(g[sl], r[sl])
    assert (ref[0][-1, 1:-1] == 1.0).all() and ref[0][-1, 0] == 0.0 == ref[0][-1, -1]


# ── operator and divergence: bit-exact ────────────────────────────────────────────
def _operator_and_divergence(c):
    from pyrmt_amd import functions as F
    ny, nx = c["a"].shape
    Ap = F._apply_variable_poisson(c["p"].ravel(), nx, ny, c["dx"], c["dy"], 1.0 / c["rho"])
    div = F._compute_divergence_rc(c["a"], c["b"], c["p_prev"], c["dt"], c["rho"], c["dx"],
                                   c["dy"])
    return Ap, div


@pytest.mark.parametrize("shape, kind", FIX)
def test_operator_and_divergence_fixture(gpu, shape, kind):
    """Against the reference's own Ap and divU."""
    c = V.fixture_case(golden("varrho_rect"), shape)
    Ap, div = _operator_and_divergence(c)
    print("%s: Ap differs in %d cells, divU in %d (bit-exact bar)"
          % (_id(shape, kind), (Ap != c["Ap"].ravel()).sum(), (div != c["divU"]).sum()))
    _eq(Ap, c["Ap"].ravel())
    _eq(div, c["divU"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", V.OP_SHAPES, ids=V.sid)
def test_operator_and_divergence_oracle(gpu, oracle, shape, kind):
    c = V.case(shape, kind)
    V.check_density(c["rho"], kind)
    ny, nx = shape
    Ap, div = _operator_and_divergence(c)
    rAp = oracle._apply_variable_poisson(c["p"].ravel(), nx, ny, c["dx"], c["dy"],
                                         1.0 / c["rho"])
    rdiv = oracle._compute_divergence_rc(c["a"], c["b"], c["p_prev"], c["dt"], c["rho"],
                                         c["dx"], c["dy"])
    print("%s: Ap differs in %d cells, divU in %d (bit-exact bar)"
          % (_id(shape, kind), (Ap != rAp).sum(), (div != rdiv).sum()))
    _eq(Ap, rAp)
    _eq(div, rdiv)


# ── the projection against the reference's own runs ───────────────────────────────
@pytest.mark.parametrize("bc", list(V.BCS))
@pytest.mark.parametrize("shape, kind", FIX)
def test_projection_fixture(gpu, monkeypatch, shape, kind, bc):
    """Every cap (1, 2, 5 with a previous pressure, 2 without) of one grid and BC."""
    G = golden("varrho_rect")
    c = V.fixture_case(G, shape)
    k = list(V.BCS).index(bc)
    for maxiter, with_prev in V.RUNS:
        ref = [G[V.run_key(shape, maxiter, with_prev, n)][k] for n in ("an", "bn", "pn")]
        got = _gpu_project(monkeypatch, c, bc, maxiter, with_prev)
        assert got[3] == int(G[V.run_key(shape, maxiter, with_prev, "it")]) == maxiter
        _held(got, ref, "%s %s maxiter %d p_prev %s" % (_id(shape, kind), bc, maxiter, with_prev))
        if bc == "lid":
            _walls_equal(got, ref)


# ── the projection against the oracle ─────────────────────────────────────────────
@pytest.mark.parametrize("bc", list(V.BCS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", V.PROJ_SHAPES, ids=V.sid)
def test_projection_oracle(gpu, monkeypatch, shape, kind, bc):
    c = V.case(shape, kind)
    for maxiter in V.MAXITERS:
        ref = _oracle_project(shape, kind, bc, maxiter)
        got = _gpu_project(monkeypatch, c, bc, maxiter)
        assert got[3] == ref[3] == maxiter
        _held(got, ref, "%s %s maxiter %d" % (_id(shape, kind), bc, maxiter))
        if bc == "lid":
            _walls_equal(got, ref)


# ── the stopping test ends the solve below the cap ────────────────────────────────
@pytest.mark.parametrize("with_prev", [True, False])
@pytest.mark.parametrize("shape, kind", [pytest.param((37, 133), "aniso", id="37x133-aniso"),
                                         pytest.param((133, 37), "iso", id="133x37-iso")])
def test_projection_convergence_exit(gpu, monkeypatch, shape, kind, with_prev):
    """rtol is the geometric mean of the oracle's relative residuals at its tests of iterations
    3 and 4, so the solve ends at 4 of 200.  Those residuals are
        (37, 133) aniso   0.0314 / 0.0103  with p_prev,   0.0331 / 0.0107  without
        (133, 37) iso     0.0376 / 0.00901 with p_prev,   0.0379 / 0.00906 without
    a factor 1.74 .. 2.04 either side of rtol (>= 1.5 is asserted), so the summation order
    cannot move the count.  (The residual falls about 3 x per iteration up to the seventh and
    stalls near 1e-4; on the 5-wide grids it stalls at 1e-3 .. 4e-3: not used here.)"""
    from oracle import oracle as O
    from pyrmt_amd import functions as F
    c = V.case(shape, kind)
    res = V.oracle_residuals(O, c, with_prev, 5)
    rtol = float(np.sqrt(res[3] * res[4]))
    print("%s p_prev %s: residuals %.4g / %.4g, rtol %.4g" % (_id(shape, kind), with_prev,
                                                              res[3], res[4], rtol))
    assert min(res[:4]) / rtol >= 1.5 and rtol / res[4] >= 1.5
    ref = _oracle_project(shape, kind, "freeslip", F.CG_MAXITER, with_prev, rtol)
    got = _gpu_project(monkeypatch, c, "freeslip", F.CG_MAXITER, with_prev, rtol=rtol)
    assert got[3] == ref[3] == 4 < F.CG_MAXITER
    _held(got, ref, "%s p_prev %s exit at %d" % (_id(shape, kind), with_prev, ref[3]))


# ── the second grid-stride trip of k_vr_apply ─────────────────────────────────────
def test_grid_stride_second_trip(gpu, oracle, monkeypatch):
    """(263, 1001) has 263263 cells and k_vr_apply strides over 1024 * 256 = 262144 threads:
    the second trip holds the last row (mirror ghost in y) and 118 interior cells of the row
    below it, in the standalone operator (grid = min(CG_BLOCKS, ...)) and in the CG's, whose
    p.q partials those cells feed.  The operator is bit-exact over the whole plane; one lid
    projection at two iterations holds the bar.  262 = 2 * 131 has a prime factor above 31, so
    this grid has no LDS DCT plan: the preconditioner runs on rocFFT (every other grid this file
    projects on factors into radices <= 23 on both axes and takes the LDS path)."""
    from pyrmt_amd import functions as F
    shape, kind = V.STRIDE_SHAPE, "aniso"
    ny, nx = shape
    assert V.CG_THREADS + nx < ny * nx < 2 * V.CG_THREADS
    c = V.case(shape, kind)
    V.check_density(c["rho"], kind)
    Ap = F._apply_variable_poisson(c["p"].ravel(), nx, ny, c["dx"], c["dy"], 1.0 / c["rho"])
    rAp = oracle._apply_variable_poisson(c["p"].ravel(), nx, ny, c["dx"], c["dy"],
                                         1.0 / c["rho"])
    print("Ap differs in %d cells of the first trip, %d of the second (bit-exact bar)"
          % ((Ap != rAp)[:V.CG_THREADS].sum(), (Ap != rAp)[V.CG_THREADS:].sum()))
    _eq(Ap, rAp)
    ref = _oracle_project(shape, kind, "lid", 2)
    got = _gpu_project(monkeypatch, c, "lid", 2)
    assert got[3] == ref[3] == 2
    _held(got, ref, "263x1001 lid maxiter 2")
    _walls_equal(got, ref)


# ── the dispatch on np.ptp(rho) next to its 1e-10 threshold ───────────────────────
def _threshold_case(amp):
    shape, kind = (37, 133), "aniso"
    ny, nx = shape
    g = np.where(np.add.outer(np.arange(ny), np.arange(nx)) % 2 == 0, 1.0, -1.0)
    return dict(V.case(shape, kind), rho=1.0 + amp * g)


def test_dispatch_above_threshold(gpu, oracle, monkeypatch):
    """ptp(rho) = 2e-10 > 1e-10: the variable path (last_cg_iterations is set afresh).  With
    the reference's rtol = 1e-6 the oracle's CG does not stop on this case (its residual is
    2.7e-5 after one iteration and grows from the third on), so no count below the cap can be
    asked for: the fields are compared at maxiter = 1."""
    c = _threshold_case(1e-10)
    assert np.ptp(c["rho"]) > 1e-10
    ref = oracle.pressure_projection_variable(c["a"], c["b"], c["dx"], c["dy"], c["dt"],
                                              c["rho"], 2, 0.0, c["p_prev"], _eig(c), maxiter=1)
    got = _gpu_project(monkeypatch, c, "freeslip", 1)
    assert got[3] == ref[3] == 1
    _held(got, ref, "ptp 2e-10, variable path")


def test_dispatch_below_threshold(gpu, oracle, monkeypatch):
    """0 < ptp(rho) = 5e-11 <= 1e-10: the constant-density branch with the array pointwise
    (rmt_pressure_projection_rho_field); no CG runs, last_cg_iterations stays untouched."""
    c = _threshold_case(2.5e-11)
    assert 0 < np.ptp(c["rho"]) <= 1e-10
    ref = oracle.pressure_projection(c["a"], c["b"], c["dx"], c["dy"], c["dt"], c["rho"], 2,
                                     0.0, c["p_prev"], _eig(c))
    got = _gpu_project(monkeypatch, c, "freeslip", 1)
    assert got[3] is None
    _held(got, ref, "ptp 5e-11, rho_field path", bar=1e-12)


# ── device tensors in, device tensors out ─────────────────────────────────────────
def test_device_tensors(gpu, monkeypatch):
    import torch
    from pyrmt_amd import functions as F
    shape, kind = (37, 133), "aniso"
    c = V.case(shape, kind)
    host = _gpu_project(monkeypatch, c, "freeslip", 2)
    t = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("a", "b", "rho", "p_prev")}
    a, b, p, _, _ = F.pressure_projection_amg(t["a"], t["b"], c["dx"], c["dy"], c["dt"],
                                              t["rho"], _bc("freeslip"), p_prev=t["p_prev"],
                                              eigenvalues=_eig(c))
    assert F.last_cg_iterations == host[3] == 2
    for dev, ref in zip((a, b, p), host[:3]):
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64
        print("device vs host call: %d cells differ (bit-exact bar)"
              % (dev.cpu().numpy() != ref).sum())
        _eq(dev.cpu().numpy(), ref)


# ── a periodic velocity BC has no place on the variable Neumann path ──────────────
def test_periodic_bc_refused(gpu, monkeypatch):
    from pyrmt_amd import functions as F
    from pyrmt_amd.bc import Periodic
    c = V.case((20, 47), "aniso")
    monkeypatch.setattr(F, "last_cg_iterations", None)
    with pytest.raises(ValueError, match="unknown velocity bc kind"):
        F.pressure_projection_amg(c["a"], c["b"], c["dx"], c["dy"], c["dt"], c["rho"],
                                  Periodic(), p_prev=c["p_prev"], eigenvalues=_eig(c))
    assert F.last_cg_iterations is None
    # the context is usable afterwards
    got = _gpu_project(monkeypatch, c, "freeslip", 1)
    _held(got, _oracle_project((20, 47), "aniso", "freeslip", 1), "after the refusal")
