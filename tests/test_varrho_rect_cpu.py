"""The oracle's variable-density projection off the square (no GPU): oracle/oracle.py's NumPy
restatements (_apply_variable_poisson, _compute_divergence_rc_variable, cg,
pressure_projection_variable) against the reference's own results on rectangular grids with
dx != dy and dx == dy (tests/golden/varrho_rect.npz, made by tests/golden/gen_varrho_rect.py),
bit for bit, as tests/test_oracle_golden.py holds them on one square.  That lets
tests/test_gpu_varrho_offsquare.py use the oracle at sizes the fixture does not hold.

Every case is bit-equal: operator, divergence, and a, b, p and the iteration count under the
free-slip box, the no-slip lid and the identity BC at 1, 2 and 5 iterations with a previous
pressure and at 2 without one.
"""
import numpy as np
import pytest

import varrho_np as V
from conftest import golden

_eq = np.testing.assert_array_equal
GRIDS = [pytest.param(s, k, id="%s-%s" % (V.sid(s), k)) for s, k in V.FIXTURE_GRIDS]


@pytest.mark.parametrize("shape, kind", GRIDS)
def test_fixture_inputs(shape, kind):
    """The fixture holds the grid and the density the cases rest on, and the builder that the
    GPU tests use at other shapes makes the same inputs (to rounding: np.sin may differ by an
    ulp between NumPy builds, everything else is exact)."""
    g = V.fixture_case(golden("varrho_rect"), shape)
    assert g["a"].shape == shape and (g["dx"], g["dy"]) == V.spacing(shape, kind)
    assert (g["dx"] != g["dy"]) == (kind == "aniso")
    V.check_density(g["rho"], kind)
    c = V.case(shape, kind)
    for k in V.INPUTS:
        np.testing.assert_allclose(c[k], g[k], rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("shape, kind", GRIDS)
def test_operator_and_divergence_bitwise(oracle, shape, kind):
    g = V.fixture_case(golden("varrho_rect"), shape)
    ny, nx = shape
    _eq(oracle._precompute_poisson_eigenvalues(nx, ny, g["dx"], g["dy"]), g["eig"])
    _eq(oracle._apply_variable_poisson(g["p"].ravel(), nx, ny, g["dx"], g["dy"],
                                       1.0 / g["rho"]), g["Ap"].ravel())
    _eq(oracle._compute_divergence_rc(g["a"], g["b"], g["p_prev"], g["dt"], g["rho"], g["dx"],
                                      g["dy"]), g["divU"])


@pytest.mark.parametrize("bc", list(V.BCS))
@pytest.mark.parametrize("shape, kind", GRIDS)
def test_projection_bitwise(oracle, shape, kind, bc):
    G = golden("varrho_rect")
    g = V.fixture_case(G, shape)
    k = list(V.BCS).index(bc)
    for maxiter, with_prev in V.RUNS:
        an, bn, pn, it = oracle.pressure_projection_variable(
            g["a"], g["b"], g["dx"], g["dy"], g["dt"], g["rho"], *V.BCS[bc],
            g["p_prev"] if with_prev else None, g["eig"], maxiter=maxiter)
        assert it == int(G[V.run_key(shape, maxiter, with_prev, "it")]) == maxiter
        for got, name in ((an, "an"), (bn, "bn"), (pn, "pn")):
            _eq(got, G[V.run_key(shape, maxiter, with_prev, name)][k])


def test_lid_bc_is_constant_on_the_walls():
    """The no-slip lid's rows are constants in the reference's result (the GPU test asserts
    them exactly): u = 1 on the lid row between the corners, 0 on the other walls, v = 0."""
    G = golden("varrho_rect")
    k = list(V.BCS).index("lid")
    for shape, _ in V.FIXTURE_GRIDS:
        an = G[V.run_key(shape, 2, True, "an")][k]
        bn = G[V.run_key(shape, 2, True, "bn")][k]
        assert (an[-1, 1:-1] == 1.0).all() and (an[0] == 0).all()
        assert (an[:, 0] == 0).all() and (an[:, -1] == 0).all()
        assert (bn[0] == 0).all() and (bn[-1] == 0).all()
        assert (bn[:, 0] == 0).all() and (bn[:, -1] == 0).all()
