"""Host side of the periodic MAC tier (pyrmt_amd.mac, mac.py:461-467, 501-509 and the
integrator names of benchmarks/mac_taylor_green_convergence.py:47-52): the eigenvalue tables
against the reference's (tests/golden/mac_periodic*.npz, gen_mac_periodic.py), the
separability check of the tables handed to the FFT solves, and the name handling.  No GPU."""
import numpy as np
import pytest

from conftest import golden

SHAPES = ((5, 7), (20, 36), (64, 64), (33, 130))


def _fixture(ny, nx):
    if ny * nx > 1000:
        return dict(golden(f"mac_periodic_{ny}x{nx}"))
    g = golden("mac_periodic")
    k = f"s{ny}x{nx}_"
    return {n[len(k):]: g[n] for n in g.files if n.startswith(k)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_fixture_shapes():
    np.testing.assert_array_equal(golden("mac_periodic")["shapes"], SHAPES)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_eigenvalue_tables_bitwise(ny, nx):
    from pyrmt_amd import mac
    g = _fixture(ny, nx)
    dx, dy = float(g["dx"]), float(g["dy"])
    eig = mac.poisson_eigs_periodic(nx, ny, dx, dy)
    lap = mac.lap_eigs_periodic(nx, ny, dx, dy)
    assert eig.shape == lap.shape == (ny, nx)
    np.testing.assert_array_equal(_bits(eig), _bits(g["eig"]))
    np.testing.assert_array_equal(_bits(lap), _bits(g["lap"]))      # (0,0) is -0.0
    assert eig[0, 0] == 1.0 and np.signbit(lap[0, 0])


@pytest.mark.parametrize("ny,nx", SHAPES[:2])
def test_axis_vectors_rebuild_the_reference_tables(ny, nx):
    from pyrmt_amd import mac
    g = _fixture(ny, nx)
    for name, pinned in (("eig", True), ("lap", False)):
        lx, ly = mac._axis_eigs_per(g[name], pinned)
        tab = lx[None, :] + ly[:, None]
        if pinned:
            tab[0, 0] = 1.0
        np.testing.assert_array_equal(_bits(tab), _bits(g[name]))


def test_separability_check_rejects_a_perturbed_table():
    from pyrmt_amd import mac
    g = _fixture(20, 36)
    for name, pinned in (("eig", True), ("lap", False)):
        bad = g[name].copy()
        bad[7, 11] = np.nextafter(bad[7, 11], 0.0)          # one ulp, one entry
        with pytest.raises(NotImplementedError):
            mac._axis_eigs_per(bad, pinned)
        mac._axis_eigs_per(g[name], pinned)
    # the Poisson pin is ignored (the solve zeroes that mode), the Laplacian's (0,0) is not
    eig = g["eig"].copy(); eig[0, 0] = 3.0
    mac._axis_eigs_per(eig, True)
    lap = g["lap"].copy(); lap[0, 0] = 1.0
    with pytest.raises(NotImplementedError):
        mac._axis_eigs_per(lap, False)
    # separable, but not even in the wavenumber: no half-spectrum solve
    skew = np.arange(36.0)[None, :] + np.zeros(20)[:, None]
    with pytest.raises(NotImplementedError):
        mac._axis_eigs_per(skew, False)
    # the public solves check before they touch the device
    with pytest.raises(NotImplementedError):
        mac.solve_poisson_periodic(g["p"], bad)
    with pytest.raises(NotImplementedError):
        mac.solve_helmholtz_periodic(g["p"], lap, 0.7)


def test_integrator_names():
    from pyrmt_amd import mac
    R = mac._resolve_periodic_integrator
    assert R(None) == "explicit" and R(None, implicit_visc=True) == "imex"
    for name in ("explicit", "exp", "forward-euler", "Forward_Euler", " EXPLICIT "):
        assert R(name) == "explicit"
    for name in ("imex", "imex-visc", "implicit-viscosity", "semi-implicit", "IMEX_visc"):
        assert R(name) == "imex"
    assert R("explicit", implicit_visc=True) == "explicit"      # the name wins over the boolean
    for name in ("imex-sl", "IMEX_SL"):
        with pytest.raises(NotImplementedError):
            R(name)
    for name in ("imex-elastic", "elastic", "implicit-elastic", "rk4", ""):
        with pytest.raises(ValueError):
            R(name)
    # run_one resolves the name before it needs the device
    with pytest.raises(NotImplementedError):
        mac.taylor_green_run_one(32, integrator="imex-sl")
    with pytest.raises(ValueError):
        mac.taylor_green_run_one(32, integrator="leapfrog")
