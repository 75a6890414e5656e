"""The free-slip MAC box without a GPU: the tests' NumPy restatements of the two operators
against the reference's fixtures (bit for bit), argument validation ahead of the GPU check,
and the two drivers' dt formulas."""
import numpy as np
import pytest

from conftest import golden
import mac_freeslip_np as NP


@pytest.mark.parametrize("N", [4, 5, 33, 64])
def test_numpy_restatement_equals_reference(N):
    g = NP.ops_fixture(golden, N)
    dx = dy = 1.0 / N
    us, vs = NP.momentum_predictor_freeslip(g["u"], g["v"], g["nu"], dx, dy, g["dt"], g["fu"],
                                            g["fv"], g["rho"])
    np.testing.assert_array_equal(us, g["us"])
    np.testing.assert_array_equal(vs, g["vs"])
    us0, vs0 = NP.momentum_predictor_freeslip(g["u"], g["v"], g["nu"], dx, dy, g["dt"])
    np.testing.assert_array_equal(us0, g["us0"])
    np.testing.assert_array_equal(vs0, g["vs0"])
    gu, gv = NP.interfacial_force_faces(g["kappa"], g["H"], g["gamma"], dx, dy)
    np.testing.assert_array_equal(gu, g["gu"])
    np.testing.assert_array_equal(gv, g["gv"])
    # the inputs' wall-normal faces are not zero, the outputs' are
    assert np.all(g["u"][:, [0, -1]] != 0) and np.all(g["v"][[0, -1], :] != 0)
    for a in (g["us"][:, [0, -1]], g["vs"][[0, -1], :], g["gu"][:, [0, -1]], g["gv"][[0, -1], :]):
        assert np.all(a == 0)


def test_bad_walls_raises_before_the_gpu_check():
    from pyrmt_amd import mac
    with pytest.raises(ValueError, match="walls"):
        mac.MacMultiDisc(16, specs=[(0.2, 0.5, 0.5)], walls="nope")
    with pytest.raises(ValueError, match="dt"):
        mac.MacMultiDisc(16, specs=[(0.2, 0.5, 0.5)], dt=-1.0)


def test_driver_dt_formulas():
    from pyrmt_amd import mac
    g = golden("mac_freeslip_tg")
    for N, _ in g["cases"]:
        assert mac.disc_in_tg_dt(int(N)) == float(g[f"n{N}_dt"])
    c = golden("mac_freeslip_contact")
    assert mac.two_disc_dt(int(c["N"]), V0=float(c["V0"])) == float(c["dt"])
    # a given dt takes the formula's place (U_lid = 0 would divide by zero in it)
    P, dt = mac.mac_params(32, [(0.15, 0.5, 0.7)], U_lid=0.0, dt=1.25e-3)
    assert dt == 1.25e-3 and P.dt == 1.25e-3 and P.U_lid == 0.0


def test_run_one_refuses_what_the_fused_loop_does_not_run():
    from pyrmt_amd import mac
    for kw in ({"scheme": "weno5"}, {"isochoric": True}, {"normalize_phi": True}):
        with pytest.raises(NotImplementedError, match="momentum_predictor_freeslip"):
            mac.disc_in_tg_run_one(32, 0.1, **kw)
