"""Reference-map reinitialisation (benchmarks/mac_reinit_test.py), the parts that need no GPU:
the committed fixtures are self-consistent and the public names exist."""
import numpy as np

from conftest import golden
import mac_reinit_np as NP


def test_trace_fixture_is_self_consistent():
    g = golden("mac_reinit_trace32")
    rec = g["record"]
    assert rec.shape == (61, 7)
    # the reinitialisation steps, as the n_reinit column and as stored
    jumps = 1 + np.flatnonzero(np.diff(np.concatenate([[0.0], rec[:, 4]])))
    assert jumps.tolist() == g["reinit_steps"].tolist() == [26, 53]
    # no decision within 1e-6 of the threshold: device rounding (~1e-14) cannot flip one
    margin = np.abs(rec[:, 1] - float(g["reinit_J"])).min()
    assert margin == float(g["margin"]) >= 1e-6
    over = rec[:, 1] > float(g["reinit_J"])
    assert (1 + np.flatnonzero(over)).tolist() == [26, 53]
    # dist is :94's max(max J, 1 / max(min J, 1e-6))
    np.testing.assert_array_equal(rec[:, 1], np.maximum(rec[:, 3], 1.0 / np.maximum(rec[:, 2], 1e-6)))
    # the last step is clipped to t_end
    dts = np.diff(np.concatenate([[0.0], rec[:, 0]]))
    np.testing.assert_allclose(dts[:60], float(g["dt"]), rtol=1e-12)
    assert dts[60] < 0.75 * float(g["dt"]) and abs(rec[60, 0] - float(g["t_end"])) < 1e-15


def test_reinitialisation_stores_ftot_and_resets_the_map():
    g = golden("mac_reinit_trace32")
    N = int(g["N"])
    dx = 1.0 / N
    xc = (np.arange(N) + 0.5) * dx
    Xc, Yc = np.meshgrid(xc, xc)
    for k in (26, 53):
        sm = g[f"after{k}_phi"] <= 0
        assert sm.any()
        # Fs after the step is the extrapolated Ftot: equal on the solid
        for c in range(4):
            np.testing.assert_array_equal(g[f"after{k}_Fs"][c][sm], g[f"ftot{k}"][c][sm])
        np.testing.assert_array_equal(g[f"after{k}_phiref"], g[f"after{k}_phi"])
        np.testing.assert_array_equal(g[f"after{k}_X1"], Xc)
        np.testing.assert_array_equal(g[f"after{k}_X2"], Yc)
    # step 40 lies in the second epoch: no reinitialisation, phiref kept, Fs away from I
    assert "ftot40" not in g.files
    np.testing.assert_array_equal(g["after40_phiref"], g["before40_phiref"])
    assert np.abs(g["before40_Fs"][0] - 1.0).max() > 1e-3
    np.testing.assert_array_equal(g["before40_phiref"], g["after26_phiref"])


def test_ops_fixture_covers_the_edge_cases():
    o = golden("mac_reinit_ops")
    for shape in NP.SHAPES:
        k = NP.key(shape)
        g = NP.op_inputs(shape)
        assert g["dx"] != g["dy"]
        assert o[f"{k}_J"].shape == shape and o[f"{k}_fu"].shape == (shape[0], shape[1] + 1)
        assert (o[f"{k}_J"] == 1.0 / 1e-9).any()                  # the detG clamp fires
        assert o[f"{k}_dist"][2] == (g["phi"] <= 0).sum() > 0
        assert np.isnan(o[f"{k}_advm"]).any() and np.signbit(o[f"{k}_advm"]).any()
        assert (o[f"{k}_fu"][:, [0, -1]] == 0).all() and (o[f"{k}_fv"][[0, -1], :] == 0).all()
    assert np.abs(o["s40_Fs"][0] - 1.0).max() > 1e-3


def test_names_exported():
    from pyrmt_amd import mac, functions, _lib
    import pyrmt_amd
    for name in ("MacReinitDisc", "mac_reinit_run", "total_stress", "total_force",
                 "epoch_distortion"):
        assert hasattr(mac, name), name
    assert hasattr(functions, "advect_reference_maps")
    assert hasattr(pyrmt_amd, "advect_reference_maps")
    for name in ("rmt_advect_sl_rk4_multi", "rmt_mac_total_stress", "rmt_mac_total_force",
                 "rmt_mac_epoch_distortion"):
        assert name in _lib.SIGNATURES, name
