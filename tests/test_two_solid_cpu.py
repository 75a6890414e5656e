"""CPU-side checks of the two-solid / surface-tension surface: the operators are exported,
their C entry points are declared, exported and bound, and the fixture file holds what the
GPU tests rely on (a contact force that is not zero, a density that is constant only to
rounding, cells inside both solids' blend regions)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT, golden

OPERATORS = ("momentum_step_rk4_2solids", "compute_curvature", "compute_contact_force")
ENTRY_POINTS = ("rmt_compute_curvature", "rmt_compute_contact_force", "rmt_momentum_step_rk4_st",
                "rmt_momentum_step_rk4_2solids", "rmt_pressure_projection_rho_field",
                "rmt_mask_solid", "rmt_mixture_density", "rmt_two_solid_diag")


def test_operators_exported():
    import pyrmt_amd
    from pyrmt_amd import functions as F
    for name in OPERATORS:
        assert callable(getattr(F, name)), name
        assert name in F.__all__, name
        assert getattr(pyrmt_amd, name) is getattr(F, name)
    assert hasattr(pyrmt_amd.simulation, "TwoDiscContact")


def test_entry_points_declared_exported_bound():
    from pyrmt_amd import _lib
    src = open(os.path.join(ROOT, "include", "rmt.h")).read()
    declared = set(re.findall(r"^\s*int\s*(rmt_\w+)\(", src, re.M))
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(h, name), name
        assert name in _lib.SIGNATURES, name


def test_fixture_conditions():
    g = golden("two_solid")
    shapes = [tuple(int(x) for x in s) for s in g["shapes"]]
    assert shapes == [(48, 48), (64, 128), (35, 130)]
    for ny, nx in shapes:
        k = f"s{ny}x{nx}_"
        assert g[k + "kap"].shape == (ny, nx)
        assert float(g[k + "fc_max"]) > 0 and np.abs(g[k + "fx"]).max() == float(g[k + "fc_max"])
        assert int(g[k + "both"]) > 0
        assert g[k + "k0_u_idx"].size > 0        # the contact force moves the velocity
    rho = g["s48x48_rho"]
    assert 0 < float(g["s48x48_rho_ptp"]) <= 1e-10
    assert np.ptp(rho) == float(g["s48x48_rho_ptp"]) and not np.all(rho == rho.flat[0])
    assert float(g["st_move"]) > 1e-3               # gamma = 0.1 is visible in u
    rec = g["drv_rec"]
    assert rec.shape == (6, 6) and np.all(np.isfinite(rec)) and np.all(np.diff(rec[:, 0]) > 0)
