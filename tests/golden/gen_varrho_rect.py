"""Golden-vector generator for the variable-density projection off the square
(functions.py:1016-1070, 1122-1168, 1296-1364): runs the pyRMT reference in pure-Python mode
(imported exactly as gen_golden.py does) on the grids of varrho_np.FIXTURE_GRIDS and writes

    tests/golden/varrho_rect.npz   (20, 47) and (131, 5) with dx = 1/(nx-1), dy = 0.7/(ny-1);
                                   (5, 131) with dy = dx

Per grid (keys g<ny>x<nx>_*): the inputs of varrho_np.case (a density that varies along the
walls), the eigenvalues, the matrix-free operator applied to p (Ap), the per-face Rhie-Chow
divergence (divU), and the reference's pressure_projection_amg under the free-slip box, the
no-slip lid (speed 1) and the identity BC, with its CG capped at 1, 2 and 5 iterations with a
previous pressure and at 2 without one: an, bn, pn (the three BCs stacked, in the order of
varrho_np.BCS) and the callback count.

The reference's cg call goes through the keyword shim of gen_golden.gen_varrho (tol -> rtol,
LinearOperator with dtype=float64), with maxiter replaced by the case's cap: the reference
hard-codes 200, and on these problems its CG never converges, so the capped
iterates are what another implementation can be held to.

The file is 360 KiB: the planes are full-entropy doubles (a rough density, random velocities
and pressures), 2250 cells x 8 bytes x (9 input and operator planes + 4 runs x 3 fields) once
the BC stacks have compressed to little more than one plane each.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz file is data.

Usage:  python -B tests/golden/gen_varrho_rect.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import C, F, OUT, save  # noqa: E402
import numpy as np  # noqa: E402
import scipy.sparse.linalg as sla  # noqa: E402
import varrho_np as V  # noqa: E402

REF_BCS = {"freeslip": C.free_slip_box_bc, "lid": C.no_slip_lid_bc,
           "identity": lambda u, v: (u, v)}
CAP = [None]
COUNTS = []


def cg_compat(A, rhs, x0=None, tol=1e-5, maxiter=None, M=None):
    n = [0]
    x, info = sla.cg(A, rhs, x0=x0, rtol=tol, maxiter=CAP[0], M=M,
                     callback=lambda xk: n.__setitem__(0, n[0] + 1))
    COUNTS.append(n[0])
    return x, info


def gen_grid(shape, kind):
    ny, nx = shape
    c = V.case(shape, kind)
    V.check_density(c["rho"], kind)
    dx, dy, dt, rho = c["dx"], c["dy"], c["dt"], c["rho"]
    out = {k: c[k] for k in V.INPUTS + ("dx", "dy", "dt")}
    out["eig"] = eig = F._precompute_poisson_eigenvalues(nx, ny, dx, dy)
    out["Ap"] = F._apply_variable_poisson(c["p"].ravel(), nx, ny, dx, dy, 1.0 / rho)
    out["divU"] = F._compute_divergence_rc(c["a"], c["b"], c["p_prev"], dt, rho, dx, dy)
    runs = {}
    for maxiter, with_prev in V.RUNS:
        CAP[0] = maxiter
        res, n0 = [], len(COUNTS)
        for bc in V.BCS:
            pp = c["p_prev"].copy() if with_prev else None
            res.append(F.pressure_projection_amg(c["a"].copy(), c["b"].copy(), dx, dy, dt,
                                                 rho.copy(), REF_BCS[bc], p_prev=pp,
                                                 eigenvalues=eig)[:3])
        its = COUNTS[n0:]
        assert len(its) == 3 and len(set(its)) == 1, its   # the BC acts after the solve
        for k, name in enumerate(("an", "bn", "pn")):
            runs[V.run_key(shape, maxiter, with_prev, name)] = np.stack([r[k] for r in res])
        runs[V.run_key(shape, maxiter, with_prev, "it")] = its[0]
        print(f"  {V.sid(shape)} {kind} maxiter {maxiter} p_prev {with_prev}: {its[0]} "
              f"iterations, |pn| {np.abs(res[0][2]).max():.3g}")
    return {**{V.key(shape, k): v for k, v in out.items()}, **runs}


if __name__ == "__main__":
    t0 = time.time()
    cg_ref, lo_ref = F.cg, F.LinearOperator
    F.cg = cg_compat
    F.LinearOperator = lambda shape, matvec: sla.LinearOperator(shape, matvec=matvec,
                                                                dtype=np.float64)
    out = {}
    try:
        for shape, kind in V.FIXTURE_GRIDS:
            out.update(gen_grid(shape, kind))
    finally:
        F.cg, F.LinearOperator = cg_ref, lo_ref
    save("varrho_rect", **out)
    size = os.path.getsize(os.path.join(OUT, "varrho_rect.npz"))
    assert size <= 400 * 1024, size
    print(f"done in {time.time() - t0:.0f}s")
