"""Times of the two conjugate-gradient paths (csrc/cg.hpp), one JSON line each on stdout,
appended to the file named by RMT_BENCH_OUT when set (profiles/reductions/bench_cg.jsonl is
such a file).  For an A/B of two builds run it once per library (RMT_LIB), alternating.
  helmholtz   N=1024: rmt_mac_helmholtz, DST-preconditioned, u and v faces
  varrho      N=1025: the variable-density projection at CG_MAXITER = 20
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrmt_amd import _lib as L, functions as F, mac as M  # noqa: E402
from pyrmt_amd.bc import FreeSlipBox  # noqa: E402
import _bench  # noqa: E402


def emit(**kw):
    _bench.emit(**kw, lib=os.path.basename(L.LIB_PATH))


def timed(fn, reps):
    """Median and spread of the device-event ms of fn over reps, after 2 warm-ups (the solves
    read r.r back every iteration, so this is the wall time of the call as well)."""
    return _bench.timed(fn, reps, warm=2, stat=lambda ms: (_bench.median(ms), float(min(ms)),
                                                           float(max(ms))))


def bench_helmholtz(N=1024, reps=9):
    dx = 1.0 / N
    coef = 2.0e-3 * 0.01 * (N / 64) ** 2     # the viscous number of the tier's tests, kept at N
    for kind in (0, 1):
        shape = (N, N - 1) if kind == 0 else (N - 1, N)
        rhs = torch.from_numpy(np.random.default_rng(4 + kind).standard_normal(shape)).cuda()
        its = []
        med, lo, hi = timed(lambda: its.append(
            M._solve_helmholtz(rhs, kind, coef, dx, dx, 1e-8, 500, 1)[1]), reps)
        emit(what="helmholtz", N=N, kind=kind, reps=reps, iterations=its[-1], ms=med, ms_min=lo,
             ms_max=hi)


def bench_varrho(N=1025, reps=9, maxiter=20):
    X, Y = np.meshgrid(np.linspace(0, 1, N), np.linspace(0, 1, N))
    dx = 1.0 / (N - 1)
    rng = np.random.default_rng(21)
    rho = 1.0 + 3.0 / (1.0 + np.exp((np.hypot(X - 0.5, Y - 0.45) - 0.25) / (2 * dx)))
    k = 2 * np.pi
    a, b, rho = (torch.from_numpy(x).cuda() for x in (
        0.5 * np.sin(k * X) * np.cos(k * Y) + 0.1 * rng.standard_normal((N, N)),
        -0.5 * np.cos(k * X) * np.sin(k * Y) + 0.1 * rng.standard_normal((N, N)), rho))
    F.CG_MAXITER = maxiter
    kind, lid = F.resolve_bc(FreeSlipBox())
    # (pressure_projection_amg's variable-density branch, past its host-side checks)
    med, lo, hi = timed(lambda: F._projection_variable(a, b, dx, dx, 1e-3, rho, kind, lid, None,
                                                       None, None), reps)
    emit(what="varrho", N=N, reps=reps, iterations=F.last_cg_iterations, ms=med, ms_min=lo,
         ms_max=hi)


if __name__ == "__main__":
    what = sys.argv[1:] or ["helmholtz", "varrho"]
    if "helmholtz" in what:
        bench_helmholtz()
    if "varrho" in what:
        bench_varrho()
