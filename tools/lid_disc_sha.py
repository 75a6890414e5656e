"""SHA-256 of everything the two lid-cavity disc loops and their fused operators compute, one
"case digest" line each: the same-bits check of a change that must not move an output bit.
   python tools/lid_disc_sha.py [ROOT]
ROOT: the tree whose pyrmt_amd (with its librmt.so) and tests/ inputs are used (default: this
one), so that a checkout of another commit is hashed by the same script, each in its own process.
  total_force, total_stress (with Ftot), epoch_distortion   the reinit operator shapes + s40
  solid_force (four variants), soft_diag                    the soft-disc operator shapes
  MacReinitDisc(32, reinit_J=1.02), 60 steps; MacSoftDisc(32), 30 steps on each of the six
  rungs: state(), the record and the counters
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                       os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from pyrmt_amd import mac as M  # noqa: E402
import mac_reinit_np as RN  # noqa: E402
import mac_soft_disc_np as SN  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def show(case, *arrays, note=""):
    print(f"{case:<44} {digest(*arrays)}{note}", flush=True)


def show_sim(case, sim, *more):
    s = sim.state()
    show(case, *[s[k] for k in sim.STATE], np.array(sim.record), [sim.nsteps, sim.diverged, *more],
         note=f"  steps {sim.nsteps}" + (" diverged" if sim.diverged else ""))


ops = np.load(os.path.join(ROOT, "tests", "golden", "mac_reinit_ops.npz"))
cases = [(RN.key(s), RN.op_inputs(s)) for s in RN.SHAPES]
dx40 = float(ops["s40_dx"])
cases.append(("s40", dict(X1=ops["s40_X1"], X2=ops["s40_X2"], Fs=list(ops["s40_Fs"]),
                          phi=ops["s40_phi"], dx=dx40, dy=dx40, w_t=2.0 * dx40)))
for name, g in cases:
    mu_s = 0.3 if name == "s40" else RN.MU_S
    args = (g["X1"], g["X2"], g["Fs"], g["phi"], g["dx"], g["dy"], g["w_t"], mu_s)
    fu, fv, J = M.total_force(*args)
    show(f"total_force {name}", fu, fv, J)
    Sxx, Sxy, Syy, J, Ft = M.total_stress(*args, with_Ftot=True)
    show(f"total_stress {name}", Sxx, Sxy, Syy, J, *Ft)
    show(f"epoch_distortion {name}", M.epoch_distortion(J, g["phi"]))

for shape in SN.SHAPES:
    g = SN.op_inputs(shape)
    for iso, clamp in SN.FORCE_VARIANTS:
        fu, fv, J = M.solid_force(g["X1"], g["X2"], g["phi"], g["dx"], g["dy"], g["w_t"], SN.MU_S,
                                  SN.KAPPA, clamp, iso)
        show(f"solid_force {SN.key(shape)} {SN.vkey(iso, clamp)}", fu, fv, J)
    show(f"soft_diag {SN.key(shape)}", M.soft_diag(g["phi"], J, g["u0"], g["v0"], g["dx"], g["dy"]))

sim = M.MacReinitDisc(32, reinit_J=1.02).step(60)     # reinitialises at steps 26 and 53
show_sim("MacReinitDisc(32, reinit_J=1.02) 60 steps", sim, sim.n_reinit, *sim.reinit_steps)
for rung in ("explicit", "imex", "imex-elastic", "explicit-sl", "imex-sl", "imex-elastic-sl"):
    sim = M.MacSoftDisc(32, integrator=rung).step(30)
    show_sim(f"MacSoftDisc(32) {rung} 30 steps", sim, sim.sl_steps, *sim.pcg_iters)
