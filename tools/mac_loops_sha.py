"""SHA-256 of what the MAC lid loop with three discs and the periodic MAC loop leave, one "case
digest" line each (tools/lid_disc_sha.py covers the two lid-cavity disc loops): the same-bits
check of a change to the host side of the library or the binding.
   python tools/mac_loops_sha.py [ROOT]
ROOT: the tree whose pyrmt_amd (with its librmt.so) is used (default: this one), so that a
checkout of another commit is hashed by the same script, each in its own process.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                       os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from pyrmt_amd import mac as M  # noqa: E402


def show(case, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    print(f"{case:<44} {h.hexdigest()}", flush=True)


sim = M.MacMultiDisc(128)
sim.step(40)
d = sim.diagnostics()
show("MacMultiDisc(128) 40 steps", *[sim.get(f) for f in ("u", "v", "p")],
     *[sim.get(f, k) for k in range(len(sim.specs)) for f in ("X1", "X2", "phi")],
     *[d[k] for k in sorted(d)])

N = 96
for integrator, semilag in (("explicit", False), ("imex", False), ("imex", True)):
    # dt = 0.2 dx: explicit-stable; dt = 1.2 dx: past cfl_switch, the semi-Lagrangian branch
    dt = (1.2 if semilag else 0.2) * 2 * np.pi / N
    sim = M.MacTaylorGreen(N, 0.05, dt, integrator, semilag=semilag)
    sim.step(30)
    show(f"MacTaylorGreen({N}) {integrator}{'-sl' if semilag else ''} 30 steps",
         sim.get("u"), sim.get("v"), sim.get("p"), [sim.nsteps, sim.sl_steps])
