"""The noise floor of the four-roll-mill viscoelastic driver: how far the NumPy restatement
(tests/mac_ve_extension_np.py) moves against itself when every exp, log, sin, cos and arctan2
result is moved by -1, 0 or +1 ulp at random and every FFT solve's output by up to 1e-12 of its
max-abs -- the project's bar for the rocFFT / pocketfft pair (tests/test_gpu_mac_periodic.py).
Each case of the GPU tests is run REPEATS times and the worst absolute difference per quantity
kept; the tests hold the device to BAR_FACTOR times that (mac_ve_extension_np.bar).  sqrt and
the arithmetic are correctly rounded on every side and stay as they are.

Usage:  python tools/mac_ve_ext_floor.py    (CPU only; writes profiles/ve_extension/floor.json)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import mac_ve_extension_np as E  # noqa: E402
from ve_floor import Nudged, worst  # noqa: E402

REPEATS, SEED = 20, 20241


def noisy_solve(rng):
    def solve(rhs, denom, pin=False):
        x = E.fft_solve(rhs, denom, pin)
        return x + (E.FFT_REL * np.abs(x).max()) * rng.uniform(-1.0, 1.0, size=x.shape)
    return solve


def op_cases(X):
    """name -> planes: the operator cases behind sin and exp, the worst over the shapes that
    the fixture holds them for."""
    out = {}
    for shape in E.SHAPES:
        r = E.op_results(X, E.op_inputs(shape))
        for k in ("force", "lock_imex", "lock_imex-elastic"):
            out.setdefault(k, []).extend(np.ravel(p) for p in r[k])
    return out


def run_cases(O, X):
    out = {}
    runs = [(E.short_key(*c), E.short_kwargs(*c)) for c in E.short_cases()]
    runs.append((E.LARGE["key"], E.large_kwargs()))
    for k, kw in runs:
        kw = dict(kw)
        _, _, sim = E.run(O, X, kw.pop("N"), kw.pop("t_end"), **kw)
        rec = np.array(sim.record)
        out[k + "_lam"], out[k + "_bxx"], out[k + "_umax"] = [rec[:, 1]], [rec[:, 2]], [rec[:, 3]]
        for name, val in sim.state().items():
            out[f"{k}_{name}"] = [val]
    return out


def main():
    from oracle import oracle as O
    rng = np.random.default_rng(SEED)
    with np.errstate(all="ignore"):
        ref = {**op_cases(E.NP), **run_cases(O, E.NP)}
        floors = dict.fromkeys(ref, 0.0)
        for r in range(REPEATS):
            X = E.Ext(Nudged(rng), noisy_solve(rng))
            got = {**op_cases(X), **run_cases(O, X)}
            for k in ref:
                floors[k] = max(floors[k], worst(ref[k], got[k]))
            print(f"repeat {r + 1}/{REPEATS}", flush=True)
    path = E.FLOOR_JSON
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"what": "worst |restatement - restatement with every transcendental result "
                           "moved by -1, 0 or +1 ulp and every FFT solve's output by up to "
                           "fft_rel of its max-abs|, per case (tools/mac_ve_ext_floor.py)",
                   "repeats": REPEATS, "seed": SEED, "fft_rel": E.FFT_REL,
                   "bar_factor": E.BAR_FACTOR, "numpy": np.__version__, "floors": floors}, f,
                  indent=1)
        f.write("\n")
    for k, v in floors.items():
        print(f"  {k:40s} {v:.3e}")


if __name__ == "__main__":
    main()
