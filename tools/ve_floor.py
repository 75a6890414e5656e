"""The noise floor of the viscoelastic operators: how far the NumPy restatement
(tests/viscoelastic_np.py) moves when every exp, log, sin, cos and arctan2 result is moved by
-1, 0 or +1 ulp at random -- the size of difference that two correct math libraries produce.
Each case of the GPU tests is run REPEATS times against its unmoved self and the worst absolute
difference kept; the tests hold the device to BAR_FACTOR times that (viscoelastic_np.bar).
sqrt and the arithmetic are correctly rounded on every side and stay as they are.

Usage:  python tools/ve_floor.py        (CPU only; writes profiles/viscoelastic/floor.json)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import viscoelastic_np as V  # noqa: E402

REPEATS, SEED = 20, 20240


class Nudged:
    """np's transcendentals with each finite non-zero result moved by -1, 0 or +1 ulp."""

    def __init__(self, rng):
        self.rng = rng

    def _move(self, r):
        r = np.asarray(r, dtype=np.float64)
        k = self.rng.integers(-1, 2, size=r.shape)
        moved = np.where(k > 0, np.nextafter(r, np.inf), np.where(k < 0, np.nextafter(r, -np.inf), r))
        out = np.where(np.isfinite(r) & (r != 0.0), moved, r)
        return out if out.ndim else float(out)

    def exp(self, x): return self._move(np.exp(x))
    def log(self, x): return self._move(np.log(x))
    def sin(self, x): return self._move(np.sin(x))
    def cos(self, x): return self._move(np.cos(x))
    def arctan2(self, y, x): return self._move(np.arctan2(y, x))


def worst(ref, got):
    """Largest |difference| over the planes, over the entries finite on both sides."""
    w = 0.0
    for a, b in zip(ref, got):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        ok = np.isfinite(a) & np.isfinite(b)
        if ok.any():
            w = max(w, float(np.abs(a[ok] - b[ok]).max()))
    return w


def op_cases(ops):
    """name -> planes, for every operator case on the shared inputs (all shapes and LONG_N in
    one go: the floor of a case is its worst over them)."""
    out = {}
    for shape in V.SHAPES + ((V.LONG_N,),):
        g = V.op_inputs(shape)
        res = {"sym_log": ops.sym_log(*g["b"]), "sym_exp": ops.sym_exp(*g["psi"]),
               "relax_exact": ops.relax_exact(*g["psi"], V.TAU, V.DT),
               "logconf_rhs": ops.logconf_local_rhs(*g["psi"], *g["L"], V.TAU),
               "step_explicit": ops.logconf_local_step(*g["psi"], *g["L"], V.TAU, V.DT),
               "step_strang": ops.logconf_local_step_strang(*g["psi"], *g["L"], V.TAU, V.DT),
               "step7_explicit": ops.logconf_local_step(*g["psi"], *g["L"], V.TAU, V.DT, 7),
               "step7_strang": ops.logconf_local_step_strang(*g["psi"], *g["L"], V.TAU, V.DT, 7)}
        if shape == (V.LONG_N,):
            res = {k: v for k, v in res.items() if not k.startswith("step7")}
        for k, v in res.items():
            out.setdefault(k, []).extend(np.ravel(p) for p in v)
    s = V.special_inputs()
    out["special_sym_log"] = ops.sym_log(*s["neg"])
    out["special_sym_exp"] = ops.sym_exp(*s["psi"])
    out["special_rhs"] = ops.logconf_local_rhs(*s["psi"], *s["L"], V.TAU)
    out["special_step_explicit"] = ops.logconf_local_step(*s["psi"], *s["L"], V.TAU, V.DT)
    out["special_step_strang"] = ops.logconf_local_step_strang(*s["psi"], *s["L"], V.TAU, V.DT)
    for gap in V.GAPS:
        g = V.gap_inputs(gap)
        out[f"gap_{gap:g}"] = ops.logconf_local_rhs(*g["psi"], *g["L"], V.TAU)
    for N in V.TG_N:
        for tau, dt in V.TG_CASES:
            for strang in (False, True):
                out[V.tg_key(N, tau, dt, strang)] = V.tg_run(ops, N, tau, dt, strang)
    d, me, ms = V.tg_compare(ops, *V.TG_COMPARE)
    out["tg_compare_diff"], out["tg_compare_min_eig_explicit"] = [d], [me]
    out["tg_compare_min_eig_strang"] = [ms]
    return out


def loop_cases(O, ops):
    out = {}
    for tau in V.UNI_TAUS:
        sim = V.UniformLoop(O, ops, tau=tau).step(V.UNI_STEPS)
        rec = np.array(sim.record)
        k = f"uni_tau{tau:g}_"
        out[k + "maps"] = [sim.X1, sim.X2]
        out[k + "psi"] = sim.psi
        out[k + "be"] = sim.be
        out[k + "lam"] = [rec[:, 1]]
        out[k + "bxx"] = [rec[:, 2]]
    return out


def main():
    from oracle import oracle as O
    rng = np.random.default_rng(SEED)
    with np.errstate(all="ignore"):
        ref = {**op_cases(V.NP), **loop_cases(O, V.NP)}
        floors = dict.fromkeys(ref, 0.0)
        for r in range(REPEATS):
            nud = V.Ops(Nudged(rng))
            got = {**op_cases(nud), **loop_cases(O, nud)}
            for k in ref:
                floors[k] = max(floors[k], worst(ref[k], got[k]))
            print(f"repeat {r + 1}/{REPEATS}", flush=True)
    # the velocity is imposed, so no transcendental reaches the maps: they are an == case
    for k in [k for k in floors if k.endswith("_maps")]:
        assert floors.pop(k) == 0.0, k
    path = V.FLOOR_JSON
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"what": "worst |restatement - restatement with every transcendental result "
                           "moved by -1, 0 or +1 ulp|, per case (tools/ve_floor.py)",
                   "repeats": REPEATS, "seed": SEED, "bar_factor": V.BAR_FACTOR,
                   "numpy": np.__version__, "floors": floors}, f, indent=1)
        f.write("\n")
    for k, v in floors.items():
        print(f"  {k:40s} {v:.3e}")


if __name__ == "__main__":
    main()
