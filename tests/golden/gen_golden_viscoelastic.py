"""Golden-vector generator for the viscoelastic constitutive layer: runs the pyRMT reference
(pyRMT/viscoelastic.py and benchmarks/mac_viscoelastic_uniform.py, imported exactly as
gen_golden.py does) and writes

    tests/golden/viscoelastic_ops.npz        every operator on tests/viscoelastic_np.py's shared
                                             inputs, the special values, the gap ladder, the
                                             Taylor-Green runs and the 0-D set-ups
    tests/golden/viscoelastic_uniform32.npz  run(N=32, t_end=11.5 dt) for tau = 0.5 and tau = inf:
                                             12 steps (the last clipped to dt / 2), the per-step
                                             record and the final state

The uniform-extension loop is not restated here: the driver's own run() is called and its state
captured by wrapping the names the driver module looks up per call.  To keep the files small the
(33, 70) shape stores the bit-exact operators only (the tests hold the others to the restatement
there, which the smaller shapes pin to the reference).

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_golden_viscoelastic.py
"""
import contextlib
import io
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import save  # noqa: E402
import numpy as np  # noqa: E402
import pyRMT.viscoelastic as R  # noqa: E402
import benchmarks.mac_viscoelastic_uniform as U  # noqa: E402
import benchmarks.viscoelastic_taylor_green as TG  # noqa: E402
import benchmarks.viscoelastic_relaxation_test as RT  # noqa: E402
import viscoelastic_np as V  # noqa: E402

ST = np.stack


def gen_ops():
    out = {}
    for shape in V.SHAPES:
        g, k = V.op_inputs(shape), V.key(shape)
        b, psi, Lc = g["b"], g["psi"], g["L"]
        out[f"{k}_ucm_step"] = ST(R.ucm_local_step(*b, *Lc, V.TAU, V.DT))
        out[f"{k}_stress_zener"] = ST(R.viscoelastic_stress(*b, V.G, g["bref"], V.G_INF))
        if shape == (33, 70):
            continue
        out[f"{k}_ucm_rhs"] = ST(R.ucm_local_rhs(*b, *Lc, V.TAU))
        out[f"{k}_ucm_step_inf"] = ST(R.ucm_local_step(*b, *Lc, np.inf, V.DT))
        out[f"{k}_stress"] = ST(R.viscoelastic_stress(*b, V.G))
        out[f"{k}_stress_ginf0"] = ST(R.viscoelastic_stress(*b, V.G, g["bref"], 0.0))
        out[f"{k}_sym_log"] = ST(R.sym_log(*b))
        out[f"{k}_sym_exp"] = ST(R.sym_exp(*psi))
        out[f"{k}_logconf_rhs"] = ST(R.logconf_local_rhs(*psi, *Lc, V.TAU))
        out[f"{k}_step_explicit"] = ST(R.logconf_local_step(*psi, *Lc, V.TAU, V.DT))
        out[f"{k}_step_strang"] = ST(R.logconf_local_step_strang(*psi, *Lc, V.TAU, V.DT))
        out[f"{k}_relax_exact"] = ST(R.relax_exact(*psi, V.TAU, V.DT))
    with np.errstate(all="ignore"):
        s = V.special_inputs()
        out["special_sym_log"] = ST(R.sym_log(*s["neg"]))
        out["special_sym_exp"] = ST(R.sym_exp(*s["psi"]))
        out["special_rhs"] = ST(R.logconf_local_rhs(*s["psi"], *s["L"], V.TAU))
        out["special_step_explicit"] = ST(R.logconf_local_step(*s["psi"], *s["L"], V.TAU, V.DT))
        out["special_step_strang"] = ST(R.logconf_local_step_strang(*s["psi"], *s["L"], V.TAU,
                                                                     V.DT))
    for gap in V.GAPS:
        g = V.gap_inputs(gap)
        out[f"gap_{gap:g}"] = ST(R.logconf_local_rhs(*g["psi"], *g["L"], V.TAU))
    for N in V.TG_N:
        Lc = TG.tg_velocity_gradient(N)
        np.testing.assert_array_equal(ST(Lc), ST(V.tg_velocity_gradient(N)))
        for tau, dt in V.TG_CASES:
            for strang, step in ((False, R.logconf_local_step),
                                 (True, R.logconf_local_step_strang)):
                p = [np.zeros((N, N))] * 3
                for _ in range(V.TG_STEPS):
                    p = step(*p, *Lc, tau, dt)
                out[V.tg_key(N, tau, dt, strang)] = ST(p)
    out["tg_compare"] = np.array(TG.run_compare(*V.TG_COMPARE))
    for n, (b, Lc, tau) in enumerate(V.relaxation_setups()):
        for _ in range(2000):
            b = R.ucm_local_step(*b, *Lc, tau, 2e-4)
        out[f"zero_d{n}"] = np.array(b)
    with contextlib.redirect_stdout(io.StringIO()):     # the 0-D driver's three errors
        out["relaxation"] = np.array([RT.test_step_relaxation(), RT.test_steady_shear(),
                                      RT.test_elastic_limit()])
    assert out["relaxation"][0] < 1e-3 and out["relaxation"][1] < 1e-3
    assert out["relaxation"][2] < 1e-6
    save("viscoelastic_ops", **out)


class Tap:
    """Wraps the driver module's operators; one dict per step."""

    NAMES = ("rebuild_phi_from_reference_map", "extrapolate_reference_map", "logconf_local_step",
             "sym_exp")

    def __init__(self):
        self.steps, self.orig = [], {k: getattr(U, k) for k in self.NAMES}

    def __enter__(self):
        for k in self.NAMES:
            setattr(U, k, getattr(self, "w_" + k))
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(U, k, f)

    def w_rebuild_phi_from_reference_map(self, *a):
        phi = self.orig["rebuild_phi_from_reference_map"](*a)
        self.steps.append(dict(phi=phi.copy(), n_extrap=0))
        return phi

    def w_extrapolate_reference_map(self, *a):
        out = self.orig["extrapolate_reference_map"](*a)
        if self.steps:      # (the initial extrapolation comes before the first step)
            s = self.steps[-1]
            s["n_extrap"] += 1
            if s["n_extrap"] == 1:
                s["X1"], s["X2"] = out[0].copy(), out[1].copy()
        return out

    def w_logconf_local_step(self, *a):
        out = self.orig["logconf_local_step"](*a)
        self.steps[-1].update(psi=ST(out), dt=a[-1], tau=a[-2])
        return out

    def w_sym_exp(self, *a):
        out = self.orig["sym_exp"](*a)
        self.steps[-1]["be"] = ST(out)
        return out


def gen_uniform():
    N = V.UNI_N
    out = dict(N=N, steps=V.UNI_STEPS)
    for tau in V.UNI_TAUS:
        dx = 1.0 / N       # the driver's dt (:60) at its default eps_rate, mu_f, rho, G
        dt = min(0.25 * dx / max(0.5 * 0.5, 0.1), 0.2 * dx * dx / 0.02,
                 0.3 * dx / (np.sqrt(0.3) + 1e-9))
        t_end = (V.UNI_STEPS - 0.5) * dt
        with Tap() as tap, contextlib.redirect_stdout(io.StringIO()), \
                tempfile.TemporaryDirectory() as tmp:
            t_ret, hist = U.run(N=N, t_end=t_end, tau=(0.0 if tau == np.inf else tau),
                                out_root=tmp)
        S = tap.steps
        assert len(S) == V.UNI_STEPS and all(s["n_extrap"] == 3 for s in S), len(S)
        assert all(s["tau"] == tau for s in S)
        rec, t = [], 0.0
        for s in S:
            t += s["dt"]
            sm = s["phi"] <= 0
            assert sm.any()
            lam = float(U._lam_max(*s["be"])[sm].max())
            rec.append((t, lam, float(s["be"][0][N // 2, N // 2]), int(sm.sum())))
        assert t == t_ret and S[-1]["dt"] < 0.75 * dt
        assert hist[-1][:3] == rec[-1][:3], (hist[-1], rec[-1])     # run()'s own last record
        k = f"tau{tau:g}_"
        out.update({k + "record": np.array(rec), k + "dts": np.array([s["dt"] for s in S]),
                    k + "X1": S[-1]["X1"], k + "X2": S[-1]["X2"], k + "phi": S[-1]["phi"],
                    k + "psi": S[-1]["psi"], k + "be": S[-1]["be"], k + "t_end": t_end})
        print(f"  tau={tau}: t={t:.6f} lam={rec[-1][1]:.6f} b_xx(c)={rec[-1][2]:.6f} "
              f"solid cells {rec[-1][3]}")
    save("viscoelastic_uniform32", **out)


if __name__ == "__main__":
    gen_ops()
    gen_uniform()
