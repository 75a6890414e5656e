"""Golden-vector generator for the periodic MAC tier's semi-Lagrangian predictor
(pyRMT/mac.py:587-633 and integrator "imex-sl" of benchmarks/mac_taylor_green_convergence.py):
runs the pyRMT reference in pure-Python mode (imported exactly as gen_mac_periodic.py does)
and writes

    tests/golden/mac_periodic_sl.npz          the four small shapes, the two Taylor-Green
                                              switch runs and the run_one results
    tests/golden/mac_periodic_sl_64x64.npz    the operators at 64 x 64
    tests/golden/mac_periodic_sl_33x130.npz   ... at 33 x 130

The u, v, p of the shapes that mac_periodic*.npz already hold are read from those files and
not stored again.  Every file stays under 600 KB.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_mac_periodic_sl.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import M, OUT, save  # noqa: E402
import numpy as np  # noqa: E402
from benchmarks.mac_taylor_green_convergence import run_one, tg_exact, _faces  # noqa: E402

# (ny, nx): the two smallest extents a periodic plane can have, then gen_mac_periodic.py's
SHAPES = ((2, 3), (3, 2), (5, 7), (20, 36), (64, 64), (33, 130))
NU, DT_CENTRAL, SWITCH = 0.05, 1e-3, 0.9
TWO_PI = 2 * np.pi
NPTS = 2000


def inputs(ny, nx):
    """u, v, p: the existing fixtures', or seeded standard_normal at the two tiny shapes."""
    if ny * nx < 10:
        return np.random.default_rng(5150 + 10 * ny + nx).standard_normal((3, ny, nx))
    if ny * nx > 1000:
        g = np.load(os.path.join(OUT, f"mac_periodic_{ny}x{nx}.npz"))
        return g["u"], g["v"], g["p"]
    g = np.load(os.path.join(OUT, "mac_periodic.npz"))
    return tuple(g[f"s{ny}x{nx}_{k}"] for k in "uvp")


def edge_coords(n):
    return [0.0, -0.0, -1e-20, -1e-300, float(n), n - 1e-13, np.nextafter(float(n), 0.0),
            -float(n), 1e6 * n, 1e15, -1e15]


def cfl_of(u, v, dx, dy, dt):
    return dt * max(np.max(np.abs(u)) / dx, np.max(np.abs(v)) / dy)


def gen_shape(ny, nx, seed):
    rng = np.random.default_rng(seed)
    u, v, p = inputs(ny, nx)
    dx, dy = TWO_PI / nx, TWO_PI / ny
    lap = M.lap_eigs_periodic(nx, ny, dx, dy)
    ei, ej = edge_coords(nx), edge_coords(ny)
    iq = np.concatenate([ei, rng.uniform(-3 * nx, 4 * nx, NPTS - len(ei))])
    # the edge coordinates of the two axes meet in every combination of neighbours
    jq = np.concatenate([ej[1:] + ej[:1], rng.uniform(-3 * ny, 4 * ny, NPTS - len(ej))])
    dt_sl = (3.0 if ny * nx < 1000 else 0.7) * min(dx, dy)
    cfl_sl = cfl_of(u, v, dx, dy, dt_sl)
    cfl_c = cfl_of(u, v, dx, dy, DT_CENTRAL)
    assert cfl_sl - SWITCH >= 1e-3 and SWITCH - cfl_c >= 1e-3, (cfl_sl, cfl_c)
    su, sv = M.momentum_predictor_periodic_semilag(u, v, NU, dx, dy, dt_sl, lap)
    # the central branch is momentum_predictor_periodic_imex, bit for bit: iu, iv of the
    # existing fixtures serve as its expected output
    cu, cv = M.momentum_predictor_periodic_semilag(u, v, NU, dx, dy, DT_CENTRAL, lap)
    iu, iv = M.momentum_predictor_periodic_imex(u, v, NU, dx, dy, DT_CENTRAL, lap)
    assert np.array_equal(cu, iu) and np.array_equal(cv, iv)
    au = M._sl_advect_per(u, u, v, 0.0, 0.5, dx, dy, dt_sl)
    av = M._sl_advect_per(v, u, v, 0.5, 0.0, dx, dy, dt_sl)
    back = max(np.abs(dt_sl * u / dx).max(), np.abs(dt_sl * v / dy).max())
    print(f"  {ny}x{nx}: cfl {cfl_sl:.3g} (SL, dt {dt_sl:.3g}), {cfl_c:.2g} (central); "
          f"backtraces up to {back:.2g} cells")
    d = dict(dx=dx, dy=dy, nu=NU, dt_sl=dt_sl, dt_central=DT_CENTRAL, cfl_switch=SWITCH,
             cfl_sl=cfl_sl, cfl_central=cfl_c, iq=iq, jq=jq, interp=M._interp_per(p, iq, jq),
             adv_u=au, adv_v=av, su=su, sv=sv)
    if ny * nx < 10:
        d.update(u=u, v=v, p=p, iu=iu, iv=iv, lap=lap)
    return d


def tg_switch_run(N, nsteps=12, nu=0.05, noise=0.0, seed=0):
    """The "imex-sl" loop of mac_taylor_green_convergence.py:53-66 at dt = 0.95 dx, keeping
    the fields and every step's cfl; noise: relative size of the perturbation added after
    every predictor and every projection."""
    rng = np.random.default_rng(seed)
    dx, Xu, Yu, Xv, Yv = _faces(N)
    dt = 0.95 * dx
    u, v = tg_exact(Xu, Yu, Xv, Yv, nu, 0.0)
    eig = M.poisson_eigs_periodic(N, N, dx, dx)
    lap = M.lap_eigs_periodic(N, N, dx, dx)

    def jitter(a):
        return a + noise * np.abs(a).max() * rng.standard_normal(a.shape) if noise else a
    cfls = []
    for _ in range(nsteps):
        cfls.append(cfl_of(u, v, dx, dx, dt))
        us, vs = M.momentum_predictor_periodic_semilag(u, v, nu, dx, dx, dt, lap)
        us, vs = jitter(us), jitter(vs)
        u, v, p = M.project_per(us, vs, dx, dx, dt, 1.0, eig)
        u, v, p = jitter(u), jitter(v), jitter(p)
    return dt, u, v, p, np.array(cfls)


if __name__ == "__main__":
    t0 = time.time()
    out = dict(shapes=np.array(SHAPES))
    for k, (ny, nx) in enumerate(SHAPES):
        d = gen_shape(ny, nx, 6200 + k)
        if ny * nx > 1000:
            save(f"mac_periodic_sl_{ny}x{nx}", **d)
        else:
            out.update({f"s{ny}x{nx}_{key}": val for key, val in d.items()})
    for N in (64, 45):
        dt, u, v, p, cfls = tg_switch_run(N)
        sl = cfls > SWITCH
        margin = np.abs(cfls - SWITCH).min()
        assert margin >= 1e-3, margin
        # SL first, central afterwards: one crossing inside the run
        nsl = int(sl.sum())
        assert 0 < nsl < len(cfls) and sl[:nsl].all() and not sl[nsl:].any()
        _, un, vn, pn, cn = tg_switch_run(N, noise=1e-12, seed=7700 + N)
        assert np.array_equal(cn > SWITCH, sl), "the noise moved the branch sequence"
        dist = np.array([np.abs(un - u).max(), np.abs(vn - v).max(),
                         np.abs(pn - p).max() / np.abs(p).max()])
        print(f"  TG switch run N={N}: SL in steps 0-{nsl - 1} of {len(cfls)}, nearest approach "
              f"to the switch {margin:.2g}; noise of 1e-12 moves u, v by {dist[0]:.2g}, "
              f"{dist[1]:.2g} and p by {dist[2]:.2g} of max|p|")
        out.update({f"tg{N}_dt": dt, f"tg{N}_u": u, f"tg{N}_v": v, f"tg{N}_p": p,
                    f"tg{N}_cfl": cfls, f"tg{N}_sl_steps": nsl, f"tg{N}_margin": margin,
                    f"tg{N}_noise": dist})
    dxb = TWO_PI / 64
    out["run_dt"] = np.array([0.02, 2 * dxb])
    out["run_sl"] = np.array([run_one(64, nu=0.05, T=1.0, dt=dt, integrator="imex-sl")
                              for dt in out["run_dt"]])
    print(f"  run_one imex-sl: {out['run_sl'].tolist()}")
    save("mac_periodic_sl", **out)
    print(f"done in {time.time() - t0:.0f}s")
