"""Golden-vector generator for the periodic MAC tier (pyRMT/mac.py:445-540, 636-650 and
benchmarks/mac_taylor_green_convergence.py): runs the pyRMT reference in pure-Python mode
(imported exactly as gen_golden.py does) and writes

    tests/golden/mac_periodic.npz          the two small shapes, the run_one results and the
                                           500-step Taylor-Green states
    tests/golden/mac_periodic_64x64.npz    the operators on one exact 64 x 64 tile
    tests/golden/mac_periodic_33x130.npz   ... on a tile edge crossed in x, odd ny

Full-entropy float64 planes do not compress, so the contents are split: every file stays
under 600 KB.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_mac_periodic.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import M, OUT, save  # noqa: E402
import numpy as np  # noqa: E402
from benchmarks.mac_taylor_green_convergence import run_one, tg_exact, _faces  # noqa: E402

# (ny, nx): below any tile; odd nx (half-spectrum width, no Nyquist column); one exact
# 64 x 64 tile; a tile edge crossed in x with the wrap inside a partial tile, odd ny
SHAPES = ((5, 7), (20, 36), (64, 64), (33, 130))
NU, DT, RHO, COEF = 0.05, 1e-3, 1.3, 0.7
TWO_PI = 2 * np.pi


def gen_shape(ny, nx, seed):
    rng = np.random.default_rng(seed)
    u, v, p = rng.standard_normal((3, ny, nx))
    dx, dy = TWO_PI / nx, TWO_PI / ny           # dx != dy on the rectangular shapes
    eig = M.poisson_eigs_periodic(nx, ny, dx, dy)
    lap = M.lap_eigs_periodic(nx, ny, dx, dy)
    pu, pv = M.momentum_predictor_periodic(u, v, NU, dx, dy, DT)
    iu, iv = M.momentum_predictor_periodic_imex(u, v, NU, dx, dy, DT, lap)
    qu, qv, phi = M.project_per(u, v, dx, dy, DT, RHO, eig)
    left = np.abs(M.divergence_per(qu, qv, dx, dy)).max() / np.abs(M.divergence_per(u, v, dx, dy)).max()
    print(f"  {ny}x{nx}: max|div| after / before the reference's projection = {left:.2g}")
    return dict(dx=dx, dy=dy, nu=NU, dt=DT, rho=RHO, coef=COEF, u=u, v=v, p=p,
                div=M.divergence_per(u, v, dx, dy), gu=M.grad_p_u_per(p, dx),
                gv=M.grad_p_v_per(p, dy), pu=pu, pv=pv, eig=eig, lap=lap,
                sol_p=M.solve_poisson_periodic(p, eig),
                sol_h=M.solve_helmholtz_periodic(p, lap, COEF), iu=iu, iv=iv,
                proj_u=qu, proj_v=qv, proj_phi=phi)


def tg_state(N, imex, nsteps=500, nu=0.05, dt=2e-4):
    """The loop of mac_taylor_green_convergence.py:53-66, keeping the fields."""
    dx, Xu, Yu, Xv, Yv = _faces(N)
    u, v = tg_exact(Xu, Yu, Xv, Yv, nu, 0.0)
    eig = M.poisson_eigs_periodic(N, N, dx, dx)
    lap = M.lap_eigs_periodic(N, N, dx, dx)
    for _ in range(nsteps):
        if imex:
            us, vs = M.momentum_predictor_periodic_imex(u, v, nu, dx, dx, dt, lap)
        else:
            us, vs = M.momentum_predictor_periodic(u, v, nu, dx, dx, dt)
        u, v, p = M.project_per(us, vs, dx, dx, dt, 1.0, eig)
    return u, v, p


if __name__ == "__main__":
    t0 = time.time()
    out = dict(shapes=np.array(SHAPES))
    for k, (ny, nx) in enumerate(SHAPES):
        d = gen_shape(ny, nx, 4450 + k)
        if ny * nx > 1000:
            save(f"mac_periodic_{ny}x{nx}", **d)
        else:
            out.update({f"s{ny}x{nx}_{key}": val for key, val in d.items()})
    # run_one: the convergence pair (tests/test_mac.py:161-169), explicit and IMEX, and the
    # IMEX run at 6x the explicit viscous limit (test_mac.py:188-199)
    for name, kw in (("exp", {}), ("imex", {"integrator": "imex"})):
        out["tg_" + name] = np.array([run_one(N, nu=0.05, T=0.1, dt=2e-4, **kw) for N in (32, 64)])
        print(f"  run_one {name}: {out['tg_' + name].tolist()}")
    dxb = TWO_PI / 64
    out["tg_big_dt"] = 6.0 * dxb ** 2 / (4 * 0.2)
    out["tg_big"] = np.array(run_one(64, nu=0.2, T=2.0, dt=out["tg_big_dt"], implicit_visc=True))
    print(f"  run_one imex big dt: {out['tg_big'].tolist()}")
    for N in (64, 45):
        for name, imex in (("exp", False), ("imex", True)):
            u, v, p = tg_state(N, imex)
            out.update({f"tg{N}_{name}_u": u, f"tg{N}_{name}_v": v, f"tg{N}_{name}_p": p})
    save("mac_periodic", **out)
    print(f"done in {time.time() - t0:.0f}s")
