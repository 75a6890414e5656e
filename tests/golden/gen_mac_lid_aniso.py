"""Golden-vector generator for the lid-tier MAC operators and the IMEX tier at dx != dy
(pyRMT/mac.py:81-139, 179-232, 243-442, 656-689, 729-749): runs the pyRMT reference in
pure-Python mode (imported exactly as gen_golden.py does) on square grids over non-square
boxes, dx, dy = mac_grid(N, N, Lx, Ly), and writes

    tests/golden/mac_lid_aniso.npz    N = 5 (1 x 1.25), N = 6 (2 x 1), N = 33 (1 x 1.25)

Per grid (keys n<N>_*): divergence, the two pressure gradients, the explicit lid predictor and
the free-slip one (with and without forces), the interfacial face force, the contact stress of
two overlapping discs, the projection, the homogeneous ghost-cell Laplacians and the DST
Helmholtz eigenvalues, CG / PCG Helmholtz solves of both face kinds (PCG counts through the
reference's `count`), the IMEX predictor (plain; forces + rho + cs2; fu only; fv only) and the
semi-Lagrangian predictor at CFL 3 (plain; forces + cs2).

Every quantity that is not bit-exact on the GPU is computed a second time with one interior
input value moved by one ulp: noise_<name> = max|a - b| / max|a| is the reference's own noise
floor.  The GPU tests hold to 1e-12 where the floor is at most a tenth of that, else to ten
times the floor.  Every CG the reference runs here goes through a recording wrapper of
scipy's cg (the solve itself untouched): the stopping test's ||r|| / atol must be >= 1.05 on
the trips that run and <= 0.95 where it stops, so that an equal iteration count is a fair
demand of another implementation; a seed that violates it is replaced.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz file is data.

Usage:  python -B tests/golden/gen_mac_lid_aniso.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import F, M, OUT, save  # noqa: E402,F401
import numpy as np  # noqa: E402
import mac_lid_aniso_np as A  # noqa: E402

# (N = 6: seed 9206 left two PCG solves within 5 % of atol on their last trip, ratio 1.014)
SEEDS = {5: 9205, 6: 9306, 33: 9233}
COEF = 0.5e-3
SOLVES = []     # (iterations, ratios, maxiter) of every cg the reference ran


def _cg_recorded(orig):
    def cg(Aop, b, x0=None, *, rtol=1e-5, atol=0.0, maxiter=None, M=None, callback=None):
        at = rtol * np.linalg.norm(b)
        ratios = [np.linalg.norm(b - Aop.matvec(x0)) / at]

        def cb(xk):
            ratios.append(np.linalg.norm(b - Aop.matvec(xk)) / at)
            if callback is not None:
                callback(xk)
        r = orig(Aop, b, x0=x0, rtol=rtol, atol=atol, maxiter=maxiter, M=M, callback=cb)
        SOLVES.append((len(ratios) - 1, ratios, maxiter))
        return r
    return cg


noise = A.with_noise


def gen_grid(N, box):
    dx, dy = M.mac_grid(N, N, *A.BOXES[box])
    assert (dx, dy) == A.spacing(N, box) and dx != dy
    d = A.op_inputs(N, SEEDS[N])
    u, v, fu, fv = d["u"], d["v"], d["fu"], d["fv"]
    out = dict(d, dx=dx, dy=dy)
    # ---- bit-exact operators
    out["div"] = M.divergence(u, v, dx, dy)
    out["gpu"] = M.gradient_p_u(d["p"], dx)
    out["gpv"] = M.gradient_p_v(d["p"], dy)
    out["gu"], out["gv"] = M.interfacial_force_faces(d["kappa"], d["H"], A.GAMMA, dx, dy)
    pa, pb = A.discs(N, dx, dy)
    eps = 3 * max(dx, dy)
    t3 = M.contact_stress(pa, pb, A.ETA, A.GSUM, eps, dx, dy)
    nz = t3[0] != 0
    assert nz[1:-1, 1:-1].any() and (nz[0].any() or nz[-1].any()) and \
        (nz[:, 0].any() or nz[:, -1].any()), "contact cells: interior, a boundary row and column"
    out.update(pa=pa, pb=pb, eps=eps, txx=t3[0], txy=t3[1], tyy=t3[2])
    out["lap_u"] = M._lap_u_lid_hom(u, dx, dy)
    out["lap_v"] = M._lap_v_lid_hom(v, dx, dy)
    out["eig_u"] = M._dst_helmholtz_eigs((N, N - 1), dx, dy)
    out["eig_v"] = M._dst_helmholtz_eigs((N - 1, N), dx, dy)
    # ---- the explicit predictors (bit-exact on the GPU)
    base = (u, v, A.NU, dx, dy, A.DT)
    forces = dict(fu=fu, fv=fv, rho=A.RHO)
    out["mp_us0"], out["mp_vs0"] = M.momentum_predictor(*base, A.U_LID)
    out["mp_us1"], out["mp_vs1"] = M.momentum_predictor(*base, A.U_LID, **forces)
    out["fs_us0"], out["fs_vs0"] = M.momentum_predictor_freeslip(*base)
    out["fs_us1"], out["fs_vs1"] = M.momentum_predictor_freeslip(*base, **forces)
    # ---- projection of the forced explicit predictor's result
    eig = M.poisson_eigs_neumann(N, N, dx, dy)
    out["pu"], out["pv"], out["pp"] = M.project(out["mp_us1"], out["mp_vs1"], dx, dy, A.DT,
                                                A.RHO, eig)
    b3 = M.project(A.nudge(out["mp_us1"]), out["mp_vs1"], dx, dy, A.DT, A.RHO, eig)
    out["noise_pu"], out["noise_pv"], out["noise_pp"] = (
        A.rel(b3[k], out[n]) for k, n in enumerate(("pu", "pv", "pp")))
    assert np.abs(M.divergence(out["pu"], out["pv"], dx, dy)).max() < 1e-9
    # ---- CG / PCG Helmholtz solves, both kinds
    emb = (lambda x: np.pad(x, ((0, 0), (1, 1))), lambda x: np.pad(x, ((1, 1), (0, 0))))
    lap = (lambda w: M._lap_u_lid_hom(w, dx, dy), lambda w: M._lap_v_lid_hom(w, dx, dy))
    for kind, tag in ((0, "u"), (1, "v")):
        rhs = d["rhs_" + tag]
        (out["cg_" + tag],), out["noise_cg_" + tag] = noise(
            M._cg_helmholtz, (rhs, lap[kind], emb[kind], COEF), 0)
        cnt = []
        (out["pcg_" + tag],), out["noise_pcg_" + tag] = noise(
            M._pcg_helmholtz, (rhs, lap[kind], emb[kind], COEF, dx, dy), 0,
            dict(rtol=1e-8, count=cnt))
        assert cnt[0] == cnt[1], cnt
        out["cnt_" + tag] = cnt[0]
    # ---- IMEX predictor: plain, forces + rho + cs2, one-sided forces
    lid = base + (A.U_LID,)
    for tag, kw in (("0", {}), ("1", dict(forces, cs2=A.CS2)), ("fu", dict(fu=fu, rho=A.RHO)),
                    ("fv", dict(fv=fv, rho=A.RHO))):
        (out["ix_us" + tag], out["ix_vs" + tag]), out["noise_ix" + tag] = noise(
            M.momentum_predictor_lid_imex, lid, 0, kw)
    # ---- semi-Lagrangian predictor at CFL 3: backtraces leave the box
    dts = A.semilag_dt(u, v, dx, dy, 3.0)
    cfl = dts * max(np.max(np.abs(u)) / dx, np.max(np.abs(v)) / dy)
    assert cfl > 0.9 and 2.0 < cfl < 5.0, cfl
    sl = (u, v, A.NU, dx, dy, dts, A.U_LID)
    for tag, kw in (("0", {}), ("1", dict(forces, cs2=A.CS2))):
        (out["sl_us" + tag], out["sl_vs" + tag]), out["noise_sl" + tag] = noise(
            M.momentum_predictor_lid_semilag, sl, 0, kw)
    out["dt_sl"] = dts
    noises = {k: float(val) for k, val in out.items() if k.startswith("noise_")}
    print(f"  N={N} {box}: dx/dy {dx / dy:g}, PCG counts {out['cnt_u']}, {out['cnt_v']}, "
          f"semilag CFL {cfl:.2f}; noise max {max(noises.values()):.2g} "
          f"({max(noises, key=noises.get)})")
    for k, val in noises.items():
        if val > 0.1 * A.BAR_FIXTURE:
            print(f"    {k} = {val:.3g}: above a tenth of {A.BAR_FIXTURE:g}, the bar is 10 x it")
    return {f"n{N}_{k}": val for k, val in out.items()}


if __name__ == "__main__":
    t0 = time.time()
    M.cg = _cg_recorded(M.cg)
    out = {}
    for N, box in A.FIXTURE_GRIDS:
        n0 = len(SOLVES)
        out.update(gen_grid(N, box))
        for it, ratios, mx in SOLVES[n0:]:
            assert A.margin_ok(ratios, it, mx), (N, it, ratios[-2:])
        print(f"    {len(SOLVES) - n0} CG solves, stopping ratios within the margins")
    save("mac_lid_aniso", Ns=np.array([g[0] for g in A.FIXTURE_GRIDS]), nu=A.NU, dt=A.DT,
         rho=A.RHO, gamma=A.GAMMA, U_lid=A.U_LID, cs2=A.CS2, eta=A.ETA, Gsum=A.GSUM, coef=COEF,
         **out)
    size = os.path.getsize(os.path.join(OUT, "mac_lid_aniso.npz"))
    assert size <= 600 * 1024, size
    print(f"done in {time.time() - t0:.0f}s")
