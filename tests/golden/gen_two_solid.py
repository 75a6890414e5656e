"""Golden-vector generator for the two-solid / surface-tension operators: runs the pyRMT
reference in pure-Python mode (imported exactly as gen_golden.py does: the numba, pyamg and
h5py stand-ins and the exp patch) and writes tests/golden/two_solid.npz.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz is data.

Usage:  python -B tests/golden/gen_two_solid.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import F, C, OUT, save  # noqa: E402
import numpy as np  # noqa: E402

SHAPES = ((48, 48), (64, 128), (35, 130))   # (ny, nx): below one 64 x 16 tile; exact tile
# multiples; a last tile narrower than the halo in both axes, dx != dy
R, K_REP, DT = 0.15, 2.0, 1e-3
MU_S, KAPPA, ETA_S, RHO_S, RHO_F, MU_F = 1.0, 0.3, 0.0, 1.2, 1.0, 0.01


def two_discs(ny, nx, xa=0.35, xb=0.65):
    """tests/test_contact.py:45-62 set-up: two discs and their extrapolated maps."""
    X, Y, dx, dy = F.create_grid(nx, ny, 1.0, 1.0)
    pa = F.apply_phi_BCs(C.initialize_disc(X, Y, xa, 0.5, R))
    pb = F.apply_phi_BCs(C.initialize_disc(X, Y, xb, 0.5, R))
    ma = (pa <= 0).astype(float); mb = (pb <= 0).astype(float)
    X1a, X2a = F.extrapolate_reference_map(X * ma, Y * ma, pa, dx, dy, 3)
    X1b, X2b = F.extrapolate_reference_map(X * mb, Y * mb, pb, dx, dy, 3)
    return X, Y, dx, dy, pa, pb, X1a, X2a, X1b, X2b


def gen_shape(ny, nx, out):
    X, Y, dx, dy, pa, pb, X1a, X2a, X1b, X2b = two_discs(ny, nx)
    w_t, w_c = 2 * dx, 3 * dx
    # smooth, non-zero velocity and pressure, rounded to half precision's 11 significant bits
    # (stored as float64: the file stays small, and they are inputs, so any values do)
    h16 = lambda q: q.astype(np.float16).astype(np.float64)
    u, v = C.taylor_green_velocity(X, Y, U0=0.05)
    u, v = C.free_slip_box_bc(h16(u), h16(v))
    p = h16(0.1 * np.cos(np.pi * X) * np.cos(np.pi * Y))
    kap = F.compute_curvature(pa, dx, dy)
    fx, fy = F.compute_contact_force(pa, pb, K_REP, w_c, dx, dy)
    assert np.abs(fx).max() > 0, "contact fixture without a contact force"
    Ha = F.smoothed_heaviside(pa, w_t); Hb = F.smoothed_heaviside(pb, w_t)
    assert np.any((Ha < 1) & (Hb < 1)), "no cell in both solids' blend regions"
    print(f"  {ny}x{nx}: max|fx| = {np.abs(fx).max():.3g}, "
          f"{int(np.sum((Ha < 1) & (Hb < 1)))} cells in both blend regions")
    k = f"s{ny}x{nx}_"
    # (pa, pb are not stored: sqrt and the arithmetic around it are exact, tests rebuild them)
    out.update({k + "dx": dx, k + "dy": dy, k + "X1a": X1a,
                k + "X2a": X2a, k + "X1b": X1b, k + "X2b": X2b, k + "u": u, k + "v": v, k + "p": p,
                k + "kap": kap, k + "fx": fx, k + "fy": fy, k + "fc_max": np.abs(fx).max(),
                k + "both": int(np.sum((Ha < 1) & (Hb < 1)))})
    for name, kr in (("k2", K_REP), ("k0", 0.0)):
        un, vn, Jm = F.momentum_step_rk4_2solids(
            u, v, p, X1a, X2a, X1b, X2b, C.free_slip_box_bc, MU_S, KAPPA, ETA_S, dx, dy, DT,
            RHO_S, RHO_F, pa, pb, MU_F, w_t, k_rep=kr, w_c=w_c)
        out.update({k + name + "_u": un, k + name + "_v": vn, k + name + "_J": Jm})
    assert not np.array_equal(out[k + "k2_u"], out[k + "k0_u"]), "contact force has no effect"
    assert np.array_equal(out[k + "k2_J"], out.pop(k + "k0_J"))
    # the k_rep = 0 result is stored where it differs from the k_rep = 2 one (near the contact)
    for c in "uv":
        d = np.flatnonzero(out[k + "k2_" + c] != out[k + "k0_" + c])
        out[k + "k0_" + c + "_idx"] = d
        out[k + "k0_" + c + "_val"] = out.pop(k + "k0_" + c).ravel()[d]
    if (ny, nx) != SHAPES[0]:
        return
    # projection with the mixture density at rho_s == rho_f == 1: constant to rounding only
    rho = (Ha + Hb - 1) * 1.0 + (1 - Ha) * 1.0 + (1 - Hb) * 1.0
    ptp = float(np.ptp(rho))
    assert 0 < ptp <= 1e-10 and not np.all(rho == rho.flat[0]), ptp
    eig = F._precompute_poisson_eigenvalues(nx, ny, dx, dy)
    a, b, pn, _, _ = F.pressure_projection_amg(u, v, dx, dy, DT, rho, C.free_slip_box_bc,
                                               p_prev=p, eigenvalues=eig)
    out.update({k + "rho": rho, k + "rho_ptp": ptp, k + "proj_a": a, k + "proj_b": b,
                k + "proj_p": pn})
    print(f"  ptp(rho) = {ptp:.2g}")


def gen_surface_tension(out):
    """momentum_step_rk4(gamma = 0.1) on the inputs of operators.npz, with the parameters of
    its free-slip momentum case."""
    o = np.load(os.path.join(OUT, "operators.npz"))
    dx, dy = float(o["dx"]), float(o["dy"])
    args = (o["a"], o["b"], o["p"], o["X1"], o["X2"], C.free_slip_box_bc, 0.7, 0.3, 0.02, dx, dy,
            2e-3, 1.0, 1.0, o["phi"], 0.01, 2 * dx)
    m = F.momentum_step_rk4(*args, 0.1)
    m0 = F.momentum_step_rk4(*args, 0.0)
    move = float(np.abs(m[0] - m0[0]).max())
    assert move > 1e-6, move
    out.update(st_u=m[0], st_v=m[1], st_J=m[5], st_move=move)
    print(f"  surface tension: gamma = 0.1 moves u by {move:.3g}")


def gen_driver(out, N=48, nsteps=6, xa0=0.34, xb0=0.66, V0=0.15):
    """The loop body of benchmarks/two_disc_contact.py:70-104 through the reference's
    operators, in the driver's order and with its parameters."""
    X, Y, dx, dy = F.create_grid(N, N, 1.0, 1.0)
    yc = 0.5
    ia = lambda Xq, Yq: C.initialize_disc(Xq, Yq, xa0, yc, R)
    ib = lambda Xq, Yq: C.initialize_disc(Xq, Yq, xb0, yc, R)
    phi_a = F.apply_phi_BCs(ia(X, Y)); phi_b = F.apply_phi_BCs(ib(X, Y))
    mu_s, kappa, rho_s, eta_s, mu_f, rho_f = 1.0, 0.0, 1.0, 0.0, 0.01, 1.0
    w_t, w_c = 2.0 * dx, 3.0 * dx
    nl = max(3, C.check_narrow_band(w_t, dx, 3))
    ma = (phi_a <= 0).astype(float); mb = (phi_b <= 0).astype(float)
    X1a, X2a = F.extrapolate_reference_map(X * ma, Y * ma, phi_a, dx, dy, nl)
    X1b, X2b = F.extrapolate_reference_map(X * mb, Y * mb, phi_b, dx, dy, nl)
    Ha = F.smoothed_heaviside(phi_a, w_t); Hb = F.smoothed_heaviside(phi_b, w_t)
    a = V0 * (1 - Ha) - V0 * (1 - Hb)
    b = np.zeros((N, N))
    a, b = C.free_slip_box_bc(a, b)
    p = np.zeros((N, N))
    eig = F._precompute_poisson_eigenvalues(N, N, dx, dy)
    t = 0.0; rec = []
    for _ in range(nsteps):
        dt = F.compute_timestep(a, b, dx, dy, 0.2, 1e-3, mu_s, rho_s, 0.0, rho_f, mu_f=mu_f,
                                kappa=kappa)
        phi_a = F.rebuild_phi_from_reference_map(X1a, X2a, ia)
        phi_b = F.rebuild_phi_from_reference_map(X1b, X2b, ib)
        ma = (phi_a <= 0).astype(float); mb = (phi_b <= 0).astype(float)
        adv = lambda q, ph: F.advect_reference_map(q, a, b, X, Y, dt, dx, dy, ph,
                                                   'semilagrangian', 0.0)
        X1a = adv(X1a, phi_a) * ma; X2a = adv(X2a, phi_a) * ma
        X1b = adv(X1b, phi_b) * mb; X2b = adv(X2b, phi_b) * mb
        X1a, X2a = F.extrapolate_reference_map(X1a, X2a, phi_a, dx, dy, nl)
        X1b, X2b = F.extrapolate_reference_map(X1b, X2b, phi_b, dx, dy, nl)
        phi_a = F.rebuild_phi_from_reference_map(X1a, X2a, ia)
        phi_b = F.rebuild_phi_from_reference_map(X1b, X2b, ib)
        fcx, _ = F.compute_contact_force(phi_a, phi_b, K_REP, w_c, dx, dy)
        assert np.abs(fcx).max() > 0, "driver step without a contact force"
        a_star, b_star, Jmin = F.momentum_step_rk4_2solids(
            a, b, p, X1a, X2a, X1b, X2b, C.free_slip_box_bc, mu_s, kappa, eta_s, dx, dy, dt,
            rho_s, rho_f, phi_a, phi_b, mu_f, w_t, k_rep=K_REP, w_c=w_c)
        Ha = F.smoothed_heaviside(phi_a, w_t); Hb = F.smoothed_heaviside(phi_b, w_t)
        rho_local = (Ha + Hb - 1) * rho_f + (1 - Ha) * rho_s + (1 - Hb) * rho_s
        a, b, p, _, _ = F.pressure_projection_amg(
            a_star, b_star, dx, dy, dt, rho_local, velocity_bc=C.free_slip_box_bc, p_prev=p,
            eigenvalues=eig, bc_type='neumann')
        cxa, _ = C.disc_centroid(phi_a, X, Y)
        cxb, _ = C.disc_centroid(phi_b, X, Y)
        t += dt
        rec.append((t, dt, cxa, cxb, cxb - cxa, Jmin.min()))
    out.update(drv_N=N, drv_centres=np.array([xa0, xb0]), drv_V0=V0, drv_rec=np.array(rec),
               drv_a=a, drv_b=b, drv_p=p, drv_X1a=X1a, drv_X2a=X2a, drv_X1b=X1b, drv_X2b=X2b,
               drv_phi_a=phi_a, drv_phi_b=phi_b)


if __name__ == "__main__":
    t0 = time.time()
    out = dict(shapes=np.array(SHAPES), R=R, k_rep=K_REP, dt=DT,
               params=np.array([MU_S, KAPPA, ETA_S, RHO_S, RHO_F, MU_F]))
    for ny, nx in SHAPES:
        gen_shape(ny, nx, out)
    gen_surface_tension(out)
    gen_driver(out)
    save("two_solid", **out)
    print(f"done in {time.time() - t0:.0f}s")
