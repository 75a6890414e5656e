"""NumPy restatements of the two free-slip MAC operators, written for the tests (the fixtures
of tests/golden/mac_freeslip_ops*.npz hold the reference's results at N = 4, 5, 33, 64; these
restatements, checked bit for bit against them, serve as the expected values at larger N).

Every expression keeps the operand order of the formulas it restates, so IEEE arithmetic
gives the same bits.
"""
import numpy as np


def momentum_predictor_freeslip(u, v, nu, dx, dy, dt, fu=None, fv=None, rho=1.0):
    """u (N, N+1), v (N+1, N): forward Euler of central advection + diffusion with mirrored
    tangential ghosts; wall-normal faces of the result are 0."""
    up = np.concatenate([u[:1], u, u[-1:]], axis=0)        # rows -1 and N mirror rows 0, N-1
    vp = np.concatenate([v[:, :1], v, v[:, -1:]], axis=1)  # columns likewise

    uc = u[:, 1:-1]
    dudx = (u[:, 2:] - u[:, :-2]) / (2 * dx)
    dudy = (up[2:, 1:-1] - up[:-2, 1:-1]) / (2 * dy)
    lapu = ((u[:, 2:] - 2 * uc + u[:, :-2]) / dx**2
            + (up[2:, 1:-1] - 2 * up[1:-1, 1:-1] + up[:-2, 1:-1]) / dy**2)
    v_u = 0.25 * (v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:])
    ru = -(uc * dudx + v_u * dudy) + nu * lapu
    if fu is not None:
        ru = ru + fu[:, 1:-1] / rho
    us = np.zeros_like(u)
    us[:, 1:-1] = uc + dt * ru

    vc = v[1:-1, :]
    dvdy = (v[2:, :] - v[:-2, :]) / (2 * dy)
    dvdx = (vp[1:-1, 2:] - vp[1:-1, :-2]) / (2 * dx)
    lapv = ((vp[1:-1, 2:] - 2 * vp[1:-1, 1:-1] + vp[1:-1, :-2]) / dx**2
            + (v[2:, :] - 2 * vc + v[:-2, :]) / dy**2)
    u_v = 0.25 * (u[:-1, :-1] + u[:-1, 1:] + u[1:, :-1] + u[1:, 1:])
    rv = -(u_v * dvdx + vc * dvdy) + nu * lapv
    if fv is not None:
        rv = rv + fv[1:-1, :] / rho
    vs = np.zeros_like(v)
    vs[1:-1, :] = vc + dt * rv
    return us, vs


def interfacial_force_faces(kappa, H, gamma, dx, dy):
    """-gamma * (kappa averaged to the face) * (compact face difference of H) / h on the
    interior faces, 0 on the wall faces."""
    N = H.shape[0]
    fu = np.zeros((N, N + 1))
    fv = np.zeros((N + 1, N))
    fu[:, 1:-1] = -gamma * (0.5 * (kappa[:, 1:] + kappa[:, :-1])) * (H[:, 1:] - H[:, :-1]) / dx
    fv[1:-1, :] = -gamma * (0.5 * (kappa[1:, :] + kappa[:-1, :])) * (H[1:, :] - H[:-1, :]) / dy
    return fu, fv


def ops_fixture(golden, N):
    """The operator fixture of one N as a dict of its arrays and the shared scalars."""
    if N == 64:
        g = golden("mac_freeslip_ops64")
        d = {k: g[k] for k in g.files}
    else:
        g = golden("mac_freeslip_ops")
        d = {k[len(f"n{N}_"):]: g[k] for k in g.files if k.startswith(f"n{N}_")}
        d.update({k: g[k] for k in ("nu", "dt", "rho", "gamma")})
    return {k: (float(a) if a.ndim == 0 else a) for k, a in d.items()}
