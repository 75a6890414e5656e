"""The unfused composition "stress planes -> face forces" that the fused kernels
(rmt_mac_total_force, rmt_mac_solid_force) are held to, bit for bit: the NumPy references, the
GPU tests and the bench tools of both lid-cavity disc loops share this one statement of it."""
import numpy as np


def faces_of_stress(O, Sxx, Sxy, Syy, dx, dy):
    """mac_reinit_test.py:82-85 / mac_soft_disc_lid.py:107-110 on the operators of O (the oracle,
    the reference's functions module, or pyrmt_amd.functions on device tensors): the central
    divergence of the stress at the cells, averaged to the interior faces; (fu (Ny, Nx+1),
    fv (Ny+1, Nx)) of the planes' array type, wall faces 0."""
    divx = O.grad_central_x_2nd(Sxx, dx) + O.grad_central_y_2nd(Sxy, dy)
    divy = O.grad_central_x_2nd(Sxy, dx) + O.grad_central_y_2nd(Syy, dy)
    ny, nx = Sxx.shape
    zeros = Sxx.new_zeros if hasattr(Sxx, "new_zeros") else np.zeros
    fu = zeros((ny, nx + 1)); fu[:, 1:-1] = 0.5 * (divx[:, 1:] + divx[:, :-1])
    fv = zeros((ny + 1, nx)); fv[1:-1, :] = 0.5 * (divy[1:, :] + divy[:-1, :])
    return fu, fv
