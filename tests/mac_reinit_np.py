"""Inputs of the reinitialisation operator tests, shared by the fixture generator
(tests/golden/gen_golden_mac_reinit.py) and the tests: built from +, * and sqrt on index grids
alone (correctly rounded everywhere), so both sides hold the same bits without storing them."""
import numpy as np

SHAPES = ((9, 9), (33, 70), (65, 64), (40, 130))
MU_S, ADV_DT = 0.3, 0.01


def key(shape):
    return f"{shape[0]}x{shape[1]}"


def op_inputs(shape):
    """A (ny, nx) cell grid on [0, 1] x [0, 1.25] (dx != dy): smooth maps masked to a disc (the
    detG clamp fires outside it), a stored deformation Fs away from the identity, eight planes to
    advect (negative values, and one NaN and one inf in the fluid: q * 0.0 keeps -0.0 and NaN)
    and a swirl that carries a foot up to four cells."""
    ny, nx = shape
    dx, dy = 1.0 / nx, 1.25 / ny
    Xc, Yc = np.meshgrid((np.arange(nx) + 0.5) * dx, (np.arange(ny) + 0.5) * dy)
    Xg, Yg = np.meshgrid(np.arange(nx) * dx, np.arange(ny) * dy)
    phi = np.sqrt((Xc - 0.3) ** 2 + (Yc - 0.35) ** 2) - 0.15
    # (the maps' disc ends 3 cells outside phi = 0: the stencils of the band |phi| <= w_t stay
    # on smooth data, so b is O(1) wherever H is a sine and the bar on S can hold)
    m = (phi <= 3.0 * max(dx, dy)).astype(float)
    X1 = (Xc + 0.0625 * Yc * Yc - 0.03125 * Xc * Yc) * m
    X2 = (Yc + 0.09375 * Xc * Xc + 0.0625 * Xc * Yc) * m
    Fs = [1.0 + 0.125 * Xc * Yc, 0.25 * Xc - 0.125 * Yc, 0.0625 * Yc * Yc, 1.0 - 0.125 * Xc]
    a = -4.0 * (Yc - 0.35)
    b = 4.0 * (Xc - 0.3)
    q = [X1, X2] + Fs + [0.5 - Xc * Yc, (Xc - 0.25) * (Yc - 1.0)]
    q = [p.copy() for p in q]
    q[3][0, 0] = np.nan
    q[6][ny - 1, 1] = np.inf
    return dict(dx=dx, dy=dy, w_t=2.0 * dx, Xg=Xg, Yg=Yg, phi=phi, X1=X1, X2=X2, Fs=Fs, a=a, b=b,
                q=q)
