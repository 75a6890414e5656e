"""Staggered (MAC) operators of pyRMT/mac.py and the config-5 loop body on MI355X.

Same names, arguments and return values as the reference module (mac.py:22-139,
196-232, 729-749); the arrays go through librmt's HIP kernels (include/rmt.h, rmt_mac_*).
Layout as the reference: p / phi (Ny, Nx) cell centres, u (Ny, Nx+1) x-faces,
v (Ny+1, Nx) y-faces (square grids: Nx == Ny, checked by _lid_n; solve_poisson_neumann alone
takes Ny != Nx).  ``MacMultiDisc`` is the device-resident loop body of
benchmarks/mac_multi_disc_lid.py:36-98 (K soft discs with pair contact).
The periodic tier (mac.py:445-540, 587-650; rmt_mac_per_*) keeps u, v and p all (Ny, Nx);
``MacTaylorGreen`` / ``taylor_green_run_one`` are benchmarks/mac_taylor_green_convergence.py,
its semi-Lagrangian integrator behind ``semilag=True``.
The free-slip box (mac.py:179-193, 656-689): ``momentum_predictor_freeslip``,
``interfacial_force_faces``, and the same fused loop with free-slip walls behind
``MacMultiDisc(walls="freeslip")``: ``MacDiscTaylorGreen`` / ``disc_in_tg_run_one``
(benchmarks/mac_disc_in_tg_convergence.py) and ``MacTwoDiscContact``
(benchmarks/mac_two_disc_contact.py).
Reference-map reinitialisation with stored deformation (benchmarks/mac_reinit_test.py,
mac_reinit.hip): ``total_stress``, ``total_force``, ``epoch_distortion`` and the loop
``MacReinitDisc`` / ``mac_reinit_run``, composed from operators on device tensors.
The soft disc under the integrator ladder (benchmarks/mac_soft_disc_lid.py, mac.py:43-78,
698-721, mac_soft.hip): ``resolve_integrator``, ``solid_force``, ``midpoint_centres``,
``soft_diag``, ``advect_xi_conservative`` and the loop ``MacSoftDisc`` / ``mac_soft_disc_run``.
Both loops stand on ``_LidDisc`` (the disc, the set-up, the projection, the state).
The viscoelastic blob in the four-roll mill (benchmarks/mac_viscoelastic_extension.py,
mac.py:560-584, mac_ve.hip): ``ve_centre_kinematics``, ``ve_face_force``,
``momentum_predictor_periodic_imex_elastic``, ``ve_lock``, ``ve_record`` and the loop
``MacViscoelasticExtension`` / ``mac_ve_extension_run`` / ``compare_integrators``.
"""
import ctypes
import math

import numpy as np

from . import _lib as L
from .functions import _IO, _p, _plane_ptrs, ctx_for, ctx_with, extrapolate_reference_map
from .simulation import _wrap_device


def mac_grid(Nx, Ny, Lx=1.0, Ly=1.0):
    """mac.py:22-23."""
    return Lx / Nx, Ly / Ny


def poisson_eigs_neumann(Nx, Ny, dx, dy):
    """mac.py:104-115 (setup, host): DCT-II symbol, (0,0) pinned to 1."""
    lx = -2.0 * (1.0 - np.cos(np.pi * np.arange(Nx) / Nx)) / dx ** 2
    ly = -2.0 * (1.0 - np.cos(np.pi * np.arange(Ny) / Ny)) / dy ** 2
    eig = (lx[np.newaxis, :] + ly[:, np.newaxis]).copy()
    eig[0, 0] = 1.0
    return eig


def _axis_eigs(eig):
    """Per-axis eigenvalues of a separable eig table (row 0 and column 0; the reference's
    lam[0] is -0.0, so eig[0, k] == lam_x[k] exactly).  Raises if eig is not separable."""
    eig = np.asarray(eig, dtype=np.float64)
    lx = eig[0, :].copy(); ly = eig[:, 0].copy()
    lx[0] = ly[0] = -0.0
    chk = lx[np.newaxis, :] + ly[:, np.newaxis]
    chk[0, 0] = eig[0, 0]
    if not np.array_equal(chk, eig):
        raise NotImplementedError("eig is not a separable per-axis symbol (DCT-II solve)")
    return np.ascontiguousarray(lx), np.ascontiguousarray(ly)


def _ctx(N):
    return ctx_for(N, N).bind()


def _lid_n(what, u=None, v=None, fu=None, fv=None, **cells):
    """N of the square grid the lid-tier arrays live on: u, fu (N, N+1) x-faces, v, fv
    (N+1, N) y-faces, every keyword field (N, N) cell centres.  The kernels behind _ctx(N) are
    square-only and index their arrays by N alone, so anything else (Ny != Nx included, which
    the reference accepts) raises NotImplementedError here, before any library call."""
    arrays = [("u", u, 0, 1), ("v", v, 1, 0), ("fu", fu, 0, 1), ("fv", fv, 1, 0)]
    arrays += [(k, a, 0, 0) for k, a in cells.items()]
    shapes = {k: tuple(np.shape(a)) for k, a, _, _ in arrays if a is not None}
    N = None
    for k, a, ey, ex in arrays:
        if a is None:
            continue
        if N is None and len(shapes[k]) == 2:
            N = shapes[k][0] - ey
        if N is None or shapes[k] != (N + ey, N + ex):
            raise NotImplementedError(
                f"{what}: the lid-tier MAC kernels are square-only (u (N, N+1), v (N+1, N), "
                f"cell fields (N, N)); got {shapes}")
    return N


def divergence(u, v, dx, dy):
    """mac.py:81-84."""
    N = _lid_n("divergence", u, v)
    io = _IO(u, v); u = io.dev(u); v = io.dev(v)
    out = io.empty((N, N))
    L.check(L.lib().rmt_mac_divergence(_ctx(N), _p(u), _p(v), dx, dy, _p(out)), "divergence")
    return io.out(out)


def _gradients(what, p, dx, dy):
    N = _lid_n(what, p=p)
    io = _IO(p); p = io.dev(p)
    gu = io.empty((N, N + 1)); gv = io.empty((N + 1, N))
    L.check(L.lib().rmt_mac_gradient_p(_ctx(N), _p(p), dx, dy, _p(gu), _p(gv)), "gradient_p")
    return io, gu, gv


def gradient_p_u(p, dx):
    """mac.py:87-93."""
    io, gu, _ = _gradients("gradient_p_u", p, dx, dx)
    return io.out(gu)


def gradient_p_v(p, dy):
    """mac.py:96-101."""
    io, _, gv = _gradients("gradient_p_v", p, dy, dy)
    return io.out(gv)


def solve_poisson_neumann(rhs, eig):
    """mac.py:118-123 (orthonormal DCT-II both ways, constant mode zeroed).  (Ny, Nx) may
    differ, as in the reference: the solve binds a context of that shape."""
    shp = tuple(np.shape(rhs))
    if len(shp) != 2 or tuple(np.shape(eig)) != shp:
        raise NotImplementedError(f"solve_poisson_neumann: rhs {shp} and eig "
                                  f"{tuple(np.shape(eig))} must be one (Ny, Nx) shape")
    lx, ly = _axis_eigs(eig)
    io = _IO(rhs); r = io.dev(rhs)
    Ny, Nx = shp
    out = io.empty(shp)
    L.check(L.lib().rmt_mac_solve_poisson_neumann(
        ctx_for(Ny, Nx).bind(), _p(r), 1.0 / Nx, 1.0 / Ny, lx.ctypes.data_as(ctypes.c_void_p),
        ly.ctypes.data_as(ctypes.c_void_p), _p(out)), "solve_poisson_neumann")
    return io.out(out)


def project(u_star, v_star, dx, dy, dt, rho, eig):
    """mac.py:126-139: returns (u, v, phi)."""
    N = _lid_n("project", u_star, v_star, eig=eig)
    lx, ly = _axis_eigs(eig)
    io = _IO(u_star, v_star); us = io.dev(u_star); vs = io.dev(v_star)
    u = io.empty(us.shape); v = io.empty(vs.shape); phi = io.empty((N, N))
    L.check(L.lib().rmt_mac_project(_ctx(N), _p(us), _p(vs), dx, dy, dt, float(rho),
                                    lx.ctypes.data_as(ctypes.c_void_p),
                                    ly.ctypes.data_as(ctypes.c_void_p), _p(u), _p(v), _p(phi)),
            "project")
    return io.out(u), io.out(v), io.out(phi)


def momentum_predictor(u, v, nu, dx, dy, dt, U_lid, fu=None, fv=None, rho=1.0):
    """mac.py:196-232."""
    if (fu is None) != (fv is None):
        raise NotImplementedError("momentum_predictor: give both face forces or neither")
    N = _lid_n("momentum_predictor", u, v, fu, fv)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    fud, fvd = io.dev(fu), io.dev(fv)
    us = io.empty(ud.shape); vs = io.empty(vd.shape)
    L.check(L.lib().rmt_mac_momentum_predictor(_ctx(N), _p(ud), _p(vd), nu, dx, dy,
                                               dt, U_lid, _p(fud), _p(fvd), float(rho), _p(us),
                                               _p(vs)), "momentum_predictor")
    return io.out(us), io.out(vs)


# ------------------------------------------------------------------ IMEX tier --------
# mac.py:243-442 through imex.hip: the homogeneous ghost-cell Laplacians,
# CG / DST-preconditioned CG Helmholtz solves and the IMEX lid-cavity predictor.
def _lap_hom(kind, f, dx, dy):
    N = _lid_n("_lap_u_lid_hom", u=f) if kind == 0 else _lid_n("_lap_v_lid_hom", v=f)
    io = _IO(f); fd = io.dev(f)
    out = io.empty((N, N - 1) if kind == 0 else (N - 1, N))
    L.check(L.lib().rmt_mac_lap_lid_hom(_ctx(N), kind, _p(fd), float(dx), float(dy), _p(out)),
            "_lap_lid_hom")
    return io.out(out)


def _lap_u_lid_hom(u, dx, dy):
    """mac.py:243-250: Laplacian of u (Ny, Nx+1) on the interior faces (Ny, Nx-1)."""
    return _lap_hom(0, u, dx, dy)


def _lap_v_lid_hom(v, dx, dy):
    """mac.py:253-260: Laplacian of v (Ny+1, Nx) on the interior faces (Ny-1, Nx)."""
    return _lap_hom(1, v, dx, dy)


def _dst_helmholtz_eigs(shp, dx, dy):
    """mac.py:278-284 (setup, host): DST-II eigenvalues of the Dirichlet Laplacian."""
    Ny, Nx = shp
    lx = -2.0 * (1.0 - np.cos(np.pi * (np.arange(Nx) + 1) / Nx)) / dx ** 2
    ly = -2.0 * (1.0 - np.cos(np.pi * (np.arange(Ny) + 1) / Ny)) / dy ** 2
    return ly[:, None] + lx[None, :]


def _helmholtz_operator(apply_lap_hom, embed, shp):
    """The reference hands the operator over as callables (mac.py:351, 366 and its tests:
    ``lambda w: _lap_u_lid_hom(w, dx, dy)``, ``np.pad`` embeddings).  Identify the face kind
    and (dx, dy) from the lambda's closure and verify both on a probe (the embedding pads
    the kind's wall axis with zeros, the operator equals this module's kernel bit for bit);
    anything else raises NotImplementedError -- there is no host fallback."""
    code = getattr(apply_lap_hom, "__code__", None)
    names = code.co_names if code is not None else ()
    kind = 0 if "_lap_u_lid_hom" in names else 1 if "_lap_v_lid_hom" in names else None
    cells = {}
    if code is not None and apply_lap_hom.__closure__:
        cells = {k: c.cell_contents for k, c in zip(code.co_freevars, apply_lap_hom.__closure__)}
    dx, dy = cells.get("dx"), cells.get("dy")
    Ny, Nx = shp
    if kind is None or dx is None or dy is None or (kind == 0 and Nx != Ny - 1) or \
            (kind == 1 and Ny != Nx - 1):
        raise NotImplementedError("helmholtz: apply_lap_hom must be the reference's "
                                  "lambda w: _lap_u_lid_hom / _lap_v_lid_hom(w, dx, dy)")
    probe = np.random.default_rng(0).standard_normal(shp)
    e = np.asarray(embed(probe), dtype=np.float64)
    pad = np.pad(probe, ((0, 0), (1, 1)) if kind == 0 else ((1, 1), (0, 0)))
    if not np.array_equal(e, pad):
        raise NotImplementedError("helmholtz: embed must zero-pad the walls as mac.py:350/365")
    host = np.asarray(apply_lap_hom(e), dtype=np.float64)
    if not np.array_equal(host, _lap_hom(kind, e, dx, dy)):
        raise NotImplementedError("helmholtz: apply_lap_hom is not the homogeneous lid Laplacian")
    return kind, float(dx), float(dy)


def _solve_helmholtz(rhs_int, kind, coef, dx, dy, rtol, maxiter, precond):
    io = _IO(rhs_int); b = io.dev(rhs_int)
    N = b.shape[0] if kind == 0 else b.shape[1]
    if tuple(b.shape) != ((N, N - 1) if kind == 0 else (N - 1, N)):
        raise NotImplementedError(f"helmholtz: the interior faces of a square grid, (N, N-1) "
                                  f"for u or (N-1, N) for v; got {tuple(b.shape)}")
    x = io.empty(b.shape)
    it = ctypes.c_int(0)
    L.check(L.lib().rmt_mac_helmholtz(_ctx(N), kind, _p(b), float(coef), dx, dy, float(rtol),
                                      int(maxiter), int(precond), _p(x), ctypes.byref(it)),
            "helmholtz")
    return io.out(x), it.value


def _cg_helmholtz(rhs_int, apply_lap_hom, embed, coef, rtol=1e-10, maxiter=500):
    """mac.py:263-275: (I - coef Lap_hom) x = rhs_int by CG (x0 = rhs_int)."""
    kind, dx, dy = _helmholtz_operator(apply_lap_hom, embed, tuple(rhs_int.shape))
    return _solve_helmholtz(rhs_int, kind, coef, dx, dy, rtol, maxiter, 0)[0]


def _pcg_helmholtz(rhs_int, apply_lap_hom, embed, coef, dx, dy, rtol=1e-8, maxiter=500,
                   count=None):
    """mac.py:287-316: DST-II-preconditioned CG; appends the iteration count to `count`."""
    kind, ldx, ldy = _helmholtz_operator(apply_lap_hom, embed, tuple(rhs_int.shape))
    if (ldx, ldy) != (float(dx), float(dy)):
        raise NotImplementedError("_pcg_helmholtz: the preconditioner's (dx, dy) differ from "
                                  "the operator's")
    x, it = _solve_helmholtz(rhs_int, kind, coef, ldx, ldy, rtol, maxiter, 1)
    if count is not None:
        count.append(it)
    return x


def _predictor_lid_imex(u, v, nu, dx, dy, dt, U_lid, fu, fv, rho, rtol, cs2):
    """momentum_predictor_lid_imex with the two PCG iteration counts: (u*, v*, (it_u, it_v))."""
    N = _lid_n("momentum_predictor_lid_imex", u, v, fu, fv)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    fud, fvd = io.dev(fu), io.dev(fv)
    us = io.empty(ud.shape); vs = io.empty(vd.shape)
    it = (ctypes.c_int * 2)()
    L.check(L.lib().rmt_mac_momentum_predictor_lid_imex(
        _ctx(N), _p(ud), _p(vd), float(nu), float(dx), float(dy), float(dt),
        float(U_lid), _p(fud), _p(fvd), float(rho), float(rtol), float(cs2), _p(us), _p(vs),
        ctypes.cast(it, ctypes.c_void_p)), "momentum_predictor_lid_imex")
    return io.out(us), io.out(vs), (it[0], it[1])


def momentum_predictor_lid_imex(u, v, nu, dx, dy, dt, U_lid, fu=None, fv=None, rho=1.0,
                                rtol=1e-8, cs2=0.0):
    """mac.py:319-369: explicit central advection + face forces, implicit (backward-Euler)
    viscosity (+ the trapezoidal elastic term, cs2 > 0) by DST-preconditioned CG."""
    return _predictor_lid_imex(u, v, nu, dx, dy, dt, U_lid, fu, fv, rho, rtol, cs2)[:2]


def _predictor_lid_semilag(u, v, nu, dx, dy, dt, U_lid, fu, fv, rho, cs2, rtol, cfl_switch):
    """momentum_predictor_lid_semilag with the PCG counts and the branch taken:
    (u*, v*, (it_u, it_v), semi-Lagrangian)."""
    N = _lid_n("momentum_predictor_lid_semilag", u, v, fu, fv)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    cfl = dt * max(float(ud.abs().max()) / dx, float(vd.abs().max()) / dy)
    if cfl <= cfl_switch:
        return _predictor_lid_imex(u, v, nu, dx, dy, dt, U_lid, fu, fv, rho, rtol, cs2) + (False,)
    fud, fvd = io.dev(fu), io.dev(fv)
    us = io.empty(ud.shape); vs = io.empty(vd.shape)
    it = (ctypes.c_int * 2)()
    L.check(L.lib().rmt_mac_momentum_predictor_lid_semilag(
        _ctx(N), _p(ud), _p(vd), float(nu), float(dx), float(dy), float(dt),
        float(U_lid), _p(fud), _p(fvd), float(rho), float(cs2), float(rtol), _p(us), _p(vs),
        ctypes.cast(it, ctypes.c_void_p)), "momentum_predictor_lid_semilag")
    return io.out(us), io.out(vs), (it[0], it[1]), True


def momentum_predictor_lid_semilag(u, v, nu, dx, dy, dt, U_lid, fu=None, fv=None, rho=1.0,
                                   cs2=0.0, rtol=1e-8, cfl_switch=0.9):
    """mac.py:381-442: adaptive predictor -- momentum_predictor_lid_imex at an advective
    CFL <= cfl_switch (mac.py:387-390), else the semi-Lagrangian midpoint backtrace through
    cubic-spline interpolation (map_coordinates order 3, 'nearest') and the same PCG
    viscosity solve."""
    return _predictor_lid_semilag(u, v, nu, dx, dy, dt, U_lid, fu, fv, rho, cs2, rtol,
                                  cfl_switch)[:2]


def momentum_predictor_freeslip(u, v, nu, dx, dy, dt, fu=None, fv=None, rho=1.0):
    """mac.py:656-689: the explicit predictor on the free-slip box (mirrored tangential
    ghosts, wall-normal faces zeroed)."""
    if (fu is None) != (fv is None):
        raise NotImplementedError("momentum_predictor_freeslip: give both face forces or neither")
    N = _lid_n("momentum_predictor_freeslip", u, v, fu, fv)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    fud, fvd = io.dev(fu), io.dev(fv)
    us = io.empty(ud.shape); vs = io.empty(vd.shape)
    # (N = 4, below the stencil contexts' 5: a context of its own, as the periodic tier's)
    L.check(L.lib().rmt_mac_momentum_predictor_freeslip(
        _pctx((N, N), True), _p(ud), _p(vd), nu, dx, dy, dt, _p(fud), _p(fvd), float(rho), _p(us), _p(vs)),
        "momentum_predictor_freeslip")
    return io.out(us), io.out(vs)


def interfacial_force_faces(kappa, H, gamma, dx, dy):
    """mac.py:179-193: the balanced continuum-surface force on the faces, (fu, fv)."""
    N = _lid_n("interfacial_force_faces", kappa=kappa, H=H)
    io = _IO(kappa, H); kd = io.dev(kappa); Hd = io.dev(H)
    fu = io.empty((N, N + 1)); fv = io.empty((N + 1, N))
    L.check(L.lib().rmt_mac_interfacial_force_faces(_pctx((N, N), True), _p(kd), _p(Hd), gamma, dx, dy,
                                                    _p(fu), _p(fv)), "interfacial_force_faces")
    return io.out(fu), io.out(fv)


def contact_stress(phi_a, phi_b, eta, Gsum, eps, dx, dy):
    """mac.py:729-749: (txx, txy, tyy)."""
    N = _lid_n("contact_stress", phi_a=phi_a, phi_b=phi_b)
    io = _IO(phi_a, phi_b); a = io.dev(phi_a); b = io.dev(phi_b)
    out = [io.empty(a.shape) for _ in range(3)]
    L.check(L.lib().rmt_mac_contact_stress(_ctx(N), _p(a), _p(b), eta, Gsum, eps, dx,
                                           dy, *map(_p, out)), "contact_stress")
    return tuple(io.out(t) for t in out)


# ------------------------------------------------------------------ periodic tier ----
# mac.py:445-540, 587-650 through macper.hip and macper_sl.hip: u (x-faces), v (y-faces) and p
# (centres) are all (Ny, Nx) planes and every index wraps.  The stencil operators are
# bit-exact; the solves go through rocFFT on the half-spectrum (the reference: numpy.fft) and
# the grid-wrap cubic splines of the semi-Lagrangian predictor through a windowed prefilter
# (the reference: scipy.ndimage), both equal to rounding.
# momentum_predictor_periodic_imex_elastic stands with its driver at the end of this module.
_small_ctxs = {}


def _pctx(shape, small=False):
    """small: the spline operators and the two predictors they switch between take extents
    from 2; below the stencil contexts' 5 they get a context of their own (no collocated
    stencil is ever called on it)."""
    ny, nx = int(shape[0]), int(shape[1])
    if small and min(ny, nx) < 5:
        from .functions import _Ctx, _torch
        key = (ny, nx, _torch().cuda.current_device())
        if key not in _small_ctxs:
            _small_ctxs[key] = _Ctx(ny, nx, key[2], stencils=False)
        return _small_ctxs[key].bind()
    return ctx_for(ny, nx).bind()


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def divergence_per(u, v, dx, dy):
    """mac.py:449-450."""
    io = _IO(u, v); u = io.dev(u); v = io.dev(v)
    out = io.empty(u.shape)
    L.check(L.lib().rmt_mac_per_divergence(_pctx(u.shape), _p(u), _p(v), float(dx), float(dy),
                                           _p(out)), "divergence_per")
    return io.out(out)


def grad_p_u_per(p, dx):
    """mac.py:453-454."""
    io = _IO(p); p = io.dev(p)
    g = io.empty(p.shape)
    L.check(L.lib().rmt_mac_per_gradient_p(_pctx(p.shape), _p(p), float(dx), float(dx), _p(g),
                                           None), "grad_p_u_per")
    return io.out(g)


def grad_p_v_per(p, dy):
    """mac.py:457-458."""
    io = _IO(p); p = io.dev(p)
    g = io.empty(p.shape)
    L.check(L.lib().rmt_mac_per_gradient_p(_pctx(p.shape), _p(p), float(dy), float(dy), None,
                                           _p(g)), "grad_p_v_per")
    return io.out(g)


def _per_axis(n, h):
    return -4.0 * np.sin(np.pi * np.arange(n) / n) ** 2 / h**2


def poisson_eigs_periodic(Nx, Ny, dx, dy):
    """mac.py:461-467 (setup, host): FFT symbol of the roll stencil, (0,0) pinned to 1."""
    eig = (_per_axis(Nx, dx)[np.newaxis, :] + _per_axis(Ny, dy)[:, np.newaxis]).copy()
    eig[0, 0] = 1.0
    return eig


def lap_eigs_periodic(Nx, Ny, dx, dy):
    """mac.py:501-509 (setup, host): the same symbol, not pinned ((0,0) is -0.0)."""
    return _per_axis(Nx, dx)[np.newaxis, :] + _per_axis(Ny, dy)[:, np.newaxis]


def _axis_eigs_per(eig, pinned):
    """Per-axis vectors (lx, ly) of a periodic symbol table: row 0 and column 0 (the
    reference's lam[0] is -0.0, so eig[0, k] == lx[k] exactly).  pinned: the Poisson table,
    whose (0,0) entry is the pin (1.0) and is ignored, as the solve zeroes that mode; else the
    Laplacian table, checked at (0,0) too.  The table must equal lx[None, :] + ly[:, None] bit
    for bit, and each axis must be even in the wavenumber to rounding (the solve works on the
    half-spectrum); anything else raises NotImplementedError -- there is no host fallback."""
    if hasattr(eig, "cpu"):
        eig = eig.cpu().numpy()
    eig = np.ascontiguousarray(eig, dtype=np.float64)
    if eig.ndim != 2 or min(eig.shape) < 2:
        raise NotImplementedError("periodic symbol: a (Ny, Nx) table with Ny, Nx >= 2")
    lx = eig[0, :].copy(); ly = eig[:, 0].copy()
    ly[0] = -0.0
    if pinned:
        lx[0] = -0.0
    chk = np.ascontiguousarray(lx[np.newaxis, :] + ly[:, np.newaxis])
    if pinned:
        chk[0, 0] = eig[0, 0]
    if not np.array_equal(chk.view(np.int64), eig.view(np.int64)):
        raise NotImplementedError("eig is not a separable per-axis symbol (periodic FFT solve)")
    for lam in (lx, ly):
        if np.abs(lam[1:] - lam[1:][::-1]).max() > 1e-12 * np.abs(lam).max():
            raise NotImplementedError("eig is not even in the wavenumber (half-spectrum solve)")
    return lx, ly


def _solve_per(rhs, lx, ly, mode, coef, what):
    io = _IO(rhs); r = io.dev(rhs)
    if tuple(r.shape) != (ly.size, lx.size):
        raise ValueError(f"{what}: rhs {tuple(r.shape)} against a {(ly.size, lx.size)} symbol")
    out = io.empty(r.shape)
    L.check(L.lib().rmt_mac_per_solve(_pctx(r.shape), _p(r), mode, float(coef), _hp(lx), _hp(ly),
                                      _p(out)), what)
    return io.out(out)


def solve_poisson_periodic(rhs, eig):
    """mac.py:470-473."""
    lx, ly = _axis_eigs_per(eig, True)
    return _solve_per(rhs, lx, ly, 0, 0.0, "solve_poisson_periodic")


def solve_helmholtz_periodic(rhs, lap_eig, coef):
    """mac.py:512-518: (I - coef Lap) x = rhs."""
    lx, ly = _axis_eigs_per(lap_eig, False)
    return _solve_per(rhs, lx, ly, 1, coef, "solve_helmholtz_periodic")


def project_per(u_star, v_star, dx, dy, dt, rho, eig):
    """mac.py:476-480: returns (u, v, phi)."""
    lx, ly = _axis_eigs_per(eig, True)
    io = _IO(u_star, v_star); us = io.dev(u_star); vs = io.dev(v_star)
    if tuple(us.shape) != (ly.size, lx.size):
        raise ValueError("project_per: the fields and eig differ in shape")
    u = io.empty(us.shape); v = io.empty(us.shape); phi = io.empty(us.shape)
    L.check(L.lib().rmt_mac_per_project(_pctx(us.shape), _p(us), _p(vs), float(dx), float(dy),
                                        float(rho / dt), float(dt / rho), _hp(lx), _hp(ly),
                                        _p(u), _p(v), _p(phi)), "project_per")
    return io.out(u), io.out(v), io.out(phi)


def momentum_predictor_periodic(u, v, nu, dx, dy, dt):
    """mac.py:636-650: forward Euler, central advection + diffusion.  dx**2, 2*dx are formed
    here, on the caller's scalar types, as the reference forms them."""
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    us = io.empty(ud.shape); vs = io.empty(ud.shape)
    L.check(L.lib().rmt_mac_per_predictor(_pctx(ud.shape), _p(ud), _p(vd), float(nu),
                                          float(dx**2), float(dy**2), float(2 * dx),
                                          float(2 * dy), float(dt), _p(us), _p(vs)),
            "momentum_predictor_periodic")
    return io.out(us), io.out(vs)


def momentum_predictor_periodic_imex(u, v, nu, dx, dy, dt, lap_eig):
    """mac.py:521-540: explicit central advection, backward-Euler viscosity by two FFT
    Helmholtz solves."""
    lx, ly = _axis_eigs_per(lap_eig, False)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    if tuple(ud.shape) != (ly.size, lx.size):
        raise ValueError("momentum_predictor_periodic_imex: the fields and lap_eig differ in shape")
    us = io.empty(ud.shape); vs = io.empty(ud.shape)
    L.check(L.lib().rmt_mac_per_predictor_imex(_pctx(ud.shape, True), _p(ud), _p(vd),
                                               float(2 * dx), float(2 * dy), float(dt),
                                               float(dt * nu), _hp(lx), _hp(ly), _p(us), _p(vs)),
            "momentum_predictor_periodic_imex")
    return io.out(us), io.out(vs)


def _plane2(what, **arrays):
    """The common (Ny, Nx) of 2-D planes with Ny, Nx >= 2 (host check, before any library
    call)."""
    shapes = {k: tuple(np.shape(a)) for k, a in arrays.items()}
    first = next(iter(shapes.values()))
    if len(first) != 2 or min(first) < 2 or any(sh != first for sh in shapes.values()):
        raise ValueError(f"{what}: (Ny, Nx) planes of one shape with Ny, Nx >= 2; got {shapes}")
    return first


def spline_filter_per(f):
    """scipy.ndimage.spline_filter(f, order=3, mode='grid-wrap'): the cubic B-spline
    coefficient plane that _interp_per evaluates (the prefilter inside mac.py:597-598)."""
    _plane2("spline_filter_per", f=f)
    io = _IO(f); fd = io.dev(f)
    out = io.empty(fd.shape)
    L.check(L.lib().rmt_mac_per_spline_prefilter(_pctx(fd.shape, True), _p(fd), _p(out)),
            "spline_filter_per")
    return io.out(out)


def _interp_per(f, iq, jq):
    """mac.py:593-598: periodic cubic interpolation of f[j, i] at the fractional indices
    (iq, jq), arrays of one shape; the result has that shape."""
    _plane2("_interp_per", f=f)
    if tuple(np.shape(iq)) != tuple(np.shape(jq)):
        raise ValueError(f"_interp_per: iq {tuple(np.shape(iq))} against jq "
                         f"{tuple(np.shape(jq))}")
    io = _IO(f, iq, jq); fd = io.dev(f)
    qi = io.dev(iq).contiguous(); qj = io.dev(jq).contiguous()
    if qi.numel() >= 2**31:
        raise ValueError("_interp_per: fewer than 2**31 points a call")
    out = io.empty(qi.shape)
    L.check(L.lib().rmt_mac_per_interp(_pctx(fd.shape, True), _p(fd), _p(qi), _p(qj),
                                       int(qi.numel()), _p(out)), "_interp_per")
    return io.out(out)


def _sl_advect_per(f, uf, vf, ox, oy, dx, dy, dt):
    """mac.py:601-614: RK2 semi-Lagrangian advection of f (at offset (ox, oy) in cells) by
    the staggered velocities uf, vf."""
    _plane2("_sl_advect_per", f=f, uf=uf, vf=vf)
    io = _IO(f, uf, vf); fd = io.dev(f); ud = io.dev(uf); vd = io.dev(vf)
    out = io.empty(fd.shape)
    L.check(L.lib().rmt_mac_per_sl_advect(_pctx(fd.shape, True), _p(fd), _p(ud), _p(vd), float(ox),
                                          float(oy), float(dx), float(dy), float(dt), _p(out)),
            "_sl_advect_per")
    return io.out(out)


def _predictor_semilag(u, v, nu, dx, dy, dt, lap_eig, cfl_switch):
    """momentum_predictor_periodic_semilag and the branch it took: (u*, v*, took_sl)."""
    shape = _plane2("momentum_predictor_periodic_semilag", u=u, v=v)
    if tuple(np.shape(lap_eig)) != shape:
        raise ValueError("momentum_predictor_periodic_semilag: the fields and lap_eig differ in "
                         "shape")
    lx, ly = _axis_eigs_per(lap_eig, False)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    us = io.empty(ud.shape); vs = io.empty(ud.shape)
    took = ctypes.c_int(0)
    L.check(L.lib().rmt_mac_per_predictor_semilag(
        _pctx(ud.shape, True), _p(ud), _p(vd), float(2 * dx), float(2 * dy), float(dx), float(dy),
        float(dt), float(dt * nu), float(cfl_switch), _hp(lx), _hp(ly), _p(us), _p(vs),
        ctypes.byref(took)), "momentum_predictor_periodic_semilag")
    return io.out(us), io.out(vs), bool(took.value)


def momentum_predictor_periodic_semilag(u, v, nu, dx, dy, dt, lap_eig, cfl_switch=0.9):
    """mac.py:617-633: momentum_predictor_periodic_imex while the advective CFL (formed on the
    device) is at most cfl_switch, else semi-Lagrangian advection; backward-Euler viscosity
    either way."""
    return _predictor_semilag(u, v, nu, dx, dy, dt, lap_eig, cfl_switch)[:2]


_PER_INTEGRATORS = {"explicit": "explicit", "exp": "explicit", "forward-euler": "explicit",
                    "imex": "imex", "imex-visc": "imex", "implicit-viscosity": "imex",
                    "semi-implicit": "imex"}
_ELASTIC_INTEGRATORS = ("imex-elastic", "elastic", "implicit-elastic")


def _resolve_periodic_integrator(integrator=None, implicit_visc=False):
    """The integrator of mac_taylor_green_convergence.py:47-52 (resolve_integrator with
    supports_elastic=False, mac.py:46-78): "explicit" or "imex" from None + the legacy
    boolean or one of the reference's aliases."""
    if integrator is None:
        return "imex" if implicit_visc else "explicit"
    key = str(integrator).lower().replace("_", "-").strip()
    if key == "imex-sl":
        raise NotImplementedError("integrator 'imex-sl' (semi-Lagrangian periodic predictor, "
                                  "mac.py:587-633) is not built as an integrator name; pass "
                                  "semilag=True (with integrator None or 'imex')")
    if key in _ELASTIC_INTEGRATORS:
        raise ValueError("integrator='imex-elastic' is not available for this driver "
                         "(no solid-stress force path); use 'explicit' or 'imex'")
    if key not in _PER_INTEGRATORS:
        raise ValueError(f"unknown integrator {integrator!r}; choose from "
                         "('explicit', 'imex', 'imex-elastic')")
    return _PER_INTEGRATORS[key]


def _resolve_periodic_semilag(integrator=None, semilag=False):
    """The integrator behind the semilag keyword: semilag=True is the reference's "imex-sl"
    (mac_taylor_green_convergence.py:47-49, IMEX with the semi-Lagrangian predictor), so the
    integrator must be None or resolve to "imex"; semilag=False: _resolve_periodic_integrator."""
    if not semilag:
        return _resolve_periodic_integrator(integrator)
    name = "imex" if integrator is None else _resolve_periodic_integrator(integrator)
    if name != "imex":
        raise ValueError(f"semilag=True is the IMEX step with semi-Lagrangian advection; "
                         f"integrator {integrator!r} resolves to {name!r}")
    return name


class MacPeriodic:
    """The loop body of mac_taylor_green_convergence.py:59-66 on the GPU (rmt_mac_per_steps):
    u, v (and the last projection's phi, p) stay in HBM, a call of step(n) runs n predictor +
    projection steps at the fixed dt with no host round trip.  options: implementation
    switches of a context of its own (macp_fused).  semilag=True: the reference's "imex-sl"
    (rmt_mac_per_steps_sl), every step's branch decided on the device against cfl_switch;
    sl_steps counts the steps that took the semi-Lagrangian branch."""

    def __init__(self, ny, nx, dx, dy, nu, dt, rho=1.0, integrator=None, options=None,
                 semilag=False, cfl_switch=0.9):
        self.integrator = _resolve_periodic_semilag(integrator, semilag)
        self.semilag, self.cfl_switch, self.sl_steps = bool(semilag), float(cfl_switch), 0
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pyrmt_amd needs a visible MI355X")
        self.torch, self.shape = torch, (int(ny), int(nx))
        self.dx, self.dy, self.nu, self.dt, self.rho = dx, dy, nu, dt, rho
        self.ctx = ctx_with(*self.shape, options)
        self.lx, self.ly = _axis_eigs_per(lap_eigs_periodic(nx, ny, dx, dy), False)
        self.u, self.v, self.p = (torch.zeros(self.shape, dtype=torch.float64, device="cuda")
                                  for _ in range(3))
        self.nsteps = 0

    def set(self, u, v):
        io = _IO(u, v)
        self.u.copy_(io.dev(u)); self.v.copy_(io.dev(v))

    def step(self, nsteps=1):
        dx, dy, dt = self.dx, self.dy, self.dt
        if self.semilag:
            took = ctypes.c_int(0)
            L.check(L.lib().rmt_mac_per_steps_sl(
                self.ctx.bind(), _p(self.u), _p(self.v), float(self.nu), float(dx), float(dy),
                float(dx**2), float(dy**2), float(2 * dx), float(2 * dy), float(dt),
                float(dt * self.nu), float(self.rho / dt), float(dt / self.rho), _hp(self.lx),
                _hp(self.ly), self.cfl_switch, int(nsteps), _p(self.p), ctypes.byref(took)),
                "rmt_mac_per_steps_sl")
            self.sl_steps += took.value
            self.nsteps += int(nsteps)
            return
        L.check(L.lib().rmt_mac_per_steps(
            self.ctx.bind(), _p(self.u), _p(self.v), float(self.nu), float(dx), float(dy),
            float(dx**2), float(dy**2), float(2 * dx), float(2 * dy), float(dt),
            float(dt * self.nu), float(self.rho / dt), float(dt / self.rho), _hp(self.lx),
            _hp(self.ly), int(self.integrator == "imex"), int(nsteps), _p(self.p)),
            "rmt_mac_per_steps")
        self.nsteps += int(nsteps)

    def get(self, name):
        self.torch.cuda.synchronize()
        return getattr(self, name).cpu().numpy()


def _tg_faces(N):
    """mac_taylor_green_convergence.py:24-31: face coordinates on [0, 2 pi]^2."""
    dx = 2 * np.pi / N
    xf = np.arange(N) * dx; xc = (np.arange(N) + 0.5) * dx
    Xu, Yu = np.meshgrid(xf, xc)
    Xv, Yv = np.meshgrid(xc, xf)
    return dx, Xu, Yu, Xv, Yv


def tg_exact(Xu, Yu, Xv, Yv, nu, t):
    """mac_taylor_green_convergence.py:34-36 (host): the decaying Taylor-Green vortex."""
    e = np.exp(-2 * nu * t)
    return -np.cos(Xu) * np.sin(Yu) * e, np.sin(Xv) * np.cos(Yv) * e


class MacTaylorGreen(MacPeriodic):
    """The decaying Taylor-Green vortex on [0, 2 pi]^2 at N x N, rho = 1."""

    def __init__(self, N, nu, dt, integrator=None, options=None, semilag=False,
                 cfl_switch=0.9):
        dx, *self.faces = _tg_faces(N)
        super().__init__(N, N, dx, dx, nu, dt, 1.0, integrator, options, semilag, cfl_switch)
        self.set(*tg_exact(*self.faces, nu, 0.0))

    def exact(self):
        return tg_exact(*self.faces, self.nu, self.nsteps * self.dt)


def taylor_green_run_one(N, nu=0.05, T=0.2, dt=2e-4, implicit_visc=False, integrator=None,
                         semilag=False):
    """mac_taylor_green_convergence.py:39-70 (run_one): integrate to T, return (L2 error of u
    against the exact solution, max|div|).  semilag=True: the reference's integrator="imex-sl"."""
    if semilag:
        sim = MacTaylorGreen(N, nu, dt, integrator, semilag=True)
    else:
        sim = MacTaylorGreen(N, nu, dt, _resolve_periodic_integrator(integrator, implicit_visc))
    sim.step(int(round(T / dt)))
    ue, _ = sim.exact()
    erru = np.sqrt(np.mean((sim.get("u") - ue) ** 2))
    divmax = float(divergence_per(sim.u, sim.v, sim.dx, sim.dx).abs().max())
    return erru, divmax


# ------------------------------------------------------------------ config 5 loop --
def place_discs(n, seed, Rrange=(0.07, 0.12), box=(0.18, 0.82)):
    """mac_multi_disc_lid.py:22-33 (setup, host): non-overlapping random discs (R, cx, cy)."""
    rng = np.random.default_rng(seed)
    discs = []
    for _ in range(2000):
        if len(discs) == n:
            break
        R = rng.uniform(*Rrange)
        cx = rng.uniform(box[0] + R, box[1] - R); cy = rng.uniform(box[0] + R, box[1] - R)
        if all((cx - d[1]) ** 2 + (cy - d[2]) ** 2 > (R + d[0] + 0.03) ** 2 for d in discs):
            discs.append((R, cx, cy))
    return discs


def mac_params(N, specs, U_lid=1.0, mu_s=0.3, mu_f=0.01, rho=1.0, eta=2.0, dt=None):
    """rmt_mac_params and the fixed dt of mac_multi_disc_lid.py:36-60 (dt given: that step in
    the formula's place, which a free-slip box with U_lid = 0 has no use for)."""
    dx, _ = mac_grid(N, N)
    specs = list(specs)
    if not 1 <= len(specs) <= 8:
        raise ValueError("1..8 discs")
    cs = np.sqrt(mu_s / rho)
    if dt is None:
        dt = min(0.3 * dx / U_lid, 0.2 * dx * dx / (mu_f / rho), 0.3 * dx / (cs + 1e-9))
    P = L.rmt_mac_params()
    P.N = N; P.dx = dx; P.n_discs = len(specs)
    for k, (R, cx, cy) in enumerate(specs):
        P.R[k], P.cx[k], P.cy[k] = R, cx, cy
    P.U_lid, P.mu_s, P.mu_f, P.rho, P.eta = U_lid, mu_s, mu_f, rho, eta
    P.layers = 3
    P.dt = float(dt)
    return P, float(dt)


def initial_maps(N, specs):
    """(X1, X2, phi) per disc (mac_multi_disc_lid.py:51-56): xi = x_c * mask, extrapolated."""
    dx, dy = mac_grid(N, N)
    xc = (np.arange(N) + 0.5) * dx
    Xc, Yc = np.meshgrid(xc, xc)
    out = []
    for R, cx, cy in specs:
        phi = np.sqrt((Xc - cx) ** 2 + (Yc - cy) ** 2) - R
        m = (phi <= 0).astype(float)
        X1, X2 = extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, 3)
        out.append((X1, X2, np.sqrt((X1 - cx) ** 2 + (X2 - cy) ** 2) - R))
    return out


class MacMultiDisc:
    """benchmarks/mac_multi_disc_lid.py:36-98 on the GPU (rmt_mac_sim_*): state (u, v, p and
    every disc's X1, X2, phi) stays in HBM; one host sync per step reads the diagnostics."""

    FIELDS = {"u": 0, "v": 1, "p": 2, "X1": 3, "X2": 4, "phi": 5}
    WALLS = {"lid": 0, "freeslip": 1}   # RMT_MAC_WALL_*

    def __init__(self, N=128, n_discs=3, seed=3, U_lid=1.0, mu_s=0.3, mu_f=0.01, rho=1.0,
                 eta=2.0, specs=None, options=None, walls="lid", stop_on_divergence=True,
                 dt=None):
        """walls: "lid" (the cavity, U_lid) or "freeslip" (the box of
        mac_disc_in_tg_convergence.py / mac_two_disc_contact.py; U_lid is not read);
        stop_on_divergence=False: the loop goes on past a record with diverged set, as those
        two drivers do; dt: a fixed step in place of mac_params' formula."""
        if walls not in self.WALLS:
            raise ValueError(f"walls {walls!r}: one of {tuple(self.WALLS)}")
        if dt is not None and not (float(dt) > 0.0 and math.isfinite(float(dt))):
            raise ValueError(f"dt {dt!r}: a positive finite step")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pyrmt_amd needs a visible MI355X")
        self.torch, self.N = torch, N
        dx, dy = mac_grid(N, N)
        self.dx = dx
        self.specs = list(specs) if specs is not None else place_discs(n_discs, seed)
        if not 1 <= len(self.specs) <= 8:
            raise ValueError("1..8 discs")
        P, self.dt = mac_params(N, self.specs, U_lid, mu_s, mu_f, rho, eta, dt)
        self.ctx = ctx_with(N, N, options)
        h = ctypes.c_void_p()
        L.check(L.lib().rmt_mac_sim_create(self.ctx.bind(), ctypes.byref(P), ctypes.byref(h)),
                "rmt_mac_sim_create")
        self.h, self.params = h, P
        self.walls, self.stop_on_divergence = walls, bool(stop_on_divergence)
        if walls != "lid" or not stop_on_divergence:
            self.set_mode(walls, stop_on_divergence)
        self._views = {}
        # the initial maps go up through one pinned staging plane: a DMA copy per map instead of
        # the runtime's pageable staging (≈0.6 MB chunks: ~7,800 copies at N=8192)
        stage = torch.empty((N, N), dtype=torch.float64, pin_memory=True)
        cur = torch.cuda.current_stream()
        for k, maps in enumerate(initial_maps(N, self.specs)):
            for name, a in zip(("X1", "X2", "phi"), maps):
                stage.numpy()[...] = a
                self.field(name, k).copy_(stage, non_blocking=True)
                cur.synchronize()   # (before the staging plane is refilled)

    def __del__(self):
        try:
            L.lib().rmt_mac_sim_destroy(self.h)
        except Exception:
            pass

    def set_mode(self, walls, stop_on_divergence):
        """rmt_mac_sim_set_mode: legal only before the first step."""
        L.check(L.lib().rmt_mac_sim_set_mode(self.h, self.WALLS[walls], int(bool(stop_on_divergence))),
                "rmt_mac_sim_set_mode")
        self.walls, self.stop_on_divergence = walls, bool(stop_on_divergence)

    def field(self, name, disc=0):
        key = (name, disc if name in ("X1", "X2", "phi") else 0)
        if key not in self._views:
            ptr = ctypes.c_void_p()
            L.check(L.lib().rmt_mac_sim_field(self.h, self.FIELDS[name], key[1], ctypes.byref(ptr)))
            N = self.N
            shape = {"u": (N, N + 1), "v": (N + 1, N)}.get(name, (N, N))
            self._views[key] = _wrap_device(self.torch, ptr.value, shape)
        return self._views[key]

    def get(self, name, disc=0):
        self.torch.cuda.synchronize()
        return self.field(name, disc).cpu().numpy()

    def step(self, nsteps=1, t_end=math.inf):
        self.ctx.bind()
        L.check(L.lib().rmt_mac_sim_step(self.h, int(nsteps), float(t_end)), "rmt_mac_sim_step")

    def diagnostics(self):
        n = ctypes.c_int()
        L.check(L.lib().rmt_mac_sim_diagnostics(self.h, None, 0, ctypes.byref(n)))
        buf = (L.rmt_mac_diag * max(n.value, 1))()
        L.check(L.lib().rmt_mac_sim_diagnostics(self.h, buf, n.value, ctypes.byref(n)))
        K = len(self.specs)
        out = {k: np.array([getattr(buf[i], k) for i in range(n.value)])
               for k in ("t", "dt", "minJ", "maxJ", "umax")}
        out["diverged"] = np.array([buf[i].diverged for i in range(n.value)], dtype=np.int32)
        out["cx"] = np.array([[buf[i].cx[k] for k in range(K)] for i in range(n.value)])
        out["cy"] = np.array([[buf[i].cy[k] for k in range(K)] for i in range(n.value)])
        return out


# ------------------------------------------------------------------ free-slip box --
def disc_in_tg_dt(N, mu_s=0.1, mu_f=0.01, U0=0.3, rho=1.0):
    """mac_disc_in_tg_convergence.py:47-49 (setup, host): the driver's fixed step."""
    dx, _ = mac_grid(N, N)
    nu = mu_f / rho; cs = np.sqrt(mu_s / rho)
    return float(min(0.25 * dx / (U0 * np.pi), 0.2 * dx * dx / nu, 0.25 * dx / (cs + 1e-9)))


def two_disc_dt(N, V0=0.3, mu_s=0.2, mu_f=0.02, rho=1.0):
    """mac_two_disc_contact.py:36-45 (setup, host): the driver's fixed step."""
    dx, _ = mac_grid(N, N)
    nu = mu_f / rho; cs = np.sqrt(mu_s / rho)
    return float(min(0.25 * dx / max(V0, 1e-9), 0.2 * dx * dx / nu, 0.25 * dx / (cs + 1e-9)))


class MacDiscTaylorGreen(MacMultiDisc):
    """benchmarks/mac_disc_in_tg_convergence.py:30-82 (run_one, scheme "semilagrangian") on the
    GPU: a neo-Hookean disc in the decaying Taylor-Green vortex psi = U0 sin(pi x) sin(pi y)
    on the free-slip box; the loop runs past a folded map, as the driver does."""

    def __init__(self, N, R=0.15, x0=0.5, y0=0.7, mu_s=0.1, mu_f=0.01, U0=0.3, rho=1.0,
                 options=None):
        super().__init__(N, specs=[(R, x0, y0)], U_lid=0.0, mu_s=mu_s, mu_f=mu_f, rho=rho,
                         eta=0.0, options=options, walls="freeslip", stop_on_divergence=False,
                         dt=disc_in_tg_dt(N, mu_s, mu_f, U0, rho))
        self.mu_s, self.U0 = mu_s, U0
        dx = self.dx
        xc = (np.arange(N) + 0.5) * dx; xf = np.arange(N + 1) * dx
        Xu, Yu = np.meshgrid(xf, xc)
        Xv, Yv = np.meshgrid(xc, xf)
        u = U0 * np.pi * np.sin(np.pi * Xu) * np.cos(np.pi * Yu)       # :40-42
        v = -U0 * np.pi * np.cos(np.pi * Xv) * np.sin(np.pi * Yv)
        u[:, 0] = 0.0; u[:, -1] = 0.0; v[0, :] = 0.0; v[-1, :] = 0.0
        self.field("u").copy_(self.torch.from_numpy(u))
        self.field("v").copy_(self.torch.from_numpy(v))
        self.torch.cuda.synchronize()


def disc_in_tg_run_one(N, t_end, R=0.15, x0=0.5, y0=0.7, mu_s=0.1, mu_f=0.01, U0=0.3, rho=1.0,
                       scheme="semilagrangian", w_cut_fac=4.0, isochoric=False,
                       normalize_phi=False):
    """mac_disc_in_tg_convergence.py:30-91 (run_one): the dict N, dx, xc, speed, p, KE,
    Estrain, divmax at t_end.  w_cut_fac is accepted and ignored, as the semi-Lagrangian
    advection ignores w_cut (functions.py:528-529)."""
    if scheme != "semilagrangian" or isochoric or normalize_phi:
        raise NotImplementedError(
            "disc_in_tg_run_one: the fused loop runs scheme='semilagrangian' with "
            "isochoric=False and normalize_phi=False; the other variants can be composed from "
            "functions.advect_reference_map, functions.extrapolate_reference_map, "
            "functions.solid_cauchy_stress, functions.smoothed_heaviside, "
            "mac.momentum_predictor_freeslip and mac.project")
    return _disc_in_tg_run(N, t_end, R, x0, y0, mu_s, mu_f, U0, rho)[1]


def _disc_in_tg_run(N, t_end, R=0.15, x0=0.5, y0=0.7, mu_s=0.1, mu_f=0.01, U0=0.3, rho=1.0,
                    options=None):
    """(sim, run_one's dict): the loop to t_end (the last step truncated, :54-55), then the
    end-of-run measures of :84-91."""
    from .functions import compute_strain_energy
    if not math.isfinite(t_end):
        raise ValueError("disc_in_tg_run_one: a finite t_end")
    sim = MacDiscTaylorGreen(N, R, x0, y0, mu_s, mu_f, U0, rho, options=options)
    sim.step(2**31 - 1, t_end)   # (the loop ends at t_end)
    dx = sim.dx
    u, v = sim.field("u"), sim.field("v")
    u_c = 0.5 * (u[:, :-1] + u[:, 1:]); v_c = 0.5 * (v[:-1, :] + v[1:, :])
    sq = (u_c**2 + v_c**2).cpu().numpy()
    KE = 0.5 * np.sum(sq) * dx * dx
    # (the reference's compute_strain_energy returns the integrated scalar; the driver's
    # finite-only sum and second dx * dy factor are kept as they are, :87-88)
    se = compute_strain_energy(sim.field("X1"), sim.field("X2"), sim.field("phi"), mu_s, dx, dx)
    Estrain = np.nansum(np.where(np.isfinite(se), se, 0.0)) * dx * dx
    divmax = float(divergence(u, v, dx, dx).abs().max())
    return sim, dict(N=N, dx=dx, xc=(np.arange(N) + 0.5) * dx, speed=np.sqrt(sq), p=sim.get("p"),
                     KE=KE, Estrain=Estrain, divmax=divmax)


class MacTwoDiscContact(MacMultiDisc):
    """benchmarks/mac_two_disc_contact.py:21-84 on the GPU: two discs driven into each other
    on the free-slip box, rebounding through the contact stress (eta)."""

    def __init__(self, N=128, V0=0.3, eta=2.0, mu_s=0.2, mu_f=0.02, rho=1.0, R=0.12, sep=0.36,
                 options=None):
        from .functions import smoothed_heaviside
        xa, xb, yc0 = 0.5 - sep / 2, 0.5 + sep / 2, 0.5
        super().__init__(N, specs=[(R, xa, yc0), (R, xb, yc0)], U_lid=0.0, mu_s=mu_s, mu_f=mu_f,
                         rho=rho, eta=eta, options=options, walls="freeslip",
                         stop_on_divergence=False, dt=two_disc_dt(N, V0, mu_s, mu_f, rho))
        self.V0, self.R = V0, R
        dx = self.dx
        xc = (np.arange(N) + 0.5) * dx; xf = np.arange(N + 1) * dx
        Xu, Yu = np.meshgrid(xf, xc)
        w_t = 2.0 * dx
        HaU = np.asarray(smoothed_heaviside(np.sqrt((Xu - xa)**2 + (Yu - yc0)**2) - R, w_t))
        HbU = np.asarray(smoothed_heaviside(np.sqrt((Xu - xb)**2 + (Yu - yc0)**2) - R, w_t))
        u = V0 * (1 - HaU) - V0 * (1 - HbU)                            # :38-42
        u[:, 0] = 0; u[:, -1] = 0
        self.field("u").copy_(self.torch.from_numpy(u))
        self.torch.cuda.synchronize()

    def history(self):
        """The (t, cxA, cxB, gap) rows the driver's run returns (:82-84, 89)."""
        d = self.diagnostics()
        cx = d["cx"].reshape(-1, 2)
        return np.column_stack([d["t"], cx[:, 0], cx[:, 1], cx[:, 1] - cx[:, 0]])


# ------------------------------------------------------------------ lid-cavity disc loops --
class _LidDisc:
    """What the operator-composed loops of one soft disc (R 0.2 at (0.6, 0.5)) in the lid cavity
    share: the disc, the set-up, the projection with the symbol's axes split once, and the
    state.  A subclass names its state() fields in STATE and in KINDS those that are not a
    (N, N) cell plane: "uface" / "vface" the face shapes, "planes4" a list of four cell planes
    (one (4, N, N) array in state()), float / int a host scalar.  Each keeps its own step()."""

    X0, Y0, R, LAYERS = 0.6, 0.5, 0.2, 3
    STATE = ("u", "v", "X1", "X2", "t")
    KINDS = {"u": "uface", "v": "vface", "t": float}

    def _setup(self, N, rho, mu_f):
        """The grid, the disc's level set, the masked and extrapolated initial map, the fluid at
        rest, the projection's per-axis symbol, the context and the bookkeeping; returns the
        host (Xc, Yc, phi) of the cell centres."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pyrmt_amd needs a visible MI355X")
        from .bc import Disc
        self.torch, self.N, self.rho = torch, int(N), rho
        dx, dy = mac_grid(N, N)
        self.dx, self.dy, self.w_t, self.nu = dx, dy, 2.0 * dx, mu_f / rho
        self.disc = Disc(self.X0, self.Y0, self.R)
        xc = (np.arange(N) + 0.5) * dx
        Xc, Yc = np.meshgrid(xc, xc)
        Xg, Yg = np.meshgrid(np.arange(N) * dx, np.arange(N) * dy)
        phi = self.disc(Xc, Yc)
        m = (phi <= 0).astype(float)
        X1, X2 = extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, self.LAYERS)
        self.Xg, self.Yg, self.X1, self.X2 = map(self._dev, (Xg, Yg, X1, X2))
        self.u, self.v = self._dev(np.zeros((N, N + 1))), self._dev(np.zeros((N + 1, N)))
        self.lx, self.ly = _axis_eigs(poisson_eigs_neumann(N, N, dx, dy))
        self.ctx = ctx_for(N, N)
        self.t, self.nsteps, self.diverged, self.record = 0.0, 0, False, []
        return Xc, Yc, phi

    def _dev(self, h):
        return self.torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).cuda()

    @staticmethod
    def _dt_bounds(dx, U_lid, nu, mu_s, rho):
        """The advective, viscous and elastic-wave bounds on dt."""
        cs = np.sqrt(mu_s / rho)
        return 0.3 * dx / U_lid, 0.2 * dx * dx / nu, 0.3 * dx / (cs + 1e-9)

    def _project(self, ustar, vstar, dt):
        """project() with the symbol's axes split once at set-up (not per step): (u, v, p)."""
        u, v = self.torch.empty_like(ustar), self.torch.empty_like(vstar)
        p = ustar.new_empty((self.N, self.N))
        L.check(L.lib().rmt_mac_project(self.ctx.bind(), _p(ustar), _p(vstar), self.dx, self.dy,
                                        dt, float(self.rho), _hp(self.lx), _hp(self.ly), _p(u),
                                        _p(v), _p(p)), "project")
        return u, v, p

    def state(self):
        """Host copies of the fields of STATE."""
        g = lambda t: t.cpu().numpy()
        out = {}
        for k in self.STATE:
            kind, val = self.KINDS.get(k), getattr(self, k)
            out[k] = (val if kind in (float, int) else
                      np.stack([g(p) for p in val]) if kind == "planes4" else g(val))
        return out

    def set_state(self, state):
        """The fields of state() (arrays or device tensors; any subset)."""
        unknown = set(state) - set(self.STATE)
        if unknown:
            raise KeyError(f"set_state: unknown fields {sorted(unknown)}; one of {self.STATE}")
        N, io = self.N, _IO(None)
        shapes = {"uface": (N, N + 1), "vface": (N + 1, N), "planes4": (4, N, N)}
        for k, val in state.items():
            kind = self.KINDS.get(k)
            if kind in (float, int):
                setattr(self, k, kind(val))
                continue
            if tuple(np.shape(val)) != shapes.get(kind, (N, N)):
                raise ValueError(f"set_state: {k} has shape {tuple(np.shape(val))}")
            d = io.dev(val).clone()
            setattr(self, k, [d[i].contiguous() for i in range(4)] if kind == "planes4" else d)
        self.diverged = False

    def get(self, name):
        return getattr(self, name).cpu().numpy()


def _run_to(what, t_end, make):
    """Integrate make() to a finite t_end or to its `diverged` stop (t_end is checked before
    the sim is made: the refusal needs no device)."""
    if not math.isfinite(t_end):
        raise ValueError(f"{what}: a finite t_end")
    return make().step(2**31 - 1, t_end)


# ------------------------------------------------------------------ reinitialisation --
# benchmarks/mac_reinit_test.py:23-113 (Rycroft 2018) through mac_reinit.hip: the reference map
# is reset to the identity when the epoch's distortion gets large, the deformation gathered so
# far lives on as four advected, extrapolated planes Fs, the shape as a stored level set phiref,
# and the stress comes from F_total = F_current . Fs.
def _planes4(io, Fs, shape, what):
    Fd = [io.dev(p) for p in Fs]
    if len(Fd) != 4 or any(tuple(p.shape) != tuple(shape) for p in Fd):
        raise ValueError(f"{what}: Fs is four planes (11, 12, 21, 22) of the map's shape")
    return Fd


def total_stress(X1, X2, Fs, phi, dx, dy, w_t, mu_s, with_Ftot=False):
    """mac_reinit_test.py:74-81: (Sxx, Sxy, Syy, J_ep) of the total deformation
    F_current(X1, X2) . Fs, S = (1 - smoothed_heaviside(phi, w_t)) mu_s b; with_Ftot: a fifth
    item, the list of the four Ftot planes (what a reinitialisation stores, :98)."""
    shape = _plane2("total_stress", X1=X1, X2=X2, phi=phi)
    io = _IO(X1, X2, phi, *Fs); X1d, X2d, pd = map(io.dev, (X1, X2, phi))
    Fd = _planes4(io, Fs, shape, "total_stress")
    outs = [io.empty(shape) for _ in range(4)]
    Ft = [io.empty(shape) for _ in range(4)] if with_Ftot else None
    L.check(L.lib().rmt_mac_total_stress(ctx_for(*shape).bind(), _p(X1d), _p(X2d), _plane_ptrs(Fd),
                                         _p(pd), float(dx), float(dy), float(w_t), float(mu_s),
                                         *map(_p, outs), _plane_ptrs(Ft) if Ft else None),
            "total_stress")
    res = tuple(io.out(o) for o in outs)
    return res + ([io.out(p) for p in Ft],) if with_Ftot else res


def total_force(X1, X2, Fs, phi, dx, dy, w_t, mu_s):
    """mac_reinit_test.py:74-85 in one launch: (fu (Ny, Nx+1), fv (Ny+1, Nx), J_ep), the face
    forces of that stress (central divergence, averaged to the interior faces, wall faces 0);
    the same bits as total_stress, grad_central_*_2nd and the average composed."""
    shape = _plane2("total_force", X1=X1, X2=X2, phi=phi)
    io = _IO(X1, X2, phi, *Fs); X1d, X2d, pd = map(io.dev, (X1, X2, phi))
    Fd = _planes4(io, Fs, shape, "total_force")
    ny, nx = shape
    fu = io.empty((ny, nx + 1)); fv = io.empty((ny + 1, nx)); J = io.empty(shape)
    L.check(L.lib().rmt_mac_total_force(ctx_for(ny, nx).bind(), _p(X1d), _p(X2d), _plane_ptrs(Fd),
                                        _p(pd), float(dx), float(dy), float(w_t), float(mu_s),
                                        _p(fu), _p(fv), _p(J)), "total_force")
    return io.out(fu), io.out(fv), io.out(J)


def epoch_distortion(J_ep, phi, out=None):
    """mac_reinit_test.py:91-94: (max J_ep, min J_ep, number of cells) over phi <= 0 as three
    doubles (a device tensor for device inputs, written into `out` when given; -inf, +inf, 0
    without a solid cell; NaN propagates as in ndarray.max)."""
    shape = _plane2("epoch_distortion", J_ep=J_ep, phi=phi)
    io = _IO(J_ep, phi); Jd, pd = io.dev(J_ep), io.dev(phi)
    o = io.empty((3,)) if out is None else out
    L.check(L.lib().rmt_mac_epoch_distortion(ctx_for(*shape).bind(), _p(Jd), _p(pd), _p(o)),
            "epoch_distortion")
    return io.out(o)


class MacReinitDisc(_LidDisc):
    """The loop body of benchmarks/mac_reinit_test.py:59-106 on device tensors, composed from
    operators (no fused step): a soft disc (R 0.2 at (0.6, 0.5)) in the lid cavity whose map
    is reinitialised when the epoch distortion max(max J, 1 / min J) over the solid exceeds
    reinit_J.  A step: phi = phiref(xi) (bilinear), the six planes xi1, xi2, Fs advected on one
    backtrace and masked (rmt_advect_sl_rk4_multi), three extrapolations, phi again, the face
    forces of the total stress in one launch (rmt_mac_total_force), predictor, projection, the
    distortion reduction; the host reads four scalars (max J, min J, the solid's cell count,
    max|u|) once and decides the reinitialisation and the `diverged` stop as :91-106 do.
    reinit=False: the plain loop, which folds and stops.  The advection skips the per-plane
    non-finite-velocity guard: the loop stops on a non-finite u before the next step reads it.

    `record`: one (t, dist, min J_ep, max J_ep, n_reinit, max|u|) per step.  state(): host
    copies of u, v, X1, X2, Fs (4, N, N), phiref, and t, n_reinit."""

    STATE = ("u", "v", "X1", "X2", "Fs", "phiref", "t", "n_reinit")
    KINDS = {**_LidDisc.KINDS, "Fs": "planes4", "n_reinit": int}

    def __init__(self, N=96, reinit=True, U_lid=1.0, mu_s=0.3, mu_f=0.01, rho=1.0, reinit_J=1.8):
        Xc, Yc, phi = self._setup(N, rho, mu_f)                                # :42-47
        self.reinit, self.reinit_J = bool(reinit), reinit_J
        self.U_lid, self.mu_s, self.mu_f = U_lid, mu_s, mu_f
        dev = self._dev
        self.Xc, self.Yc, self.phiref = dev(Xc), dev(Yc), dev(phi)
        one, zero = np.ones((N, N)), np.zeros((N, N))
        self.Fs = [dev(one), dev(zero), dev(zero), dev(one)]
        self.dt = float(min(self._dt_bounds(self.dx, U_lid, self.nu, mu_s, rho)))
        self.stats = self.torch.empty(4, dtype=self.torch.float64, device="cuda")
        self.n_reinit, self.reinit_steps = 0, []
        self.phi = self.J_ep = None

    def _geom(self):
        """:55-56: phi = phiref(xi), bilinear at the cell-centred offset."""
        from .functions import bilinear_interpolate
        N = self.N
        return bilinear_interpolate(self.phiref, self.X1 - 0.5 * self.dx, self.X2 - 0.5 * self.dy,
                                    self.dx, self.dy, N, N)

    def _extrapolate_pairs(self, phi):
        dx, dy, Fs = self.dx, self.dy, self.Fs
        Fs[0], Fs[1] = extrapolate_reference_map(Fs[0], Fs[1], phi, dx, dy, self.LAYERS)
        Fs[2], Fs[3] = extrapolate_reference_map(Fs[2], Fs[3], phi, dx, dy, self.LAYERS)

    def step(self, nsteps=1, t_end=math.inf):
        from .functions import _advect_sl_rk4_multi
        torch, dx, dy, dt = self.torch, self.dx, self.dy, self.dt
        for _ in range(int(nsteps)):
            if self.diverged or not self.t < t_end:
                break
            if self.t + dt > t_end:
                dt = t_end - self.t                                            # :61-62
            u, v = self.u, self.v
            u_c = 0.5 * (u[:, :-1] + u[:, 1:]); v_c = 0.5 * (v[:-1, :] + v[1:, :])
            phi = self._geom()
            qs = [self.X1, self.X2] + self.Fs
            outs = [torch.empty_like(q) for q in qs]
            _advect_sl_rk4_multi(self.ctx, qs, u_c.contiguous(), v_c.contiguous(), self.Xg, self.Yg,
                                 dt, dx, dy, phi, outs)
            self.X1, self.X2 = extrapolate_reference_map(outs[0], outs[1], phi, dx, dy,
                                                         self.LAYERS)
            self.Fs = outs[2:]
            self._extrapolate_pairs(phi)
            phi = self._geom()
            fu, fv, J_ep = total_force(self.X1, self.X2, self.Fs, phi, dx, dy, self.w_t, self.mu_s)
            ustar, vstar = momentum_predictor(u, v, self.nu, dx, dy, dt, self.U_lid, fu=fu, fv=fv,
                                              rho=self.rho)
            self.u, self.v, _ = self._project(ustar, vstar, dt)
            self.t += dt
            self.nsteps += 1
            epoch_distortion(J_ep, phi, out=self.stats[:3])
            self.stats[3] = self.u.abs().max()
            maxJ, minJ, count, umax = self.stats.tolist()        # the step's one host read
            solid = count > 0
            dist = max(maxJ, 1.0 / max(minJ, 1e-6)) if solid else math.inf     # :91-96
            if self.reinit and dist > self.reinit_J and solid:                 # :97-103
                # Fs <- Ftot: the stress kernel once more with Ftot requested, so that the
                # per-step path never writes those four planes
                self.Fs = list(total_stress(self.X1, self.X2, self.Fs, phi, dx, dy, self.w_t,
                                            self.mu_s, with_Ftot=True)[4])
                self._extrapolate_pairs(phi)
                self.phiref = phi
                self.X1, self.X2 = self.Xc.clone(), self.Yc.clone()
                self.n_reinit += 1
                self.reinit_steps.append(self.nsteps)
            self.phi, self.J_ep = phi, J_ep
            self.record.append((self.t, dist, minJ, maxJ, self.n_reinit, umax))
            if not math.isfinite(umax) or not solid:                           # :105-106
                self.diverged = True
        return self


def mac_reinit_run(N=96, t_end=15.0, reinit=True, U_lid=1.0, mu_s=0.3, mu_f=0.01, rho=1.0,
                   reinit_J=1.8, return_sim=False):
    """mac_reinit_test.py:36-113 (run): integrate to t_end or to the `diverged` stop; returns
    the time reached (return_sim: (t, the MacReinitDisc))."""
    sim = _run_to("mac_reinit_run", t_end,
                  lambda: MacReinitDisc(N, reinit, U_lid, mu_s, mu_f, rho, reinit_J))
    return (sim.t, sim) if return_sim else sim.t


# ------------------------------------------------------------------ integrator ladder --
# benchmarks/mac_soft_disc_lid.py (the soft disc against Sugiyama 2011) under the reference's
# one-knob ladder explicit -> imex -> imex-elastic, each with an optional "-sl" suffix
# (mac.py:25-78), through mac_soft.hip.
INTEGRATORS = ("explicit", "imex", "imex-elastic")


def resolve_integrator(integrator=None, imex=False, elastic_imex=False, implicit_visc=False,
                       supports_elastic=True):
    """mac.py:46-78 (host): (canonical name, use_imex, use_elastic) of a unified `integrator=`
    name (aliases accepted) or, with None, of the legacy booleans."""
    if integrator is None:
        name = "imex-elastic" if elastic_imex else "imex" if (imex or implicit_visc) else "explicit"
    else:
        key = str(integrator).lower().replace("_", "-").strip()
        aliases = {
            "explicit": "explicit", "exp": "explicit", "forward-euler": "explicit",
            "imex": "imex", "imex-visc": "imex", "implicit-viscosity": "imex",
            "semi-implicit": "imex",
            "imex-elastic": "imex-elastic", "elastic": "imex-elastic",
            "implicit-elastic": "imex-elastic",
        }
        if key not in aliases:
            raise ValueError(f"unknown integrator {integrator!r}; choose from {INTEGRATORS}")
        name = aliases[key]
    if name == "imex-elastic" and not supports_elastic:
        raise ValueError("integrator='imex-elastic' is not available for this driver "
                         "(no solid-stress force path); use 'explicit' or 'imex'")
    return name, name in ("imex", "imex-elastic"), name == "imex-elastic"


def _faces2(what, shape, u, v):
    ny, nx = shape
    got = (tuple(np.shape(u)), tuple(np.shape(v)))
    if got != ((ny, nx + 1), (ny + 1, nx)):
        raise ValueError(f"{what}: u (Ny, Nx+1) and v (Ny+1, Nx) of the {shape} cells; got {got}")


def _stencil_shape(what, **planes):
    shape = _plane2(what, **planes)
    if min(shape) < 5:
        raise ValueError(f"{what}: Ny, Nx >= 5 (the one-sided edge stencils); got {shape}")
    return shape


def solid_force(X1, X2, phi, dx, dy, w_t, mu_s, kappa=0.0, detg_clamp=0.0, isochoric=False):
    """mac_soft_disc_lid.py:103-110 in one launch: (fu (Ny, Nx+1), fv (Ny+1, Nx), J), the face
    forces of the neo-Hookean stress of solid_cauchy_stress (w_cut = 0) blended with
    1 - smoothed_heaviside(phi, w_t): central divergence, averaged to the interior faces, wall
    faces 0.  The same bits as those operators composed."""
    ny, nx = _stencil_shape("solid_force", X1=X1, X2=X2, phi=phi)
    io = _IO(X1, X2, phi); X1d, X2d, pd = map(io.dev, (X1, X2, phi))
    fu = io.empty((ny, nx + 1)); fv = io.empty((ny + 1, nx)); J = io.empty((ny, nx))
    L.check(L.lib().rmt_mac_solid_force(ctx_for(ny, nx).bind(), _p(X1d), _p(X2d), _p(pd),
                                        float(dx), float(dy), float(w_t), float(mu_s),
                                        float(kappa), float(detg_clamp), int(bool(isochoric)),
                                        _p(fu), _p(fv), _p(J)), "solid_force")
    return io.out(fu), io.out(fv), io.out(J)


def midpoint_centres(u0, v0, u1, v1):
    """mac_soft_disc_lid.py:133-134: the mean of two face velocities averaged to the cell
    centres, (uc, vc); with u1 is u0 and v1 is v0 the plain average of :82-83."""
    shape = (np.shape(u0)[0], np.shape(v0)[1]) if np.ndim(u0) == 2 and np.ndim(v0) == 2 else ()
    if len(shape) != 2 or min(shape) < 2:
        raise ValueError("midpoint_centres: u (Ny, Nx+1) and v (Ny+1, Nx) faces")
    _faces2("midpoint_centres", shape, u0, v0)
    _faces2("midpoint_centres", shape, u1, v1)
    io = _IO(u0, v0, u1, v1); u0d, v0d = io.dev(u0), io.dev(v0)
    u1d = u0d if u1 is u0 else io.dev(u1); v1d = v0d if v1 is v0 else io.dev(v1)
    uc = io.empty(shape); vc = io.empty(shape)
    L.check(L.lib().rmt_mac_midpoint_centres(_pctx(shape, True), _p(u0d), _p(v0d), _p(u1d),
                                             _p(v1d), _p(uc), _p(vc)), "midpoint_centres")
    return io.out(uc), io.out(vc)


def soft_diag(phi, J, u, v, dx, dy, out=None):
    """What mac_soft_disc_lid.py:139-150 reads, in one reduction, as eight doubles (a device
    tensor for device inputs, written into `out` when given): the number of phi <= 0 cells, the
    sums of Xc and Yc over them, min J, max J, max|u|, max|v| (NaN propagates as in
    ndarray.min / max) and 1.0 if u or v holds a non-finite value."""
    shape = _plane2("soft_diag", phi=phi, J=J)
    _faces2("soft_diag", shape, u, v)
    io = _IO(phi, J, u, v); pd, Jd, ud, vd = map(io.dev, (phi, J, u, v))
    o = io.empty((8,)) if out is None else out
    L.check(L.lib().rmt_mac_soft_diag(_pctx(shape, True), _p(pd), _p(Jd), _p(ud), _p(vd),
                                      float(dx), float(dy), _p(o)), "soft_diag")
    return io.out(o)


def advect_xi_conservative(xi, u, v, dx, dy, dt, phi, w_cut=0.0):
    """mac.py:713-721: SSP-RK3 of -H div(u xi) for a cell-centred map component with the MAC
    face velocity (Jain 2019, eq. 26), H = (phi <= w_cut); the reference's bits."""
    shape = _plane2("advect_xi_conservative", xi=xi, phi=phi)
    _faces2("advect_xi_conservative", shape, u, v)
    io = _IO(xi, u, v, phi); xd, ud, vd, pd = map(io.dev, (xi, u, v, phi))
    out = io.empty(shape)
    L.check(L.lib().rmt_mac_advect_xi_conservative(_pctx(shape, True), _p(xd), _p(ud), _p(vd),
                                                   float(dx), float(dy), float(dt), _p(pd),
                                                   float(w_cut), _p(out)),
            "advect_xi_conservative")
    return io.out(out)


class MacSoftDisc(_LidDisc):
    """The loop body of benchmarks/mac_soft_disc_lid.py:79-150 on device tensors, composed from
    operators (no fused step): the soft disc (R 0.2 at (0.6, 0.5), kappa 0, rho 1, mu_f 0.01,
    w_t = 2 dx, U_lid 1, 3 extrapolation layers) under the integrator ladder.

    explicit / imex (and imex-sl): phi from the map, both map components advected with the
    centre velocity and masked with that phi, extrapolated, phi again, the face forces in one
    launch (rmt_mac_solid_force), predictor, projection.  imex-elastic (and imex-elastic-sl):
    forces from the un-advected map, the predictor with cs2 = mu_s / rho, projection, then the
    map advanced with the midpoint velocity of the old and new faces; phi and mask are the
    step's first.  The "-sl" rungs go through momentum_predictor_lid_semilag's CFL switch.
    One reduction (rmt_mac_soft_diag) feeds the stop test and the record: the host reads its
    eight doubles once a step (the -sl rungs also read the CFL, the IMEX solves r.r).  The stop
    test of :139-147 (no solid cell, non-finite u or v, min J < 0, max J > 20) comes before
    t += dt: a diverging step leaves no row and sets `diverged`.  dt is not clipped to t_end.
    The semi-Lagrangian map advection skips the non-finite-velocity guard: the loop stops on a
    non-finite velocity before the next step reads it.

    `record`: one (t, cx, cy, min J, max J) per step; `sl_steps`: the steps that took the
    semi-Lagrangian branch; `pcg_iters`: the last step's two PCG counts.  state(): host copies
    of u, v, X1, X2, and t."""

    KAPPA, RHO, MU_F, U_LID = 0.0, 1.0, 0.01, 1.0
    SCHEMES = ("semilagrangian", "semilagrangian_cubic", "central2", "weno5")

    def __init__(self, N=128, integrator=None, imex=False, dt=None, mu_s=0.1,
                 scheme="semilagrangian", w_cut_fac=0.0, detg_clamp=0.0, isochoric=False,
                 reinit=False):
        name, self.use_semilag, self.use_imex, self.use_elastic = self.parse_integrator(
            integrator, imex)
        self.integrator = name
        if scheme == "conservative" or reinit:
            raise NotImplementedError(
                "MacSoftDisc: scheme='conservative' and reinit=True need the reference's FMM "
                "level-set reinitialisation (scikit-fmm), which is not part of this build")
        if scheme not in self.SCHEMES:
            raise ValueError("Unknown advection scheme %r (expected one of %s)"
                             % (scheme, ", ".join(self.SCHEMES)))
        if scheme in ("central2", "weno5") and w_cut_fac == 0.0:
            w_cut_fac = 4.0                                                    # :43-45
        self._setup(N, self.RHO, self.MU_F)                                    # :51
        self.scheme, self.mu_s = scheme, float(mu_s)
        self.w_cut_fac, self.detg_clamp, self.isochoric = w_cut_fac, detg_clamp, bool(isochoric)
        cs = np.sqrt(mu_s / self.RHO)
        self.cs2 = float(cs * cs) if self.use_elastic else 0.0                 # :113
        self.dt = float(self.default_dt(N, name, mu_s) if dt is None else dt)
        self.stats = self.torch.empty(8, dtype=self.torch.float64, device="cuda")
        self.sl_steps, self.pcg_iters = 0, (0, 0)
        self.phi = self.J = None

    @staticmethod
    def parse_integrator(integrator=None, imex=False):
        """:57-62 (host): the "-sl" suffix, then the ladder: (canonical name with its suffix,
        use_semilag, use_imex, use_elastic)."""
        istr = str(integrator).lower().replace("_", "-") if integrator is not None else ""
        use_semilag = istr.endswith("-sl")
        base = (istr[:-3] or "imex") if use_semilag else integrator
        name, use_imex, use_elastic = resolve_integrator(base, imex=imex, supports_elastic=True)
        if use_semilag:
            use_imex = True; name = name + "-sl"
        return name, use_semilag, use_imex, use_elastic

    @classmethod
    def default_dt(cls, N, integrator, mu_s=0.1):
        """:63-74 for a canonical integrator name ("explicit", "imex", "imex-elastic", each with
        an optional "-sl")."""
        dx = 1.0 / N
        sl = integrator.endswith("-sl")
        _, use_imex, use_elastic = resolve_integrator(integrator[:-3] if sl else integrator)
        dt_adv, dt_visc, dt_elastic = cls._dt_bounds(dx, cls.U_LID, cls.MU_F / cls.RHO, mu_s,
                                                     cls.RHO)
        if sl and use_elastic:
            return 2.0 * dt_adv
        if sl:
            return min(2.0 * dt_adv, dt_elastic)
        if use_elastic:
            return dt_adv
        if use_imex:
            return min(dt_adv, dt_elastic)
        return min(dt_adv, dt_visc, dt_elastic)

    def _advect_maps(self, a, b, phi):
        """:96-98 / :135-137: both components advected with the centre velocity (a, b), masked
        with (phi <= 0), extrapolated."""
        from . import functions as F
        torch, dx, dy, dt, wc = self.torch, self.dx, self.dy, self.dt, self.w_cut_fac * self.dx
        if self.scheme == "semilagrangian":
            outs = [torch.empty_like(self.X1), torch.empty_like(self.X2)]
            F._advect_sl_rk4_multi(self.ctx, [self.X1, self.X2], a, b, self.Xg, self.Yg, dt, dx,
                                   dy, phi, outs)
        else:
            sm = (phi <= 0).to(torch.float64)
            if self.scheme == "semilagrangian_cubic":
                adv = lambda q: F.advect_semilagrangian_cubic_rk4(q, a, b, self.Xg, self.Yg, dt,
                                                                  dx, dy)
            elif self.scheme == "central2":
                adv = lambda q: F.advect_central2_rk3(q, a, b, dx, dy, dt, phi, wc)
            else:
                adv = lambda q: F.advect_weno5_rk3(q, a, b, dx, dy, dt, phi, wc)
            outs = [adv(self.X1) * sm, adv(self.X2) * sm]
        self.X1, self.X2 = extrapolate_reference_map(outs[0], outs[1], phi, dx, dy, self.LAYERS)

    def step(self, nsteps=1, t_end=math.inf):
        from .functions import rebuild_phi_from_reference_map
        dx, dy, dt, rho = self.dx, self.dy, self.dt, self.RHO
        for _ in range(int(nsteps)):
            if self.diverged or not self.t < t_end:
                break
            u, v = self.u, self.v
            phi = rebuild_phi_from_reference_map(self.X1, self.X2, self.disc)      # :84
            if not self.use_elastic:
                u_c, v_c = midpoint_centres(u, v, u, v)                            # :82-83
                self._advect_maps(u_c, v_c, phi)
                phi = rebuild_phi_from_reference_map(self.X1, self.X2, self.disc)  # :99
            fu, fv, J = solid_force(self.X1, self.X2, phi, dx, dy, self.w_t, self.mu_s,
                                    self.KAPPA, self.detg_clamp, self.isochoric)
            took_sl, its = False, (0, 0)
            if self.use_semilag:                                                   # :114-127
                ustar, vstar, its, took_sl = _predictor_lid_semilag(
                    u, v, self.nu, dx, dy, dt, self.U_LID, fu, fv, rho, self.cs2, 1e-8, 0.9)
            elif self.use_imex:
                ustar, vstar, its = _predictor_lid_imex(u, v, self.nu, dx, dy, dt, self.U_LID, fu,
                                                        fv, rho, 1e-8, self.cs2)
            else:
                ustar, vstar = momentum_predictor(u, v, self.nu, dx, dy, dt, self.U_LID, fu=fu,
                                                  fv=fv, rho=rho)
            un, vn, _ = self._project(ustar, vstar, dt)
            if self.use_elastic:                                                   # :130-137
                umc, vmc = midpoint_centres(u, v, un, vn)
                self._advect_maps(umc, vmc, phi)
            self.u, self.v, self.phi, self.J = un, vn, phi, J
            self.pcg_iters = tuple(its)
            soft_diag(phi, J, un, vn, dx, dy, out=self.stats)
            count, sx, sy, minJ, maxJ, _, _, bad = self.stats.tolist()  # the step's host read
            if count == 0 or bad or minJ < 0.0 or maxJ > 20.0:                     # :139-147
                self.diverged = True
                break
            self.t += dt
            self.nsteps += 1
            self.sl_steps += int(took_sl)
            self.record.append((self.t, sx / count, sy / count, minJ, maxJ))
        return self


def mac_soft_disc_run(N=128, t_end=8.0, scheme="semilagrangian", w_cut_fac=0.0, detg_clamp=0.0,
                      reinit=False, isochoric=False, imex=False, dt=None, integrator=None,
                      mu_s=0.1, return_sim=False):
    """mac_soft_disc_lid.py:23-157 (run(..., write=False)): integrate to t_end or to the
    `diverged` stop; returns the (n, 5) trajectory (t, cx, cy, min J, max J) (return_sim:
    (trajectory, the MacSoftDisc))."""
    sim = _run_to("mac_soft_disc_run", t_end, lambda: MacSoftDisc(
        N, integrator=integrator, imex=imex, dt=dt, mu_s=mu_s, scheme=scheme, w_cut_fac=w_cut_fac,
        detg_clamp=detg_clamp, isochoric=isochoric, reinit=reinit))
    traj = np.array(sim.record)
    return (traj, sim) if return_sim else traj


# ------------------------------------------------- viscoelastic blob, four-roll mill ----
# benchmarks/mac_viscoelastic_extension.py (a soft blob at the stagnation point of a four-roll
# mill; the elastic limit diverges, the viscoelastic case saturates at b_xx = 1 / (1 - 2 Wi))
# through mac_ve.hip: what joins the constitutive layer (pyrmt_amd.viscoelastic) to the periodic
# tier above.  Planes are (Ny, Nx) with Ny, Nx >= 3; the face averages wrap, the gradients are
# the collocated grad_central_*_2nd (one-sided at the first and last column / row).
def _ve_shape(what, **planes):
    """The common (Ny, Nx) of 2-D planes with Ny, Nx >= 3 (host check, before any device
    call)."""
    shapes = {k: tuple(np.shape(a)) for k, a in planes.items()}
    first = next(iter(shapes.values()))
    if len(first) != 2 or min(first) < 3 or any(sh != first for sh in shapes.values()):
        raise ValueError(f"{what}: (Ny, Nx) planes of one shape with Ny, Nx >= 3; got {shapes}")
    return first


def ve_centre_kinematics(u, v, dx, dy):
    """mac_viscoelastic_extension.py:106, :119-120 in one launch: (u_c, v_c, L11, L12, L21,
    L22), u_c = 0.5 (u + roll(u, -1, 1)), v_c = 0.5 (v + roll(v, -1, 0)) and their
    grad_central_{x,y}_2nd; the reference's bits."""
    shape = _ve_shape("ve_centre_kinematics", u=u, v=v)
    io = _IO(u, v); ud = io.dev(u); vd = io.dev(v)
    o = io.empty((6,) + shape)
    L.check(L.lib().rmt_mac_ve_centre_kinematics(_pctx(shape, True), _p(ud), _p(vd), float(dx),
                                                 float(dy), _p(o[0]), _p(o[1]),
                                                 _plane_ptrs([o[2], o[3], o[4], o[5]])),
            "ve_centre_kinematics")
    return tuple(io.out(o[k]) for k in range(6))


def ve_face_force(be11, be12, be22, phi, G, w_t, dx, dy):
    """mac_viscoelastic_extension.py:125-131: (f_su, f_sv, Hu, Hv, chi) of the stress
    S = (1 - H) G b_e, H = smoothed_heaviside(phi, w_t): div S averaged onto the x / y faces, H
    there, and chi = 1 - H at the centres."""
    shape = _ve_shape("ve_face_force", be11=be11, be12=be12, be22=be22, phi=phi)
    io = _IO(be11, be12, be22, phi)
    b = [io.dev(a) for a in (be11, be12, be22)]; pd = io.dev(phi)
    o = io.empty((5,) + shape)
    L.check(L.lib().rmt_mac_ve_face_force(_pctx(shape, True), _plane_ptrs(b), _p(pd), float(G),
                                          float(w_t), float(dx), float(dy),
                                          *[_p(o[k]) for k in range(5)]), "ve_face_force")
    return tuple(io.out(o[k]) for k in range(5))


def _imex_elastic(what, solve, u, v, nu, dx, dy, dt, lap_eig, cs2, chi_c, fu, fv, rho):
    shape = _ve_shape(what, u=u, v=v, chi_c=chi_c, fu=fu, fv=fv)
    c_el = dt * dt * cs2                                                    # mac.py:573, 580
    io = _IO(u, v, chi_c, fu, fv)
    ud, vd, xd, fud, fvd = (io.dev(a) for a in (u, v, chi_c, fu, fv))
    us = io.empty(shape); vs = io.empty(shape)
    head = (_pctx(shape, True), _p(ud), _p(vd), float(2 * dx), float(2 * dy), float(dx**2),
            float(dy**2), float(dt), float(c_el))
    if solve:
        if tuple(np.shape(lap_eig)) != shape:
            raise ValueError(f"{what}: the fields and lap_eig differ in shape")
        lx, ly = _axis_eigs_per(lap_eig, False)
        L.check(L.lib().rmt_mac_per_predictor_imex_elastic(
            *head, float(dt * nu + c_el), float(rho), _p(xd), _p(fud), _p(fvd), _hp(lx), _hp(ly),
            _p(us), _p(vs)), what)
    else:
        L.check(L.lib().rmt_mac_per_imex_elastic_rhs(*head, float(rho), _p(xd), _p(fud), _p(fvd),
                                                     _p(us), _p(vs)), what)
    return io.out(us), io.out(vs)


def momentum_predictor_periodic_imex_elastic(u, v, nu, dx, dy, dt, lap_eig, cs2, chi_c, fu, fv,
                                             rho=1.0):
    """mac.py:560-584: the IMEX predictor with the linearly-implicit elastic-wave stabiliser
    c_el = dt^2 cs2: explicit central advection, the face force fu / fv inside the solve, the
    defect c_el (1 - chi_face) lap that removes the stabiliser from the fluid, then
    (I - (dt nu + c_el) Lap) x = rhs per component by FFT.  chi_c: the solid indicator at the
    centres.  Returns (u*, v*)."""
    return _imex_elastic("momentum_predictor_periodic_imex_elastic", True, u, v, nu, dx, dy, dt,
                         lap_eig, cs2, chi_c, fu, fv, rho)


def imex_elastic_rhs(u, v, dx, dy, dt, cs2, chi_c, fu, fv, rho=1.0):
    """mac.py:566-579 alone: (rhs_u, rhs_v) of momentum_predictor_periodic_imex_elastic's two
    solves (arithmetic only: the reference's bits)."""
    return _imex_elastic("imex_elastic_rhs", False, u, v, 0.0, dx, dy, dt, None, cs2, chi_c, fu,
                         fv, rho)


VE_LOCK_MODES = {"explicit": 0, "imex": 1, "imex-elastic": 2}


def ve_lock(star, u, f_s, Hf, mill, dt, beta, rho, mode):
    """mac_viscoelastic_extension.py:139-155 on one velocity component: the solid force and the
    lock of the fluid to the mill applied to the predictor's u* (`star`).  mode "explicit":
    u* + dt (f_s + Hf beta (mill - u)) / rho; "imex": mill + (u* + dt f_s / rho - mill)
    exp(-dt beta Hf / rho), the relaxation towards the mill integrated exactly; "imex-elastic":
    the same without the force (it went into the predictor's solve)."""
    if mode not in VE_LOCK_MODES:
        raise ValueError(f"ve_lock: mode is one of {tuple(VE_LOCK_MODES)}, got {mode!r}")
    shape = _ve_shape("ve_lock", star=star, u=u, f_s=f_s, Hf=Hf, mill=mill)
    io = _IO(star, u, f_s, Hf, mill)
    sd, ud, fd, hd, md = (io.dev(a) for a in (star, u, f_s, Hf, mill))
    out = io.empty(shape)
    L.check(L.lib().rmt_mac_ve_lock(_pctx(shape, True), VE_LOCK_MODES[mode], sd.numel(), _p(sd),
                                    _p(ud), _p(fd), _p(hd), _p(md), float(dt), float(beta),
                                    float(rho), _p(out)), "ve_lock")
    return io.out(out)


def ve_record(be11, be12, be22, phi, u, at, out=None):
    """mac_viscoelastic_extension.py:159-171 as one reduction: five doubles, the largest
    eigenvalue of b_e over phi <= 0 (NaN propagates; -inf without such a cell), the number of
    those cells, be11 at the flat index `at`, max |u| (NaN propagates) and 1.0 / 0.0 for u all
    finite or not (a device tensor for device inputs, written into `out` when given).  The
    planes share one shape, of any rank."""
    shapes = {tuple(np.shape(a)) for a in (be11, be12, be22, phi, u)}
    if len(shapes) != 1 or not int(np.prod(next(iter(shapes)), dtype=np.int64)) >= 1:
        raise ValueError(f"ve_record: non-empty planes of one shape, got {sorted(shapes)}")
    io = _IO(be11, be12, be22, phi, u)
    b = [io.dev(a) for a in (be11, be12, be22)]; pd = io.dev(phi); ud = io.dev(u)
    o = io.empty((5,)) if out is None else out
    L.check(L.lib().rmt_mac_ve_record(ctx_for(5, 5).bind(), pd.numel(), _plane_ptrs(b), _p(pd),
                                      _p(ud), int(at), _p(o)), "ve_record")
    return io.out(o)


class MacViscoelasticExtension:
    """The loop body of benchmarks/mac_viscoelastic_extension.py:102-171 on device tensors: a
    soft blob (radius R at the centre of the unit square) in the four-roll mill
    u_mill = U0 (sin kx cos ky, -cos kx sin ky), k = 2 pi, U0 = eps_rate / k, to which a
    penalisation (beta = 150) locks the fluid.  A step: centre kinematics; phi rebuilt from the
    map; the five planes X1, X2, p11, p12, p22 advected on one backtrace and masked; three
    extrapolations (p22 with a zero partner); the log-conformation step (Strang under "imex" and
    "imex-elastic", explicit RK2 otherwise); sym_exp; the face force; the integrator's predictor
    (explicit, IMEX, elastic IMEX); the lock; the periodic projection; the record reduction,
    whose five doubles are the step's one host read.  tau <= 0 means inf.  dt: the reference's
    choice (:75-85) unless given.  t and dt are host floats formed as the reference forms them.

    `record`: one (t, lam_max, b_xx(centre), max|u|) per step (lam_max NaN without a solid
    cell); `dts`: the step sizes; history(t_end): the reference's view, every 100th step and
    those with t >= t_end.  The loop stops (`stopped`, `clause`) when u is not all finite, no
    solid cell is left or lam_max > 1e4 (:170)."""

    LAYERS, BETA = 3, 150.0

    def __init__(self, N=128, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.05, rho=1.0, R=0.13,
                 integrator=None, imex=False, elastic_imex=False, dt=None):
        from .functions import _torch
        self.integrator, self.imex, self.elastic = resolve_integrator(
            integrator, imex=imex, elastic_imex=elastic_imex, supports_elastic=True)
        if int(N) != N or N < 3:
            raise ValueError(f"MacViscoelasticExtension: N is a whole number >= 3, got {N!r}")
        torch = _torch()
        self.torch, self.N, self.R, self.G, self.rho = torch, int(N), float(R), G, rho
        N = self.N
        dx, dy = mac_grid(N, N)
        self.dx, self.dy = dx, dy
        xc = (np.arange(N) + 0.5) * dx; xf = np.arange(N) * dx                       # :52-60
        Xc, Yc = np.meshgrid(xc, xc)
        Xu, Yu = np.meshgrid(xf, xc); Xv, Yv = np.meshgrid(xc, xf)
        Xg, Yg = np.meshgrid(xf, xf)
        self.w_t = 2.0 * dx; self.nu = mu_f / rho
        k = 2.0 * np.pi; U0 = eps_rate / k
        u_mill = U0 * np.sin(k * Xu) * np.cos(k * Yu)
        v_mill = -U0 * np.cos(k * Xv) * np.sin(k * Yv)
        phi = np.sqrt((Xc - 0.5)**2 + (Yc - 0.5)**2) - R; m = (phi <= 0).astype(float)   # :64-66
        X1, X2 = extrapolate_reference_map(Xc * m, Yc * m, phi, dx, dy, self.LAYERS)
        dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).cuda()
        self.Xg, self.Yg, self.u_mill, self.v_mill, self.X1, self.X2 = map(
            dev, (Xg, Yg, u_mill, v_mill, X1, X2))
        z = lambda *s: torch.zeros(s + (N, N), dtype=torch.float64, device="cuda")
        self.psi = [z() for _ in range(3)]
        self.u, self.v, self.p, self.zero = z(), z(), z(), z()
        cs = np.sqrt(G / rho)                                                        # :75-85
        dt_adv = 0.25 * dx / max(U0, 0.1)
        dt_visc = 0.2 * dx * dx / self.nu
        dt_elastic = 0.3 * dx / (cs + 1e-9)
        if dt is None:
            dt = dt_adv if self.elastic else (min(dt_adv, dt_elastic) if self.imex
                                              else min(dt_adv, dt_visc, dt_elastic))
        self.dt = float(dt)
        self.tau = math.inf if tau <= 0 else float(tau)                              # :86-90
        self.Wi = eps_rate * self.tau
        self.bxx_analytic = (math.inf if (self.tau == math.inf or self.Wi >= 0.5)
                             else 1.0 / (1.0 - 2.0 * self.Wi))
        self.lx, self.ly = _axis_eigs_per(lap_eigs_periodic(N, N, dx, dy), False)
        self.ctx = ctx_for(N, N) if N >= 5 else None
        self.kin, self.be, self.ff = z(6), z(3), z(5)
        self.star = z(2)
        self.stats = torch.empty(5, dtype=torch.float64, device="cuda")
        self.phi = None
        self.t, self.nsteps, self.stopped, self.clause = 0.0, 0, False, None
        self.record, self.dts = [], []

    def _bind(self):
        return self.ctx.bind() if self.ctx is not None else _pctx((self.N, self.N), True)

    def step(self, nsteps=1, t_end=None):
        from .functions import _advect_sl_rk4_multi
        torch, lib, N, dx, dy, rho = self.torch, L.lib(), self.N, self.dx, self.dy, self.rho
        if self.ctx is None:
            raise ValueError("MacViscoelasticExtension.step: N >= 5 (advection, extrapolation)")
        t_end = math.inf if t_end is None else t_end
        dt, n, at = self.dt, N * N, (N // 2) * N + N // 2
        kin, be, ff, star = self.kin, self.be, self.ff, self.star
        Lp = _plane_ptrs([kin[2], kin[3], kin[4], kin[5]])
        bp = _plane_ptrs([be[0], be[1], be[2]])
        mode = VE_LOCK_MODES[self.integrator]
        for _ in range(int(nsteps)):
            if self.stopped or not self.t < t_end:
                break
            if self.t + dt > t_end:
                dt = t_end - self.t                                                # :104-105
            c = self.ctx.bind()
            L.check(lib.rmt_mac_ve_centre_kinematics(c, _p(self.u), _p(self.v), dx, dy, _p(kin[0]),
                                                     _p(kin[1]), Lp), "centre kinematics")
            phi = torch.empty_like(self.X1)
            L.check(lib.rmt_rebuild_phi_disc(c, _p(self.X1), _p(self.X2), 0.5, 0.5, self.R,
                                             _p(phi)), "rebuild_phi")              # :107
            qs = [self.X1, self.X2] + self.psi
            outs = [torch.empty_like(q) for q in qs]
            _advect_sl_rk4_multi(self.ctx, qs, kin[0], kin[1], self.Xg, self.Yg, dt, dx, dy, phi,
                                 outs)                                             # :110-116
            self.X1, self.X2 = extrapolate_reference_map(outs[0], outs[1], phi, dx, dy,
                                                         self.LAYERS)
            p11, p12 = extrapolate_reference_map(outs[2], outs[3], phi, dx, dy, self.LAYERS)
            p22, _ = extrapolate_reference_map(outs[4], self.zero, phi, dx, dy, self.LAYERS)
            self.psi = [p11, p12, p22]
            pp = _plane_ptrs(self.psi)
            c = self.ctx.bind()
            L.check(lib.rmt_ve_logconf_steps(c, n, pp, Lp, self.tau, dt, 1, int(self.imex), pp),
                    "logconf step")                                                # :121-122
            L.check(lib.rmt_ve_sym_exp(c, n, pp, bp), "sym_exp")
            L.check(lib.rmt_mac_ve_face_force(c, bp, _p(phi), float(self.G), self.w_t, dx, dy,
                                              *[_p(ff[k]) for k in range(5)]), "face force")
            us, vs = star[0], star[1]
            if self.elastic:                                                       # :137-138
                c_el = dt * dt * (self.G / rho)
                L.check(lib.rmt_mac_per_predictor_imex_elastic(
                    c, _p(self.u), _p(self.v), float(2 * dx), float(2 * dy), float(dx**2),
                    float(dy**2), dt, float(c_el), float(dt * self.nu + c_el), float(rho),
                    _p(ff[4]), _p(ff[0]), _p(ff[1]), _hp(self.lx), _hp(self.ly), _p(us), _p(vs)),
                    "elastic IMEX predictor")
            elif self.imex:                                                        # :146
                L.check(lib.rmt_mac_per_predictor_imex(
                    c, _p(self.u), _p(self.v), float(2 * dx), float(2 * dy), dt,
                    float(dt * self.nu), _hp(self.lx), _hp(self.ly), _p(us), _p(vs)),
                    "IMEX predictor")
            else:                                                                  # :154
                L.check(lib.rmt_mac_per_predictor(
                    c, _p(self.u), _p(self.v), float(self.nu), float(dx**2), float(dy**2),
                    float(2 * dx), float(2 * dy), dt, _p(us), _p(vs)), "explicit predictor")
            for s, w, f, H, mill in ((us, self.u, ff[0], ff[2], self.u_mill),
                                     (vs, self.v, ff[1], ff[3], self.v_mill)):     # :139-155
                L.check(lib.rmt_mac_ve_lock(c, mode, n, _p(s), _p(w), _p(f), _p(H), _p(mill), dt,
                                            self.BETA, float(rho), _p(s)), "lock")
            L.check(lib.rmt_mac_per_project(c, _p(us), _p(vs), dx, dy, float(rho / dt),
                                            float(dt / rho), _hp(self.lx), _hp(self.ly),
                                            _p(self.u), _p(self.v), _p(self.p)), "project")  # :156
            L.check(lib.rmt_mac_ve_record(c, n, bp, _p(phi), _p(self.u), at, _p(self.stats)),
                    "record")
            self.t += dt
            self.nsteps += 1
            lam, count, bxx_c, umax, finite = self.stats.tolist()    # the step's one host read
            if count == 0:
                lam = math.nan                                                     # :160
            self.phi = phi
            self.record.append((self.t, lam, bxx_c, umax))
            self.dts.append(dt)
            if not finite or count == 0 or lam > 1e4:                              # :170
                self.stopped = True
                self.clause = ("non-finite u" if not finite else "no solid cell" if count == 0
                               else "lam_max > 1e4")
        return self

    def history(self, t_end=math.inf):
        """The reference's `hist` (:163-164): every 100th step and those with t >= t_end."""
        return [r for k, r in enumerate(self.record, 1) if k % 100 == 0 or r[0] >= t_end]

    def get(self, name):
        """Host copy of u, v, p, X1, X2, phi, p11, p12, p22, be11, be12, be22, u_c, v_c, f_su,
        f_sv, Hu, Hv or chi (the last step's)."""
        planes = dict(u=self.u, v=self.v, p=self.p, X1=self.X1, X2=self.X2, phi=self.phi,
                      p11=self.psi[0], p12=self.psi[1], p22=self.psi[2], be11=self.be[0],
                      be12=self.be[1], be22=self.be[2], u_c=self.kin[0], v_c=self.kin[1],
                      f_su=self.ff[0], f_sv=self.ff[1], Hu=self.ff[2], Hv=self.ff[3],
                      chi=self.ff[4])
        return planes[name].cpu().numpy()


def mac_ve_extension_run(N=128, t_end=12.0, tau=0.5, eps_rate=0.5, G=0.3, mu_f=0.05, rho=1.0,
                         R=0.13, imex=False, elastic_imex=False, dt=None, integrator=None,
                         return_sim=False):
    """mac_viscoelastic_extension.run (:41-189) without frames and files: integrate to t_end or
    to the stop; returns (t, hist) as the reference does (return_sim: (t, hist, the
    MacViscoelasticExtension))."""
    if not math.isfinite(t_end):
        raise ValueError("mac_ve_extension_run: a finite t_end")
    sim = MacViscoelasticExtension(N, tau, eps_rate, G, mu_f, rho, R, integrator, imex,
                                   elastic_imex, dt).step(2**31 - 1, t_end)
    hist = sim.history(t_end)
    return (sim.t, hist, sim) if return_sim else (sim.t, hist)


def compare_integrators(N=40, tau=0.5, t_end=1.0, eps_rate=0.5, G=0.3, mu_f=0.05):
    """mac_viscoelastic_extension.compare_integrators (:253-280) as data: explicit against IMEX
    at the explicit viscous step (regression), and both at 2, 3 and 4 times it (capability).
    Returns dict(dt_visc, dt_elastic, explicit_bxx, imex_bxx, rel, rows), rows one (factor,
    explicit reached the end, IMEX reached the end, IMEX b_xx, its relative difference from
    explicit_bxx) per factor."""
    dx = 1.0 / N; nu = mu_f
    dt_visc = 0.2 * dx * dx / nu
    dt_elastic = 0.3 * dx / (np.sqrt(G) + 1e-9)
    cfg = dict(N=N, tau=tau, t_end=t_end, eps_rate=eps_rate, G=G, mu_f=mu_f)
    last = lambda h: h[-1][2] if h else math.nan
    end = lambda h: bool(h) and h[-1][0] >= t_end - 1e-9
    br = last(mac_ve_extension_run(imex=False, dt=dt_visc, **cfg)[1])
    bs = last(mac_ve_extension_run(imex=True, dt=dt_visc, **cfg)[1])
    rows = []
    for fac in (2, 3, 4):
        he = mac_ve_extension_run(imex=False, dt=fac * dt_visc, **cfg)[1]
        hi = mac_ve_extension_run(imex=True, dt=fac * dt_visc, **cfg)[1]
        rows.append((fac, end(he), end(hi), last(hi), abs(last(hi) - br) / br))
    return dict(dt_visc=dt_visc, dt_elastic=dt_elastic, explicit_bxx=br, imex_bxx=bs,
                rel=abs(bs - br) / br, rows=rows)
