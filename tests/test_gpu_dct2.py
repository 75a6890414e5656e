"""k_dct2 (pyrmt_amd/csrc/dct2.hip), the DCT-II Neumann solve of the MAC grid, beyond
power-of-two squares: mixed-radix plans, the 512-thread variant, several slots per thread with
a partly filled last one, ny != nx, the compile-time 8192 plan beside a generic one, single
row passes (rmt_selftest_dct2_rows), plan reuse and rejection.

References are scipy's pocketfft in long double, computed here.  Bar: 1e-13 of max|ref|, the
project's bar between FFT roundings (test_dct_solve_sizes, test_gpu_dct_sym.py); pocketfft in
float64 sits within 1.5e-15 (solve) and 4e-16 (row pass) of the long-double reference at
these shapes, so the reference has ~70x room under the bar (DESIGN.md section 4 lists the
figures per shape beside the GPU's)."""
import ctypes

import numpy as np
import pytest
from scipy.fft import dct, dctn, idct, idctn

pytestmark = pytest.mark.gpu

LD = np.longdouble
if dctn(np.ones((2, 2), LD), type=2, norm="ortho").dtype != LD or np.finfo(LD).eps >= 2e-19:
    pytest.skip("scipy.fft keeps no long double with eps < 2e-19 here: no reference for k_dct2",
                allow_module_level=True)

BAR = 1e-13

# (ny, nx) and the plan factor() gives each axis
ONE_SLOT = [(2, 6), (10, 14), (12, 18), (22, 26), (30, 36), (90, 126)]
# k_dct2<., 1>: [2 17] [2 19] [2 23]; a power-of-two axis dragged onto it by the shared `big`,
# both ways round; [2 17 23] x [2 17 19], two slots per thread on both axes
BIG = [(34, 38), (46, 34), (64, 34), (34, 64), (782, 646)]
# several slots, the last partly filled: 2310 = [3 7 10 11] (3 slots); 8190 = [7 9 10 13] (8,
# the last 2 short, non-power-of-two Ns); 1088 = [8 8 17] (512 threads, 3); 5888 = [4 8 8 23]
# (512 threads, 12, the last half full); 7168 = [2 7 8 8 8] (five passes)
SLOTS = [(4, 2310), (2310, 4), (6, 8190), (8190, 6), (6, 1088), (1088, 6), (8, 5888), (4, 7168)]
# the compile-time 8192 plan beside a generic one ((8192, 4): mode 1 on K2_8192)
K8192 = [(4, 8192), (8192, 4), (4, 4096)]
# odd n (Makhoul's reordering takes (n + 1) / 2 even samples): 3 = [3], 7 = [7], 9 = [9],
# 15 = [3 5], 33 = [3 11], 51 = [3 17] (512 threads), 1155 = [3 5 7 11] (2 slots, the last
# 131/1024), beside an even axis both ways round
ODD = [(3, 3), (7, 8), (9, 9), (15, 22), (33, 33), (8, 51), (3, 1155), (1155, 4)]


@pytest.fixture(scope="module")
def env(gpu):
    import torch
    from pyrmt_amd import functions as F, _lib as L, mac
    return torch, F, L, mac


def _ctx(env, ny, nx):
    torch, F, _, _ = env
    return F._Ctx(ny, nx, torch.cuda.current_device(), stencils=False)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _ref_solve(rhs, eig):
    h = dctn(rhs.astype(LD), type=2, norm="ortho") / eig.astype(LD)
    h[0, 0] = 0
    p = idctn(h, type=2, norm="ortho")
    assert p.dtype == LD
    return p


def _gpu_solve(env, c, rhs, lx=None, ly=None, out=None):
    torch, F, L, _ = env
    ny, nx = rhs.shape
    r = torch.from_numpy(rhs).cuda()
    out = torch.empty_like(r) if out is None else out
    L.check(L.lib().rmt_mac_solve_poisson_neumann(c.bind(), F._p(r), 1.0 / nx, 1.0 / ny, _hp(lx),
                                                  _hp(ly), F._p(out)), "solve_poisson_neumann")
    return out.cpu().numpy()


def _err(got, ref):
    return float(np.abs(got.astype(LD) - ref).max() / np.abs(ref).max())


def _case(mac, ny, nx):
    eig = mac.poisson_eigs_neumann(nx, ny, 1.0 / nx, 1.0 / ny)
    rhs = np.random.default_rng(7 * ny + nx).standard_normal((ny, nx))   # mean kept: the pin
    return rhs, eig


# ------------------------------------------------------------------ a. the solve --
@pytest.mark.parametrize("shape", ONE_SLOT + BIG + SLOTS + K8192 + ODD)
def test_solve_against_long_double(env, shape):
    """rmt_mac_solve_poisson_neumann on a (ny, nx) context against idctn(dctn(rhs) / eig) in
    long double; the right-hand side keeps its mean, so the (0, 0) pin decides the result."""
    mac = env[3]
    ny, nx = shape
    rhs, eig = _case(mac, ny, nx)
    lx, ly = mac._axis_eigs(eig)
    err = _err(_gpu_solve(env, _ctx(env, ny, nx), rhs, lx, ly), _ref_solve(rhs, eig))
    print(shape, err)
    assert err <= BAR, err


@pytest.mark.parametrize("shape", [(10, 14), (34, 64)])
def test_solve_rectangular_through_wrapper(env, shape):
    """mac.solve_poisson_neumann takes Ny != Nx, as the reference does."""
    mac = env[3]
    ny, nx = shape
    rhs, eig = _case(mac, ny, nx)
    got = mac.solve_poisson_neumann(rhs, eig)
    assert got.shape == rhs.shape
    err = _err(got, _ref_solve(rhs, eig))
    print(shape, err)
    assert err <= BAR, err


# ------------------------------------------------------------------ b. row passes --
def _rows(env, c, mode, axis, src, nrows, dst, row0=0, mroot=None, mcount=1.0):
    _, F, L, _ = env
    L.check(L.lib().rmt_selftest_dct2_rows(c.bind(), mode, axis, F._p(src), nrows, row0,
                                           F._p(mroot), mcount, 1.0 / c.nx, 1.0 / c.ny,
                                           F._p(dst)), "selftest_dct2_rows")


def _host_pass(mode, x):
    """mode 0: the unnormalised DCT-II 2 sum x cos of every row; mode 2: its inverse"""
    y = (dct if mode == 0 else idct)(x.astype(LD), type=2, axis=1)
    assert y.dtype == LD
    return y


# (context, axis, row counts): the rows of axis 0 are nx long, of axis 1 ny long.  (6, 46):
# odd row counts, the last row without a partner in its workgroup
ROW_CASES = [((6, 8190), 0, (6,)), ((1088, 6), 1, (6,)), ((6, 46), 0, (1, 3, 5)),
             ((5, 45), 0, (2, 5)), ((1155, 4), 1, (3,))]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape,axis,counts", ROW_CASES)
def test_row_pass(env, shape, axis, counts, mode):
    """Modes 0 and 2 of one pass against scipy's dct / idct (type 2, unnormalised) in long
    double; rows >= nrows of a dst filled with -7.0 stay as they were."""
    torch = env[0]
    ny, nx = shape
    n, rows = (nx, ny) if axis == 0 else (ny, nx)
    x = np.random.default_rng(31 * ny + nx + mode).standard_normal((rows, n))
    ref = _host_pass(mode, x)
    c = _ctx(env, ny, nx)
    src = torch.from_numpy(x).cuda()
    for nrows in counts:
        dst = torch.full_like(src, -7.0)
        _rows(env, c, mode, axis, src, nrows, dst)
        got = dst.cpu().numpy()
        err = _err(got[:nrows], ref[:nrows])
        print(shape, "axis", axis, "mode", mode, "nrows", nrows, err)
        assert err <= BAR, err
        assert (got[nrows:] == -7.0).all()


@pytest.mark.parametrize("row0", [0, 2, 40])
def test_row_pass_mode1_row0(env, row0):
    """Mode 1 (forward, / eig, inverse) on 6 rows that stand for the x-frequencies row0 ..
    row0 + 5 of a (126, 90) grid: row r is divided by lamx[row0 + r] + lamy[k], and only the
    (x-frequency 0, k = 0) entry is zeroed.  lamx, lamy: mac_lambda's formula (dct2.hip), which
    the plan made from (dx, dy) holds."""
    torch = env[0]
    ny, nx, nrows = 126, 90, 6
    dx, dy = 1.0 / nx, 1.0 / ny
    lamx = -2.0 * (1.0 - np.cos(np.pi * np.arange(nx) / nx)) / dx ** 2
    lamy = -2.0 * (1.0 - np.cos(np.pi * np.arange(ny) / ny)) / dy ** 2
    x = np.random.default_rng(row0).standard_normal((nrows, ny))
    lam = lamx[row0:row0 + nrows, None] + lamy[None, :]      # float64, as the kernel adds them
    pin = row0 == 0
    if pin:
        lam[0, 0] = 1.0
    h = _host_pass(0, x) / lam.astype(LD)
    if pin:
        h[0, 0] = 0
    ref = _host_pass(2, h)
    src = torch.from_numpy(x).cuda()
    dst = torch.full((nrows + 2, ny), -7.0, dtype=torch.float64, device="cuda")
    _rows(env, _ctx(env, ny, nx), 1, 1, src, nrows, dst, row0=row0)
    got = dst.cpu().numpy()
    err = _err(got[:nrows], ref)
    print("mode 1 row0", row0, err)
    assert err <= BAR, err
    assert (got[nrows:] == -7.0).all()


@pytest.mark.parametrize("shape", [(12, 18), (6, 1088)])
def test_row_pass_mean_on_load(env, shape):
    """mroot = [S], mcount = c: the pass transforms x - S / c.  One IEEE division and one
    subtraction per element, then the same kernel input as the pass without mroot on the
    host-prepared x - S / c: bit for bit equal."""
    torch = env[0]
    ny, nx = shape
    x = np.random.default_rng(nx).standard_normal((ny, nx))
    S, cnt = float(x.sum()) + 3.25, float(ny * nx)
    c = _ctx(env, ny, nx)
    root = torch.tensor([S], dtype=torch.float64, device="cuda")
    a = torch.empty((ny, nx), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    _rows(env, c, 0, 0, torch.from_numpy(x).cuda(), ny, a, mroot=root, mcount=cnt)
    _rows(env, c, 0, 0, torch.from_numpy(x - S / cnt).cuda(), ny, b)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.abs(b).min() > 0 and (a.view(np.uint64) == b.view(np.uint64)).all()
    assert _err(a, _host_pass(0, x - S / cnt)) <= BAR


# ------------------------------------------------------------------ c. projection --
@pytest.mark.parametrize("N", [30, 46, 90, 33])
def test_projection_mixed_radix(env, N):
    """mac.project against the oracle at mixed-radix N (the mean on load, k_mac_rhs_rows and
    the solve; 46: the 512-thread variant), test_mac_projection's bars.  The wall-normal faces
    are zero: otherwise the Neumann problem is inconsistent and the reference itself leaves a
    divergence of 0.27."""
    from oracle import mac_oracle as MO
    mac = env[3]
    dx = dy = 1.0 / N
    rng = np.random.default_rng(N)
    us = rng.standard_normal((N, N + 1)); vs = rng.standard_normal((N + 1, N))
    us[:, 0] = us[:, -1] = 0; vs[0] = vs[-1] = 0
    eig = mac.poisson_eigs_neumann(N, N, dx, dy)
    ru, rv, rphi = MO.project(us, vs, dx, dy, 1e-3, 1.0, eig)
    u, v, phi = mac.project(us, vs, dx, dy, 1e-3, 1.0, eig)
    sc = np.abs(rphi).max()
    div = np.abs(mac.divergence(u, v, dx, dy)).max()
    print(N, np.abs(phi - rphi).max() / sc, np.abs(u - ru).max(), np.abs(v - rv).max(), div)
    np.testing.assert_allclose(phi, rphi, rtol=0, atol=1e-12 * sc)
    np.testing.assert_allclose(u, ru, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-12)
    assert div < 1e-9


# ------------------------------------------------------------------ d. plan reuse --
def test_plan_reuse_after_custom_eigenvalues(env):
    """dct2_set_lambda overwrites the plan's eigenvalues and poisons its key; the next call
    with the library's own eigenvalues has to replan.  One context, three calls, each against
    its own long-double reference."""
    mac = env[3]
    ny, nx = 30, 36
    rhs, eig = _case(mac, ny, nx)
    lx, ly = mac._axis_eigs(eig)
    eig2 = 2.0 * lx[None, :] + 2.0 * ly[:, None]
    eig2[0, 0] = 1.0
    ref_own, ref_custom = _ref_solve(rhs, eig), _ref_solve(rhs, eig2)
    c = _ctx(env, ny, nx)
    p1 = _gpu_solve(env, c, rhs, 2.0 * lx, 2.0 * ly)
    p2 = _gpu_solve(env, c, rhs)                       # lamx = lamy = NULL, (1/36, 1/30)
    p3 = _gpu_solve(env, c, rhs, 2.0 * lx, 2.0 * ly)
    errs = _err(p1, ref_custom), _err(p2, ref_own), _err(p3, ref_custom)
    print("plan reuse", errs)
    assert max(errs) <= BAR, errs
    # the doubled eigenvalues halve the solution: call 2 did not keep them
    assert np.abs(p2 - p1).max() > 0.4 * np.abs(p2).max()


# ------------------------------------------------------------------ e. rejection --
@pytest.mark.parametrize("shape", [(29, 8), (8, 58), (8, 8194)])
def test_rejected_shapes(env, shape):
    """A prime factor > 23 (29; 58 = 2 29) and N > 8192 raise NotImplementedError
    (RMT_ENOTSUP).  dct2_plan tests factor() and lds_fits() of both axes before it
    allocates, uploads or launches anything, and rmt_mac_solve_poisson_neumann returns on its
    status, so no kernel runs: the output plane keeps its fill.  A process that met the
    refusal still solves a valid shape correctly."""
    torch, _, _, mac = env
    ny, nx = shape
    rhs = np.random.default_rng(1).standard_normal((ny, nx))
    out = torch.full((ny, nx), -7.0, dtype=torch.float64, device="cuda")
    c = _ctx(env, ny, nx)
    for _ in range(2):      # the refusal leaves the context without a plan: it refuses again
        with pytest.raises(NotImplementedError):
            _gpu_solve(env, c, rhs, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    rhs, eig = _case(mac, 10, 14)
    lx, ly = mac._axis_eigs(eig)
    assert _err(_gpu_solve(env, _ctx(env, 10, 14), rhs, lx, ly), _ref_solve(rhs, eig)) <= BAR
