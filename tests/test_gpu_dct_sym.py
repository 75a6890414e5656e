"""k_dct1s (pyrmt_amd/csrc/dct1.hip, switch dct_sym): the DCT-I of an axis whose n - 1 is
odd with pairwise coprime radices 3 .. 13, as one even complex prime-factor DFT on half the
row.  The solve against the oracle's pocketfft solve with the switch on and off, and the
row pass's own row sums and row marks (rmt_selftest_dct_rows)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# n - 1 = 15, 35, 45, 63, 91, 195, 585: radix sets {5,3} {7,5} {9,5} {9,7} {13,7} {13,5,3}
# {13,9,5}, one line per thread at the most
SQUARE = [(n, n) for n in (16, 36, 46, 64, 92, 196, 586)]
# one eligible axis beside one on k_dct1 (48 = 6 8, 256 = 4 8 8), either way round; two
# eligible axes of different plans; 3465 = 11 9 7 5: the radix 11, four passes, and the
# generic kernel's second line per thread (347 lines in the radix-5 pass, 256 threads)
MIXED = [(49, 36), (36, 257), (92, 586), (16, 3466)]


def _ctx(F, ny, nx, sym):
    import torch
    c = F._Ctx(ny, nx, torch.cuda.current_device())
    c.set_option("dct_sym", sym)
    return c


@pytest.mark.parametrize("sym", [1, 0])
@pytest.mark.parametrize("shape", SQUARE + MIXED)
def test_solve_against_pocketfft(gpu, oracle, shape, sym):
    """|p - p_ref| <= 1e-13 max|p_ref| (the project's bar between FFT roundings)."""
    import torch
    from pyrmt_amd import functions as F, _lib as L
    ny, nx = shape
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    rhs = np.random.default_rng(ny * 7 + nx).standard_normal((ny, nx))
    ref = oracle._solve_poisson_dct(rhs, oracle._precompute_poisson_eigenvalues(nx, ny, dx, dy))
    c = _ctx(F, ny, nx, sym)
    r = torch.from_numpy(rhs).cuda()
    out = torch.empty_like(r)
    L.check(L.lib().rmt_solve_poisson_dct(c.bind(), F._p(r), dx, dy, F._p(out)), "solve")
    err = np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(shape, sym, err)
    assert err <= 1e-13, err


def _rows(F, L, c, src, scale, dst, rs=None, rs_ref=None, mark=None, unmarked=0):
    ny, nx = src.shape
    L.check(L.lib().rmt_selftest_dct_rows(c.bind(), F._p(src), 1.0 / (nx - 1), 1.0 / (ny - 1),
                                          scale, F._p(dst), F._p(rs), F._p(rs_ref), F._p(mark),
                                          unmarked), "selftest_dct_rows")


@pytest.mark.parametrize("shape", [(37, 196), (5, 4096)])
def test_row_sums_bitwise(gpu, shape):
    """The row sums the pass takes itself are bit for bit k_rowsum's of the plane it wrote
    (the pressure mean is built from them), and the rows are the DCT-I (scipy, 1e-13)."""
    import torch
    from scipy.fft import dct
    from pyrmt_amd import functions as F, _lib as L
    ny, nx = shape
    x = np.random.default_rng(nx).standard_normal((ny, nx))
    c = _ctx(F, ny, nx, 1)
    src = torch.from_numpy(x).cuda()
    dst = torch.empty_like(src)
    rs = torch.zeros(ny, dtype=torch.float64, device="cuda")
    rs_ref = torch.zeros_like(rs)
    scale = 1.0 / (2.0 * (nx - 1))
    _rows(F, L, c, src, scale, dst, rs, rs_ref)
    a, b = rs.cpu().numpy(), rs_ref.cpu().numpy()
    assert np.abs(b).min() > 0 and (a.view(np.uint64) == b.view(np.uint64)).all()
    ref = dct(x, type=1, axis=1) * scale
    assert np.abs(dst.cpu().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("unmarked", [0, 1])
def test_row_marks(gpu, unmarked):
    """With a row mark the pass transforms only the marked rows (unmarked: only the others),
    to the same bits as the unmarked pass, and leaves the other rows of dst as they were."""
    import torch
    from pyrmt_amd import functions as F, _lib as L
    ny, nx = 23, 196
    x = np.random.default_rng(3).standard_normal((ny, nx))
    c = _ctx(F, ny, nx, 1)
    src = torch.from_numpy(x).cuda()
    full = torch.empty_like(src)
    _rows(F, L, c, src, 1.0, full)
    m = np.zeros(ny, np.uint8); m[[0, 4, 5, 22]] = 1
    mark = torch.from_numpy(m).cuda()
    dst = torch.full_like(src, -7.0)
    _rows(F, L, c, src, 1.0, dst, mark=mark, unmarked=unmarked)
    done = (m != 0) != bool(unmarked)
    got, want = dst.cpu().numpy(), full.cpu().numpy()
    assert (got[done].view(np.uint64) == want[done].view(np.uint64)).all()
    assert (got[~done] == -7.0).all()
