"""sha256 of the FFT-based Poisson solves, one line per case (compare two libraries: every
kernel of dct1.hip and dct2.hip that dct_pass / dct2_pass can launch, the rocFFT fallback,
the periodic solve and the IMEX DST preconditioner).
    RMT_LIB=... python tools/dct_sha.py"""
import hashlib
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyrmt_amd import functions as F, _lib as L, mac as M


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def ctx(ny, nx, sym=1):
    c = F._Ctx(ny, nx, torch.cuda.current_device())
    c.set_option("dct_sym", sym)
    return c


def dct1_solve(ny, nx, sym=1):
    rhs = torch.from_numpy(np.random.default_rng(ny * 7 + nx).standard_normal((ny, nx))).cuda()
    out = torch.empty_like(rhs)
    c = ctx(ny, nx, sym)   # (held to the end of the call: a _Ctx destroys its context when dropped)
    L.check(L.lib().rmt_solve_poisson_dct(c.bind(), F._p(rhs), 1.0 / (nx - 1), 1.0 / (ny - 1),
                                          F._p(out)), "solve")
    return sha(out.cpu().numpy())


def dct1_rows(ny, nx, marks):
    """one row pass (rmt_selftest_dct_rows): with its row sums, or on the marked rows only"""
    src = torch.from_numpy(np.random.default_rng(nx).standard_normal((ny, nx))).cuda()
    dst = torch.full_like(src, -7.0)
    rs = rs_ref = mark = None
    if marks:
        m = np.zeros(ny, np.uint8); m[[0, ny // 2, ny - 1]] = 1
        mark = torch.from_numpy(m).cuda()
    else:
        rs = torch.zeros(ny, dtype=torch.float64, device="cuda")
        rs_ref = torch.zeros_like(rs)
    c = ctx(ny, nx)
    L.check(L.lib().rmt_selftest_dct_rows(c.bind(), F._p(src), 1.0 / (nx - 1), 1.0 / (ny - 1),
                                          1.0 / (2.0 * (nx - 1)), F._p(dst), F._p(rs),
                                          F._p(rs_ref), F._p(mark), 0), "dct_rows")
    return sha(dst.cpu().numpy(), *([] if marks else [rs.cpu().numpy()]))


def dct2_solve(N):
    rhs = np.random.default_rng(N).standard_normal((N, N))
    return sha(M.solve_poisson_neumann(rhs, M.poisson_eigs_neumann(N, N, 1.0 / N, 1.0 / N)))


def periodic_solve(N):
    h = 1.0 / (N - 1)
    rhs = np.random.default_rng(N).standard_normal((N, N))
    return sha(F._solve_poisson_fft(rhs, F._precompute_poisson_eigenvalues_periodic(N, N, h, h)))


def imex_pcg(N):
    """tests/test_gpu_imex.py::test_pcg_vs_oracle_sizes, the u faces"""
    dx = dy = 1.0 / N   # (the names mac._helmholtz_operator reads from the lambda's closure)
    rhs = np.random.default_rng(N).standard_normal((N, N - 1))
    return sha(M._pcg_helmholtz(rhs, lambda w: M._lap_u_lid_hom(w, dx, dy),
                                lambda x: np.pad(x, ((0, 0), (1, 1))), 2.0e-5, dx, dy, rtol=1e-8))


CASES = [(f"dct1 solve {s}", dct1_solve, s) for s in
         [(65, 65), (256, 256), (32, 32), (196, 196), (36, 257), (16, 3466), (8, 4096),
          (130, 200)]]
CASES += [("dct1 solve (8, 4096) dct_sym=0", dct1_solve, (8, 4096, 0))]
CASES += [(f"dct1 rows {s} {'marks' if m else 'sums'}", dct1_rows, s + (m,))
          for s in [(5, 4096), (23, 196)] for m in (False, True)]
CASES += [(f"dct2 solve {N}", dct2_solve, (N,)) for N in (64, 46, 8192)]
CASES += [("periodic solve 64", periodic_solve, (64,)), ("imex pcg 64", imex_pcg, (64,))]
for name, fn, args in CASES:
    print(f"{name:34s} {fn(*args)}", flush=True)
