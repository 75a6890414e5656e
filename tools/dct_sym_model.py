"""CPU model of k_dct1s (pyrmt_amd/csrc/dct1.hip): the DCT-I of a real row of length n,
N = n - 1 odd with pairwise coprime radices, as ONE even complex length-N DFT held on half
its indices.  The index maps here are the kernel's.

    python tools/dct_sym_model.py        # relative error against scipy at a few sizes
"""
import numpy as np

RADICES = (13, 11, 9, 7, 5, 3)


def radices(N):
    """Pairwise coprime radices of N (descending: the kernel's pass order), or None."""
    out = []
    for R in RADICES:
        if N % R == 0 and not (R == 3 and out and 9 in out):
            out.append(R)
            N //= R
    return out if N == 1 and out else None


def readout_table(N, rad):
    """slot(sigma(k)), k = 0 .. (N - 1) / 2: where C at frequency k (N + 1) / 2 ends up."""
    k2 = np.arange((N + 1) // 2) * ((N + 1) // 2) % N
    sig = sum((k2 % R) * (N // R) for R in rad) % N
    return np.minimum(sig, N - sig)


def dct1_sym(x, rad=None):
    n = len(x); N = n - 1; H = (N - 1) // 2
    rad = rad or radices(N)
    slot = lambda i: np.minimum(i, N - i)
    m = np.arange(H + 1)
    # c = a + i b, a / b the even- / odd-index halves of the even extension, indexed mod N
    z = np.where(m % 2 == 0, x[m] + 1j * x[N - m], x[N - m] + 1j * x[m])
    for R in rad:
        s = N // R
        q = np.arange((s + 1) // 2)[:, None]               # line s - q mirrors line q
        idx = (R * q + np.arange(R) * s) % N
        v = z[slot(idx)] @ np.exp(-2j * np.pi * (np.outer(np.arange(R), np.arange(R)) % R) / R)
        keep = np.ones(idx.shape, bool); keep[0, (R + 1) // 2:] = False   # line 0: own mirror
        assert sorted(slot(idx[keep])) == list(range(H + 1))   # every slot written once
        z = np.empty_like(z); z[slot(idx[keep])] = v[keep]
    C = z[readout_table(N, rad)]
    sg = 1 - 2 * (m % 2)
    X = np.empty(n)
    X[m] = C.real + sg * C.imag
    X[N - m] = C.real - sg * C.imag
    return X


if __name__ == "__main__":
    from scipy.fft import dct
    rng = np.random.default_rng(0)
    for n in (16, 36, 46, 64, 92, 196, 586, 4096):
        x = rng.standard_normal(n); ref = dct(x, type=1)
        print(n, radices(n - 1), np.abs(dct1_sym(x) - ref).max() / np.abs(ref).max())
