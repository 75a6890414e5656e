"""tools/dct_sym_model.py -- the index maps of k_dct1s (even-symmetric prime-factor DCT-I on
half the row) -- against scipy's DCT-I.  CPU only."""
import os
import sys

import numpy as np
import pytest
from scipy.fft import dct

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import dct_sym_model as M  # noqa: E402


@pytest.mark.parametrize("n", [16, 36, 46, 64, 92, 196, 586, 4096])
def test_model_matches_scipy(n):
    """Bar 1e-14 (the model rounds at a few 1e-16; this guards the index maps, where a wrong
    entry costs O(1)).  The model itself asserts every slot is written once per pass."""
    x = np.random.default_rng(n).standard_normal(n)
    ref = dct(x, type=1)
    err = np.abs(M.dct1_sym(x) - ref).max() / np.abs(ref).max()
    print(n, M.radices(n - 1), err)
    assert err <= 1e-14, err


def test_model_pass_order_free():
    """Any pass order is exact (the kernel fixes one because the bits depend on it)."""
    x = np.random.default_rng(5).standard_normal(4096)
    ref = dct(x, type=1)
    for rad in ([13, 9, 7, 5], [5, 7, 9, 13]):
        assert np.abs(M.dct1_sym(x, rad) - ref).max() / np.abs(ref).max() <= 1e-14


def test_eligibility():
    assert M.radices(4095) == [13, 9, 7, 5] and M.radices(195) == [13, 5, 3]
    for N in (27, 25, 1023, 299, 4094, 49):   # repeated factor, 31, 23, even
        assert M.radices(N) is None
