"""CPU: quantiles_ref.py (sbag.h's quantile rule) against np.quantile(method="linear").

Where (n - 1) * p is an integer both give an order statistic: equal bytes.  Elsewhere both
interpolate between the same two values with three roundings each, in different formulas
(NumPy: a lerp that switches form at g = 0.5), so they may differ by a few ulp of the larger
magnitude: the bound is 4 ulp of max |v|.  Seen on these inputs (normal values, 2 000 columns
a case): 2 ulp of max |v| at n = 2 and 3, at most 1 ulp from n = 63 to 129."""
import numpy as np
import pytest

import quantiles_ref as qr


@pytest.mark.parametrize("n", [1, 5, 9])
def test_order_statistics_are_exact(n):
    rng = np.random.default_rng(n)
    pt = rng.normal(size=(n, 300)) * 3
    pt[0, :7] = -0.0
    probs = [0.0, 0.25, 0.5, 1.0]
    got, cnt = qr.quantiles(pt, probs)
    assert (cnt == n).all()
    want = np.quantile(pt + 0.0, probs, axis=0, method="linear").T
    np.testing.assert_array_equal(got, want)
    assert not np.signbit(got[got == 0]).any()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 128, 129])
def test_interpolation_within_four_ulp(n):
    rng = np.random.default_rng(100 + n)
    pt = rng.normal(size=(n, 2000)) * rng.choice([1e-3, 1.0, 1e6], size=2000)
    probs = [0.0, 0.05, 0.25, 0.5, 0.9, 0.975, 1.0]
    got, _ = qr.quantiles(pt, probs)
    want = np.quantile(pt, probs, axis=0, method="linear").T
    ulp = np.spacing(np.abs(pt).max(axis=0))[:, None]
    worst = float((np.abs(got - want) / ulp).max())
    print(f"n = {n}: worst difference {worst} ulp of max |v|")
    assert worst <= 4


def test_masked_rows():
    """With counts: the values of the trees with count 0 only; n == 0 gives NaN."""
    rng = np.random.default_rng(5)
    pt = rng.normal(size=(9, 400))
    counts = rng.integers(0, 3, size=(9, 400)).astype(np.uint8)
    counts[:, :3] = 1
    counts[:, 3] = 0
    probs = [0.0, 0.3, 0.5, 1.0]
    got, n = qr.quantiles(pt, probs, counts)
    assert (n[:3] == 0).all() and np.isnan(got[:3]).all() and n[3] == 9
    for r in range(3, 400):
        v = pt[counts[:, r] == 0, r]
        assert n[r] == len(v)
        if len(v):
            want = np.quantile(v, probs, method="linear")
            assert (np.abs(got[r] - want) <= 4 * np.spacing(np.abs(v).max())).all()
            assert got[r, 0] == v.min() and got[r, 3] == v.max()
        else:
            assert np.isnan(got[r]).all()
