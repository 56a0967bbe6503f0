"""sbag.h's quantile rule in NumPy, the reference of test_gpu_quantiles.py (held to
np.quantile by test_quantiles_host.py).

Row r: the predictions of the trees concerned (all, or those with counts[i][r] == 0), -0.0 read
as +0.0, sorted ascending: v[0, n).  h = (double)(n - 1) * p, lo = floor(h), g = h - lo;
out = v[lo] when g == 0, else v[lo] + g * (v[lo + 1] - v[lo]), each operation rounded on its
own (NumPy's fp64 arithmetic does); NaN where n == 0."""
import numpy as np


def quantiles(pt, probs, counts=None):
    """pt fp64 [L][N] per-tree predictions, counts [L][N] or None -> (fp64 [N][Q], n int32 [N])."""
    pt = np.asarray(pt, np.float64) + 0.0  # -0.0 + 0.0 is +0.0
    L, N = pt.shape
    probs = np.asarray(probs, np.float64).reshape(-1)
    if counts is not None:
        pt = np.where(np.asarray(counts) == 0, pt, np.inf)  # in bag: sorts last, never selected
    v = np.sort(pt, axis=0)
    n = np.full(N, L, np.int32) if counts is None else (np.asarray(counts) == 0).sum(axis=0).astype(np.int32)
    out = np.full((N, len(probs)), np.nan)
    rows = np.arange(N)
    some = n > 0
    for q, p in enumerate(probs):
        h = (n - 1).astype(np.float64) * p
        fl = np.floor(h)
        g = h - fl
        lo = np.where(some, fl, 0).astype(np.int64)
        hi = np.minimum(lo + 1, np.maximum(n - 1, 0))
        v0, v1 = v[lo, rows], v[hi, rows]
        with np.errstate(invalid="ignore"):
            mid = v0 + g * (v1 - v0)
        out[:, q] = np.where(some, np.where(g == 0, v0, mid), np.nan)
    return out, n
