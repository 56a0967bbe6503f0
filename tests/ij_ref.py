"""sbag.h's rule for sbag_predict_variance in NumPy, vectorised over the rows: every fp64
operation is one ufunc call, so each is rounded on its own."""
import numpy as np


def variance(pt, gram):
    """pt: per-tree predictions [T, N]; gram: int64 [T, T].  Returns (m, v_ij, v_iju, d)."""
    pt = np.asarray(pt, np.float64)
    T, N = pt.shape
    s = np.zeros(N)
    for b in range(T):
        s = s + pt[b]
    m = s / float(T)
    d = pt - m
    Gd = np.asarray(gram, np.int64).astype(np.float64)
    q, c = np.zeros(N), np.zeros(N)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(T):
            s = np.zeros(N)
            for b in range(a):
                s = s + Gd[a, b] * d[b]
            u = (s + s) + Gd[a, a] * d[a]
            q = q + d[a] * u
            c = c + d[a] * d[a]
        tt = float(T * T)
        tr = sum(int(gram[a][a]) for a in range(T))
        tot = tr + 2 * sum(int(gram[a][b]) for a in range(T) for b in range(a))
        w = float(tr) / float(T) - float(tot) / tt
        v_ij = q / tt
        return m, v_ij, v_ij - (w * c) / tt, d
