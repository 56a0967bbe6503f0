"""A plain NumPy restatement of the per-class raw predictions (sbag_predict_raw and its
out-of-bag form), the reference of test_gpu_proba.py; test_proba_host.py holds it to the
oracle's per-tree predictions and leaf stats.

The rule, literally (include/sbag.h): the learner loop is outermost and a row's sums grow
one tree at a time, s = s + frac.
  VOTES  raw[r][c] = number of aggregated trees whose prediction for row r is class c
  LEAF   st = the class counts of the leaf row r reaches in tree t, total = st[0] + st[1] +
         ... left to right; if total != 0: s[c] = s[c] + st[c] / total for c < ns_t
With `counts` (bag multiplicities [L][N]) tree i is aggregated for row r iff
counts[i][r] == 0 and n_oob counts those trees."""
import numpy as np

import predict_ref

VOTES, LEAF = 0, 1


def leaf_fractions(st):
    """st [n][ns] class counts -> (fractions [n][ns], total != 0 [n]); the total is the
    left-to-right sum (cumsum adds in order; np.sum would add pairwise)."""
    st = np.asarray(st, np.float64)
    total = np.cumsum(st, axis=1)[:, -1] if st.shape[1] else np.zeros(len(st))
    ok = total != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = st / total[:, None]
    return frac, ok


def raw(trees, stats, subs, X, kind, C, counts=None):
    """raw fp64 [N][C]; with counts: (raw, n_oob int32 [N])."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    s = np.zeros((N, C), np.float64)
    n_oob = np.zeros(N, np.int32)
    rows = np.arange(N)
    for i, (nodes, sub) in enumerate(zip(trees, subs)):
        leaf = predict_ref.walk(nodes, sub, X)
        use = np.ones(N, bool) if counts is None else np.asarray(counts[i]) == 0
        n_oob += use
        if kind == VOTES:
            cls = nodes["prediction"][leaf].astype(np.int64)
            add = np.zeros((N, C), np.float64)
            add[rows[use], cls[use]] = 1.0
            s = s + add  # + 0.0 elsewhere: no bit changes (s is never -0.0)
            continue
        frac, ok = leaf_fractions(np.asarray(stats[i], np.float64)[leaf])
        ns = frac.shape[1]
        upd = use & ok
        s[upd, :ns] = s[upd, :ns] + frac[upd]
    return s if counts is None else (s, n_oob)
