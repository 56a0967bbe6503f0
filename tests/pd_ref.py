"""A plain NumPy restatement of sbag_partial_dependence's rule (sbag.h), the reference of
test_gpu_pd.py; test_pd_host.py pins it on a forest worked by hand.

cnt[t][l][g]: the rows that tree t sends to its leaf l (leaves counted in node, i.e. pre-order,
order) when column `feature` of X is overwritten with grid[g].  Then
  mean   tree_pd[t][g] = s / N, s = 0.0, s = s + cnt[t][l][g] * value_l for l in order;
         pd[g] = (in-order sum of tree_pd[t][g]) / L, or with weights the in-order sum of
         tree_pd[t][g] * weights[t]
  votes  pd[g][c] = (sum over t and the leaves that predict c of cnt[t][l][g]) / (N * L)"""
import numpy as np

import predict_ref as ref


def counts(trees, subs, X, feature, grid):
    """[(leaf values fp64 [leaves], cnt int64 [leaves][G])] per tree."""
    X = np.array(X, np.float64)
    out = []
    for t, s in zip(trees, subs):
        leaf_ids = np.nonzero(t["left"] < 0)[0]
        ordinal = np.cumsum(t["left"] < 0) - 1
        cnt = np.zeros((len(leaf_ids), len(grid)), np.int64)
        for g, v in enumerate(grid):
            X[:, feature] = v
            cnt[:, g] = np.bincount(ordinal[ref.walk(t, s, X)], minlength=len(leaf_ids))
        out.append((t["prediction"][leaf_ids].astype(np.float64), cnt))
    return out


def mean(trees, subs, X, feature, grid, weights=None):
    """(pd fp64 [G], tree_pd fp64 [L][G])."""
    N, L = float(len(X)), len(trees)
    tree_pd = np.zeros((L, len(grid)))
    for t, (val, cnt) in enumerate(counts(trees, subs, X, feature, grid)):
        s = np.zeros(len(grid))
        for l in range(len(val)):
            s = s + cnt[l].astype(np.float64) * val[l]
        tree_pd[t] = s / N
    pd = np.zeros(len(grid))
    for t in range(L):
        pd = pd + (tree_pd[t] if weights is None else tree_pd[t] * np.float64(weights[t]))
    return (pd / float(L) if weights is None else pd), tree_pd


def votes(trees, subs, X, feature, grid, num_classes):
    """pd fp64 [G][num_classes]."""
    v = np.zeros((len(grid), num_classes), np.int64)
    for val, cnt in counts(trees, subs, X, feature, grid):
        for l in range(len(val)):
            v[:, int(val[l])] += cnt[l]
    return v.astype(np.float64) / (float(len(X)) * float(len(trees)))
