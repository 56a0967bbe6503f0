"""A plain NumPy restatement of transform, the reference of the hand-built-forest tests
(test_gpu_predict_forests.py); test_predict_ref_host.py holds it to oracle.predict bit for
bit, so it is no second opinion of our own making.

A tree is a pre-order node array (NODE_DTYPE: left / right child ids, -1 at a leaf;
`feature` indexes the tree's subspace) and a row goes left iff
x[sub[feature]] <= threshold: NaN compares false and goes right, -0.0 equals +0.0
(ml/tree/Node.scala, InternalNode.predictImpl through Split.shouldGoLeft)."""
import numpy as np


def walk(nodes, sub, X):
    """Leaf node id reached by every row of X (fp64 [N][F]) in one tree."""
    X = np.asarray(X, np.float64)
    left = nodes["left"].astype(np.int64)
    right = nodes["right"].astype(np.int64)
    thr = nodes["threshold"].astype(np.float64)
    sub = np.asarray(sub, np.int64)
    gfeat = sub[np.maximum(nodes["feature"], 0)] if sub.size else np.zeros(len(nodes), np.int64)
    idx = np.zeros(X.shape[0], np.int64)
    act = np.nonzero(left[idx] >= 0)[0]  # rows still at an internal node
    while act.size:
        i = idx[act]
        with np.errstate(invalid="ignore"):
            go_left = X[act, gfeat[i]] <= thr[i]
        idx[act] = np.where(go_left, left[i], right[i])
        act = act[left[idx[act]] >= 0]
    return idx


def per_tree(trees, subs, X):
    """Per-tree predictions fp64 [L][N]."""
    return np.stack([t["prediction"].astype(np.float64)[walk(t, s, X)] for t, s in zip(trees, subs)])


def seq_sum(pt):
    """The in-order fp64 sum over trees 0..L-1, one tree at a time (breeze's sum)."""
    s = np.zeros(pt.shape[1])
    for t in range(pt.shape[0]):
        s = s + pt[t]
    return s


def mean(pt):
    return seq_sum(pt) / float(pt.shape[0])


def mode(pt):
    """breeze.stats.mode of class ids: the class that first reaches the final maximum
    count, the trees taken in order."""
    L, N = pt.shape
    ids = pt.astype(np.int64)
    cnt = np.zeros((N, int(ids.max()) + 1), np.int64)
    maxc = np.zeros(N, np.int64)
    best = np.zeros(N, np.float64)
    rows = np.arange(N)
    for t in range(L):
        cnt[rows, ids[t]] += 1
        k = cnt[rows, ids[t]]
        up = k > maxc
        maxc = np.where(up, k, maxc)
        best = np.where(up, pt[t], best)
    return best
