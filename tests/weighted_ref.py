"""A plain NumPy restatement of sbag_predict_weighted's two rules, the reference of
test_gpu_weighted.py, built on predict_ref.walk; test_weighted_ref_host.py holds it to
oracle.gbm_predict, oracle.gbm_classifier_predict and boosting_ref.boosting_predict bit for
bit, so it is no second opinion of our own making.

  dot    out[r][c] = 0.0; for every tree t in order with t % num_cols == c:
         out[r][c] = out[r][c] + (tree_t(r) * weights[t]), the product rounded to fp64 first
  cls    out[r][c] = 0.0; for every tree t in order: out[r][k] = out[r][k] + weights[t] with
         k the class tree_t(r) predicts

It also carries the small forest builders and the planner's formulas of
test_gpu_predict_forests.py, restated (that module is a GPU test file and is not imported)."""
import numpy as np

import predict_ref as ref

NODE_DTYPE = np.dtype([("id", "<i4"), ("left", "<i4"), ("right", "<i4"), ("feature", "<i4"),
                       ("split_bin", "<i4"), ("pad", "<i4"), ("threshold", "<f8"),
                       ("prediction", "<f8"), ("impurity", "<f8"), ("gain", "<f8")])

K_PRED_ROWS = 512                  # the tile of the fused passes (kPredRows / kWpRows)
LDS_CAP = 160 * 1024 - 512         # plan_tiled's lds_cap


# ---------------------------------------------------------------- the two rules
def dot(pt, weights, num_cols=1):
    """pt fp64 [L][N] per-tree predictions -> fp64 [N][num_cols]."""
    L, N = pt.shape
    assert L % num_cols == 0 and len(weights) == L
    out = np.zeros((N, num_cols))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(L):
            c = t % num_cols
            out[:, c] = out[:, c] + pt[t] * np.float64(weights[t])
    return out


def cls(pt, weights, num_cols):
    """pt fp64 [L][N] class ids -> fp64 [N][num_cols]."""
    L, N = pt.shape
    assert len(weights) == L
    out = np.zeros((N, num_cols))
    rows = np.arange(N)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(L):
            k = pt[t].astype(np.int64)
            out[rows, k] = out[rows, k] + np.float64(weights[t])
    return out


def dot_forest(trees, subs, X, weights, num_cols=1):
    return dot(ref.per_tree(trees, subs, X), weights, num_cols)


def cls_forest(trees, subs, X, weights, num_cols):
    return cls(ref.per_tree(trees, subs, X), weights, num_cols)


# ---------------------------------------------------------------- the planner's formulas
def tiled_budget(S, code_bytes, mode_classes=0):
    """plan_tiled's chunk budget for rows of S codes beside mode_classes * 1024 bytes of
    accumulators (None: it refuses).  A column of 512 fp64 sums is 4096 bytes: four
    `mode_classes`."""
    fixed = K_PRED_ROWS * (S * code_bytes + 4)
    fixed = ((fixed + 15) & ~15) + mode_classes * K_PRED_ROWS * 2
    if fixed + 4096 > LDS_CAP:
        return None
    return min(64 * 1024, LDS_CAP - fixed) & ~15


def weighted_budget(S, code_bytes, num_cols):
    """The chunk budget of the fused weighted pass with num_cols accumulator columns."""
    return tiled_budget(S, code_bytes, 4 * num_cols)


def max_tiled_cols(S, code_bytes):
    """The largest num_cols the fused weighted pass holds beside rows of S codes."""
    return max(c for c in range(1, 64) if weighted_budget(S, code_bytes, c) is not None)


def tree_bytes(n_internal):
    return (2 * n_internal + 1) * 8 + (n_internal + 1) * 8


def host_stride(F):
    return (F + 15) // 16 * 16     # the u16 codes of host rows


def plan_chunks(sizes, budget):
    """plan_tiled's greedy chunking of trees of `sizes` bytes: [(t0, t1)]."""
    chunks, used = [], 0
    for t, b in enumerate(sizes):
        assert b <= budget
        if not chunks or used + b > budget:
            chunks.append([t, t])
            used = 0
        chunks[-1][1] = t + 1
        used += b
    return [tuple(c) for c in chunks]


# ---------------------------------------------------------------- forests
def _blank(n):
    a = np.zeros(n, NODE_DTYPE)
    a["id"] = np.arange(n)
    a["left"] = a["right"] = a["feature"] = -1
    return a


def leaf(v):
    a = _blank(1)
    a["prediction"] = v
    return a


def stump(thr, lv, rv, feature=0):
    a = _blank(3)
    a["left"][0], a["right"][0], a["feature"][0], a["threshold"][0] = 1, 2, feature, thr
    a["prediction"][1], a["prediction"][2] = lv, rv
    return a


def comb(thr, leaves, feature=0, left_deep=False):
    """n = len(thr) internal nodes in one chain, pre-order ids.  Right-deep: node 2i has
    leaf 2i + 1 on the left and node 2i + 2 on the right; left-deep: node i has node i + 1
    on the left and leaf 2n - i on the right.  leaves[k] is the leaf internal node k hangs
    off the chain, leaves[n] the leaf at its end."""
    thr = np.asarray(thr, np.float64)
    n = len(thr)
    a = _blank(2 * n + 1)
    if left_deep:
        i = np.arange(n)
        a["left"][i], a["right"][i] = i + 1, 2 * n - i
        ids = np.concatenate([2 * n - i, [n]])
    else:
        i = 2 * np.arange(n)
        a["left"][i], a["right"][i] = i + 1, i + 2
        ids = np.concatenate([i + 1, [2 * n]])
    a["feature"][i] = feature
    a["threshold"][i] = thr
    a["prediction"][ids] = leaves
    return a


def n_internal(tree):
    return int((tree["left"] >= 0).sum())
