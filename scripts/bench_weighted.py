#!/usr/bin/env python3
"""The boosted models' transform: the fused weighted pass (sbag_predict_weighted /
sbag_predict_weighted_dataset, k_wpred_tiled) against the composed path the models ran before
it, in one run:

  fused dataset   nat.predict_weighted_dataset over the resident rows: one kernel, the
                  N x num_cols fp64 result on the host
  fused host      nat.predict_weighted over host rows: upload in row batches, k_quantize,
                  the same kernel
  composed        what GBMRegressionModel.transform / GBMClassificationModel.raw_sums did:
                  nat.predict(per_tree=True) over host rows (k_predict, the [trees x N] fp64
                  matrix to the host) plus the host loop of `trees` NumPy passes; from a
                  DeviceDataset the models first took dataset.features(), timed apart
                  (features_ms).  COMPOSED_ROWS (default ROWS) rows: lower it where the
                  [trees x N] matrix does not fit; the JSON line says which N each side ran at.

Shapes (SHAPES=reg,cls): `reg` 64 depth-5 boosters of a squared-loss GBM loop at learning
rate 0.5, num_cols = 1; `cls` 20 iterations x 5 classes of the GBMClassifier loop (one
booster per class on 1{label == k} - softmax_k), num_cols = 5.  Rows: sbag_dataset_synthetic
ROWS x 100 (default 10M).  One warm-up of every path, then REPS timed repeats (COMPOSED_REPS
of the composed path), host clock around calls that end with their results on the host.
Prints one JSON line per shape.  Kernel (device) times are not taken here: run the script
under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (the fused calls only, after the
warm-up) and read k_wpred_tiled there."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
NCMP = min(N, int(os.environ.get("COMPOSED_ROWS", N)))
F = 100
DEPTH = int(os.environ.get("DEPTH", 5))
REPS = max(3, int(os.environ.get("REPS", 5)))
COMPOSED_REPS = max(1, int(os.environ.get("COMPOSED_REPS", 2)))
SHAPES = os.environ.get("SHAPES", "reg,cls").split(",")
PROFILE = os.environ.get("PROFILE", "0") == "1"

ctx = nat.Context(0)
sub = np.arange(F, dtype=np.int32)


def fit_reg(ds, L):
    """GBMRegressor.train's loop, squared loss, learning rate 0.5, on real-valued labels."""
    y = ds.labels() * 1.1 + 0.3
    counts = nat.sample(ctx, True, 1.0, 1234, 0, L, N, None)
    res, trees = y.copy(), []
    for m in range(L):
        f = nat.fit_booster(ctx, ds, res, counts[m], sub, max_depth=DEPTH, max_bins=32)
        trees.append(f.tree(0)[0])
        res = res - 0.5 * nat.predict_dataset(ctx, f, ds, nat.AGG_MEAN)
        f.free()
    return trees, [0.5] * L


def fit_cls(ds, M, K):
    """GBMClassifier.train's loop: per iteration one booster per class on 1{y == k} - p_k."""
    y = ds.labels()
    counts = nat.sample(ctx, True, 1.0, 1234, 0, M, N, None)
    res, trees = np.zeros((N, K)), []
    for m in range(M):
        e = np.exp(res - res.max(axis=1, keepdims=True))
        prob = e / e.sum(axis=1, keepdims=True)
        for k in range(K):
            f = nat.fit_booster(ctx, ds, (y == k) - prob[:, k], counts[m], sub, max_depth=DEPTH, max_bins=32)
            trees.append(f.tree(0)[0])
            res[:, k] += 0.5 * nat.predict_dataset(ctx, f, ds, nat.AGG_MEAN)
            f.free()
        print(f"# cls iteration {m + 1} / {M} fitted", file=sys.stderr, flush=True)
    return trees, [0.5] * (M * K)


def composed(forest, X, w, nc):
    """The parent models' transform path, to the letter."""
    _, pt = nat.predict(ctx, forest, X, nat.AGG_MEAN, per_tree=True)
    if nc == 1:
        s = np.zeros(X.shape[0])
        for p, wt in zip(pt, w):
            s = s + p * wt
        return s[:, None]
    res = np.zeros((X.shape[0], nc))
    for m in range(len(w) // nc):
        for k in range(nc):
            res[:, k] = res[:, k] + pt[m * nc + k] * w[m * nc + k]
    return res


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def run(shape):
    nc = 1 if shape == "reg" else 5
    ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=0 if shape == "reg" else nc, ctx=ctx)
    t_fit, (trees, w) = timed(lambda: fit_reg(ds, 64) if shape == "reg" else fit_cls(ds, 20, nc))
    forest = nat.NativeForest.from_trees(trees, [sub] * len(trees), nat.IMPURITY_VARIANCE)
    fused_ds = lambda: nat.predict_weighted_dataset(ctx, forest, ds, nat.W_DOT, w, nc)  # noqa: E731
    out = fused_ds()  # warm-up
    if PROFILE:
        fused_ds()
        X = ds.features(0, min(N, 2_000_000))
        nat.predict_weighted(ctx, forest, X, nat.W_DOT, w, nc)
        print(json.dumps({"shape": shape, "rows": N, "trees": len(trees), "num_cols": nc, "profile_run": True,
                          "host_rows": len(X)}), flush=True)
    else:
        t_feat, X = timed(lambda: ds.features())
        fused_host = lambda: nat.predict_weighted(ctx, forest, X, nat.W_DOT, w, nc)  # noqa: E731
        same_host = bool(np.array_equal(fused_host(), out))
        Xc = X[:NCMP]
        t_c, base = [], None
        for r in range(COMPOSED_REPS + 1):  # the first is the warm-up
            t, base = timed(lambda: composed(forest, Xc, w, nc))
            if r:
                t_c.append(t)
            print(f"# {shape}: composed pass {r} took {t:.0f} ms", file=sys.stderr, flush=True)
        same = bool(np.array_equal(base, out[:NCMP]))
        del base
        t_d, t_h = [], []
        for r in range(REPS):
            t_d.append(timed(fused_ds)[0])
            t_h.append(timed(fused_host)[0])
        print(json.dumps({"shape": shape, "rows": N, "features": F, "trees": len(trees), "depth": DEPTH,
                          "num_cols": nc, "nodes": int(sum(len(t) for t in trees)), "fit_s": round(t_fit / 1e3, 1),
                          "fused_dataset": spread(t_d), "fused_host_rows": spread(t_h),
                          "composed": dict(spread(t_c), rows=NCMP, per_tree_bytes=8 * len(trees) * NCMP),
                          "features_ms": round(t_feat, 1), "result_bytes": 8 * N * nc,
                          "fused_equals_composed": same, "host_rows_equal_dataset": same_host}), flush=True)
    forest.free()
    ds.free()


for s in SHAPES:
    run(s)
ctx.close()
