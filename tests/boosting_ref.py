"""Restatement of the reference's Boosting estimators on top of the CPU oracle: the boosted
bag (ml/boosting/BoostingParams.scala:127-148) and the two training loops
(ml/classification/BoostingClassifier.scala, ml/regression/BoostingRegressor.scala), with no
call into the library under test.  The trees are oracle.fit's, the walks oracle.predict's;
exp / pow / log are numpy's, as in spark_bagging_amd/boosting.py (the JVM's are
StrictMath's: see that module's docstring).
"""
import numpy as np

import oracle

_DOUBLE_MAX = np.finfo(np.float64).max
DEFAULT_SEED_BOOSTING_CLASSIFIER = 779462656   # "org.apache.spark.ml.classification.BoostingClassifier".hashCode
DEFAULT_SEED_BOOSTING_REGRESSOR = -596032410   # "org.apache.spark.ml.regression.BoostingRegressor".hashCode


def wrap64(v):
    """A Python int as a JVM Long (two's-complement wrap)."""
    return ((int(v) + 2**63) % 2**64) - 2**63


def boosted_bag(mean, part_off, seed):
    """extractBoostedBag: row j of partition i with mean != 0.0 gets the first draw of a
    PoissonDistribution(mean) reseeded with seed + i + j (Long arithmetic); else 0."""
    mean = np.asarray(mean, np.float64)
    out = np.zeros(len(mean), np.uint8)
    for i in range(len(part_off) - 1):
        for j, r in enumerate(range(int(part_off[i]), int(part_off[i + 1]))):
            if mean[r] != 0.0:
                k = int(oracle.poisson(float(mean[r]), wrap64(seed + i + j), 1)[0])
                if k > 255:
                    raise ValueError("a Poisson draw exceeded 255")
                out[r] = k
    return out


def doubles_drawn(mean, count):
    """nextDouble() calls of PoissonDistribution.nextPoisson(mean) that returned `count`:
    count + 1 when the product fell below p, count when the loop bound n < 1000 * mean
    ended it; 0 for a mean of 0.0 (no draw)."""
    mean = np.asarray(mean, np.float64)
    count = np.asarray(count, np.int64)
    d = np.where(count.astype(np.float64) < 1000.0 * mean, count + 1, count)
    return np.where(mean == 0.0, 0, d)


def partition_sum(x, part_off):
    """SQL sum over a partitioned column: each partition's left-to-right fp64 sum, the
    partial sums merged in partition order (empty partitions contribute nothing)."""
    total = None
    for i in range(len(part_off) - 1):
        seg = np.asarray(x[int(part_off[i]):int(part_off[i + 1])], np.float64)
        if len(seg) == 0:
            continue
        s = float(np.cumsum(seg)[-1])
        total = s if total is None else total + s
    return 0.0 if total is None else total


def _split_parts(part_off, vmask):
    """Partition offsets of the training rows and of the validation rows after the
    validation filter (a filter keeps the partitioning)."""
    tr, va = [0], [0]
    for i in range(len(part_off) - 1):
        m = vmask[int(part_off[i]):int(part_off[i + 1])]
        tr.append(tr[-1] + int((~m).sum()))
        va.append(va[-1] + int(m.sum()))
    return tr, va


def _terminate(avgl, with_validation, error, verror, tol, num_round, num_try, it, num_classes=2.0):
    """BoostingParams.terminate / terminateVal -> (iter, error, numTry)."""
    if avgl > (num_classes - 1.0) / num_classes:
        return 0, 0.0, 1
    if avgl == 0.0:
        return 0, 0.0, 0
    if with_validation:
        if verror < error * (1 - tol):
            return it - 1, verror, 0
        if num_try == num_round - 1:
            return 0, 0.0, num_try + 1
        return it - 1, error, num_try + 1
    return it - 1, 0.0, 0


def _loss_fn(name):
    return {"exponential": lambda e: 1.0 - np.exp(-e), "squared": lambda e: np.power(e, 2),
            "absolute": lambda e: e}[name]


def _fit_tree(X, y, bag, sub, part, classification, tp):
    return oracle.fit(X, y, bag[None, :], [sub], max_depth=tp.get("max_depth", 5),
                      max_bins=tp.get("max_bins", 32),
                      min_instances_per_node=tp.get("min_instances_per_node", 1),
                      min_info_gain=tp.get("min_info_gain", 0.0), classification=classification,
                      part=part, dt_seed=tp.get("dt_seed"))


def weighted_mean(pt, weights):
    """BoostingRegressionModel.predict: BLAS.dot(preds, weights) / weights.sum, both as
    running sums in booster order."""
    acc = np.zeros(pt.shape[1])
    wsum = 0.0
    for p, w in zip(pt, weights):
        acc = acc + p * w
        wsum = wsum + w
    return acc / wsum


def raw_votes(pt, weights, num_classes):
    """BoostingClassificationModel.predictRaw: weight added to class ceil(pred), in booster
    order."""
    raw = np.zeros((pt.shape[1], num_classes))
    rows = np.arange(pt.shape[1])
    for p, w in zip(pt, weights):
        k = np.ceil(p).astype(np.int64)
        raw[rows, k] = raw[rows, k] + w
    return raw


def _per_tree(trees, subs, X, classification):
    L = len(trees)
    width = max(len(t[0]) for t in trees)
    nodes = np.zeros((L, width), oracle.NODE_DTYPE)
    for l, (n, _) in enumerate(trees):
        nodes[l, : len(n)] = n
    f = oracle.Forest(nodes, np.zeros((L, width, 3)), np.array([len(t[0]) for t in trees], np.int32),
                      np.full(L, 3, np.int32), [np.asarray(s, np.int32) for s in subs], np.ones(L, bool))
    return oracle.predict(f, X, classification=classification, per_tree=True)[1]


def boosting_fit(X, y, *, classification, num_base_learners=10, loss="exponential",
                 seed=None, tol=1e-3, num_round=5, part=None, validation=None, **tp):
    """BoostingClassifier.train (SAMME) / BoostingRegressor.train (AdaBoost.R2), one
    iteration per step of the reference's trainBoosters recursion.  Returns (weights, trees
    [(nodes, stats)], num_classes or None, iterations run)."""
    X = np.ascontiguousarray(X, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    if seed is None:
        seed = DEFAULT_SEED_BOOSTING_CLASSIFIER if classification else DEFAULT_SEED_BOOSTING_REGRESSOR
    part = [0, len(y)] if part is None else [int(p) for p in part]
    vmask = np.zeros(len(y), bool) if validation is None else np.asarray(validation, bool)
    with_validation = validation is not None
    ptr, pva = _split_parts(part, vmask)
    Xt, yt, Xv, yv = X[~vmask], y[~vmask], X[vmask], y[vmask]
    n, F = Xt.shape
    K = int(y.max()) + 1 if classification else None
    sub = np.arange(F, dtype=np.int32)
    lossf = _loss_fn(loss)
    w = np.ones(n)
    weights, trees = [], []
    it, error, num_try, s = num_base_learners, _DOUBLE_MAX, 0, seed
    while it != 0:
        proba = w / partition_sum(w, ptr)
        bag = boosted_bag(proba * float(n), ptr, s)
        f = _fit_tree(Xt, yt, bag, sub, ptr, classification, tp)
        pred = oracle.predict(f, Xt, classification=classification, per_tree=True)[1][0]
        if classification:
            ls = lossf(np.where(yt == pred, 0.0, 1.0))
        else:
            err = np.abs(yt - pred)
            max_error = float(err.max())
            ls = lossf(err / max_error) if max_error != 0.0 else np.zeros(n)  # x / 0 is NULL
        avgl = partition_sum(ls * proba, ptr)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            beta = float(np.float64(avgl) / ((np.float64(1) - avgl) * np.float64((K if classification else 2) - 1)))
            weight = 1.0 if beta == 0.0 else float(np.log(np.float64(1) / np.float64(beta)))
            w = w * np.power(np.float64(beta), 1 - ls)
        weights.append(weight)
        trees.append(f.tree(0))
        verror = _DOUBLE_MAX
        if len(yv):
            pt = _per_tree(trees, [sub] * len(trees), Xv, classification)
            with np.errstate(invalid="ignore", over="ignore"):
                vp = weighted_mean(pt, weights)
            if classification:
                verror = partition_sum(lossf(np.where(yv == vp, 0.0, 1.0)), pva)
            else:
                verror = partition_sum(lossf(np.abs(yv - vp)), pva)
        old = it
        it, error, num_try = _terminate(avgl, with_validation, error, verror, tol, num_round, num_try,
                                        it, float(K) if classification else 2.0)
        s = s + old
    keep = len(trees) - num_try
    return weights[:keep], trees[:keep], K, len(trees)


def boosting_predict(weights, trees, X, num_classes=None):
    """(prediction, raw or None) of the boosted model on X."""
    X = np.ascontiguousarray(X, np.float64)
    F = X.shape[1]
    pt = _per_tree(trees, [np.arange(F, dtype=np.int32)] * len(trees), X, num_classes is not None)
    if num_classes is None:
        return weighted_mean(pt, weights), None
    raw = raw_votes(pt, weights, num_classes)
    return np.argmax(raw, axis=1).astype(np.float64), raw
