"""GPU: sbag_fit_bag (one tree on a given bag, the dataset's own labels, gini or variance)
against the oracle's tree on the same bag, node by node and stat by stat.

The bags are shaped like a boosting iteration's after the weights have concentrated
(BoostingParams.extractBoostedBag): most rows absent, a few drawn 40-60 times, one at the u8
column's limit -- counts no bagging sampler at ratio <= 1 produces.
"""
import numpy as np
import pytest

import oracle
from parity_utils import assert_forest_equal

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

N, F, DEPTH = 3000, 6, 4
PART = [0, 1100, 1101, N]
SUB = np.array([0, 2, 3, 5], np.int32)


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def features(n, seed=5):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, F)) * 6) / 4
    X[rng.random((n, F)) < 0.15] = 0.0
    X[:, 5] = rng.integers(0, 3, n)
    return X


def labels(kind, X, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "gini":
        return ((np.floor(np.abs(X[:, 0]) * 2) + (X[:, 3] > 0) + rng.integers(0, 2, len(X))) % 4).astype(np.float64)
    y = np.round(X[:, 0] * 8 - X[:, 2] * 4) / 8 + rng.integers(-8, 9, len(X)) / 16.0
    return y if kind == "dyadic" else y * 1.1 + 0.3 + rng.normal(size=len(X)) / 7


def boosted_style_bag(n, seed=3, scale=1.0):
    """~70 % zeros, small counts, a few of 40-60 and one 255."""
    rng = np.random.default_rng(seed)
    c = rng.poisson(0.4 * scale, n)
    c[rng.random(n) < 0.5] = 0
    heavy = rng.choice(n, 12, replace=False)
    c[heavy] = rng.integers(40, 61, len(heavy))
    c[heavy[0]] = 255
    return c.astype(np.uint8)


def fit_both(ctx, X, y, bag, sub, part, gini, depth=DEPTH, bins=32):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = nat.fit_bag(ctx, ds, bag, sub, impurity=nat.IMPURITY_GINI if gini else nat.IMPURITY_VARIANCE,
                        partition_offsets=part, max_depth=depth, max_bins=bins)
        raw = nat.predict_raw_dataset(ctx, f, ds, nat.RAW_LEAF) if gini else None
    finally:
        ds.free()
    orf = oracle.fit(X, y, bag[None, :], [sub], max_depth=depth, max_bins=bins, classification=gini,
                     part=part)
    assert_forest_equal(f, orf)
    return f, orf, raw


@pytest.mark.parametrize("kind", ["gini", "dyadic", "real"])
def test_fit_bag_matches_oracle(ctx, kind):
    X = features(N)
    y = labels(kind, X)
    bag = boosted_style_bag(N)
    assert (bag == 0).mean() > 0.6 and ((bag >= 40) & (bag <= 60)).sum() >= 3 and bag.max() == 255
    f, orf, raw = fit_both(ctx, X, y, bag, SUB, PART, kind == "gini")
    assert len(f) == 1 and len(f.tree(0)[0]) > 3
    if kind == "gini":
        # the forest carries leaf class counts: soft votes of one tree are a distribution
        assert f.num_classes == 4 and f.tree(0)[1].shape[1] == 4
        assert raw.shape == (N, 4)
        np.testing.assert_allclose(raw.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    else:
        assert f.num_classes == 0


@pytest.mark.parametrize("kind", ["gini", "real"])
def test_fit_bag_replays_the_split_finding_sample(ctx, kind):
    """A bag of more than max(maxBins^2, 10^4) rows: RandomForest.findSplits samples it."""
    n = 6000
    rng = np.random.default_rng(9)
    X = np.round(rng.normal(size=(n, F)) * 40) / 16  # more distinct values than bins
    y = labels(kind, X)
    bag = boosted_style_bag(n, seed=4, scale=10.0)
    assert int(bag.astype(np.int64).sum()) > 10_000
    fit_both(ctx, X, y, bag, np.arange(F, dtype=np.int32), [0, 2500, 2500, n], kind == "gini")


def test_all_zero_bag_is_empty(ctx):
    X = features(N)
    ds = nat.DeviceDataset.from_numpy(X, labels("gini", X), ctx)
    try:
        for imp in (nat.IMPURITY_GINI, nat.IMPURITY_VARIANCE):
            with pytest.raises(sb.SparkException) as e:
                nat.fit_bag(ctx, ds, np.zeros(N, np.uint8), SUB, impurity=imp)
            assert e.value.code == nat.SBAG_EEMPTY
        # the context and the dataset stay usable
        f = nat.fit_bag(ctx, ds, boosted_style_bag(N), SUB, impurity=nat.IMPURITY_GINI, max_depth=2)
        assert len(f) == 1
    finally:
        ds.free()


def test_fit_bag_validation_is_the_boosters(ctx):
    X = features(200)
    ds = nat.DeviceDataset.from_numpy(X, labels("real", X), ctx)
    bag = np.ones(200, np.uint8)
    try:
        with pytest.raises(sb.IllegalArgumentException):  # gini needs class labels
            nat.fit_bag(ctx, ds, bag, SUB, impurity=nat.IMPURITY_GINI)
        with pytest.raises(sb.IllegalArgumentException):
            nat.fit_bag(ctx, ds, bag, SUB, impurity=7)
        with pytest.raises(sb.IllegalArgumentException):
            nat.fit_bag(ctx, ds, bag, [3, 2], impurity=nat.IMPURITY_VARIANCE)
        with pytest.raises(sb.IllegalArgumentException):
            nat.fit_bag(ctx, ds, bag, SUB, impurity=nat.IMPURITY_VARIANCE, max_depth=31)
        with pytest.raises(sb.IllegalArgumentException):
            nat.fit_bag(ctx, ds, bag, SUB, impurity=nat.IMPURITY_VARIANCE, partition_offsets=[0, 10, 199])
    finally:
        ds.free()
    assert nat.lib().sbag_fit_bag(None, None, None, None) == nat.SBAG_EINVAL
