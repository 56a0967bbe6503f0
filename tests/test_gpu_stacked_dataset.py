"""GPU: sbag_dataset_create_stacked (the level-1 dataset of a stacking fit, built on the device
from the base trees' leaves) against sbag_dataset_create on the host matrix of sbag_predict's
per-tree predictions: layout, every code byte, dictionaries, offsets and labels are compared for
equality, and both against the NumPy restatement (stacking_ref.dataset_layout).  Then the stacker
(sbag_fit_bag) on both datasets against the oracle's tree on the host matrix.

The planner's chunking is restated from its formulas (plan_tiled, sbag_host.cpp): a tree of n
internal nodes takes (3n + 2) * 8 bytes of a chunk of min(64 KB, 160 KB - 512 - the row tile)
bytes, the row tile being 512 * (S * code_bytes + 4) bytes."""
import ctypes

import numpy as np
import pytest

import oracle
import predict_ref as ref
import stacking_ref as sref
from parity_utils import assert_forest_equal

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

F = 6
VAR, GINI = nat.IMPURITY_VARIANCE, nat.IMPURITY_GINI


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def features(n, seed=5):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, F)) * 6) / 4
    X[rng.random((n, F)) < 0.15] = 0.0
    X[:, 5] = rng.integers(0, 3, n)
    return X


def labels(kind, X, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "gini":
        return ((np.floor(np.abs(X[:, 0]) * 2) + (X[:, 3] > 0) + rng.integers(0, 2, len(X))) % 3).astype(np.float64)
    y = np.round(X[:, 0] * 8 - X[:, 2] * 4) / 8 + rng.integers(-8, 9, len(X)) / 16.0
    return y if kind == "dyadic" else y * 1.1 + 0.3 + rng.normal(size=len(X)) / 7


XTEST = features(4099, seed=23)   # shared by the cases, never written


# ---------------------------------------------------------------- hand-built trees
def _blank(n):
    a = np.zeros(n, nat.NODE_DTYPE)
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


def comb(thr, leaves, feature=0):
    """len(thr) internal nodes in one right-deep chain, pre-order ids: node 2i has leaf 2i + 1
    on the left and node 2i + 2 on the right."""
    thr = np.asarray(thr, np.float64)
    n = len(thr)
    a = _blank(2 * n + 1)
    i = 2 * np.arange(n)
    a["left"][i], a["right"][i] = i + 1, i + 2
    a["feature"][i] = feature
    a["threshold"][i] = thr
    a["prediction"][np.concatenate([i + 1, [2 * n]])] = leaves
    return a


def full_sub(k):
    return [np.arange(F, dtype=np.int32)] * k


# ---------------------------------------------------------------- the comparison
def exported(ds):
    n, f, s, cb, dv = ds.layout()
    codes = np.zeros(n * s * cb, np.uint8)
    d, off, y = ds.export(codes.ctypes.data)
    return (n, f, s, cb, dv), codes, d, off, y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_stacked(ctx, X, y, forest, gini, code_bytes=None):
    """-> (device-built level-1 dataset, sbag_dataset_create's, the host matrix); the caller
    frees the two datasets."""
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        dev = ds.stacked(forest)
    finally:
        ds.free()
    _, pt = nat.predict(ctx, forest, X, nat.AGG_MODE if gini else nat.AGG_MEAN, per_tree=True)
    P = np.ascontiguousarray(pt.T)
    host = nat.DeviceDataset.from_numpy(P, y, ctx)
    got, want = exported(dev), exported(host)
    assert got[0] == want[0], f"layout {got[0]} vs {want[0]}"
    assert np.array_equal(got[1], want[1]), "codes differ"
    assert same_bits(got[2], want[2]), "dictionaries differ"   # (bits: no -0.0 may slip in)
    assert np.array_equal(got[3], want[3]), "dictionary offsets differ"
    assert same_bits(got[4], want[4]) and same_bits(got[4], y), "labels differ"
    # and the restatement, from predict_ref's walk
    trees = [forest.tree(t)[0] for t in range(len(forest))]
    subs = [forest.subspace(t) for t in range(len(forest))]
    d, off, cb, S, codes = sref.dataset_layout(sref.level1(trees, subs, X))
    assert got[0] == (len(X), len(trees), S, cb, len(d))
    assert same_bits(got[2], d) and np.array_equal(got[3], off)
    assert np.array_equal(got[1], codes.reshape(-1).view(np.uint8))
    if code_bytes is not None:
        assert dev.layout()[3] == code_bytes
    return dev, host, P


def free(*objs):
    for o in objs:
        o.free()


def fitted(ctx, kind, K, depth=3, n=600, seed=7):
    X = features(n, seed=seed)
    ds = nat.DeviceDataset.from_numpy(X, labels(kind, X), ctx)
    try:
        return nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=41, learner_begin=0, learner_end=K,
                       subspace_ratio=1.0, max_depth=depth, impurity=GINI if kind == "gini" else VAR)
    finally:
        ds.free()


# ---------------------------------------------------------------- 1. row and tree counts
@pytest.fixture(scope="module")
def forest3(ctx):
    f = fitted(ctx, "dyadic", 3)
    yield f
    f.free()


@pytest.mark.parametrize("n", [1, 63, 257, 4099])
def test_row_counts(ctx, forest3, n):
    """Wave and workgroup tails; the rows are not the ones the trees were fitted on."""
    X = XTEST[:n]
    free(*check_stacked(ctx, X, labels("real", X), forest3, False)[:2])


@pytest.mark.parametrize("K,stride", [(1, 16), (16, 16), (17, 32), (65, 128)])
def test_tree_counts(ctx, K, stride):
    """Stride 16 without padding, 32 with 15 padding columns, and the 128 stride."""
    f = fitted(ctx, "dyadic", K)
    X = XTEST[:257]
    dev, host, _ = check_stacked(ctx, X, labels("dyadic", X), f, False)
    assert dev.layout()[2] == stride
    free(dev, host, f)


# ---------------------------------------------------------------- 2. class-valued trees
def test_gini_trees_share_few_values(ctx):
    """Many leaves, three values; a stump whose children predict the same class gives a
    one-value dictionary."""
    f = fitted(ctx, "gini", 4, depth=5)
    trees = [f.tree(t)[0] for t in range(4)] + [stump(0.0, 1.0, 1.0, feature=2)]
    assert all((t["left"] < 0).sum() > 3 for t in trees[:4])
    g = nat.NativeForest.from_trees(trees, full_sub(5), GINI)
    X = XTEST[:1000]
    dev, host, P = check_stacked(ctx, X, labels("gini", X), g, True, code_bytes=1)
    d, off, _ = dev.export()
    assert off[5] - off[4] == 1 and d[off[4]] == 1.0 and (np.diff(off) <= 3).all()
    free(dev, host, f, g)


# ---------------------------------------------------------------- 3. u16 codes
def test_u16_code_width(ctx):
    """A depth-10 variance tree on 4000 rows with real-valued labels: 792 distinct leaf values
    on the CPU oracle (seed 17), all reached by the training rows, so the codes are u16."""
    rng = np.random.default_rng(17)
    n = 4000
    X = np.round(rng.normal(size=(n, F)) * 40) / 16
    y = X[:, 0] * 1.1 + np.sin(X[:, 1]) * 3 + rng.normal(size=n) / 7
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = nat.fit_bag(ctx, ds, np.ones(n, np.uint8), np.arange(F, dtype=np.int32), impurity=VAR,
                        max_depth=10, min_instances_per_node=1)
    finally:
        ds.free()
    nodes = f.tree(0)[0]
    assert len(np.unique(nodes["prediction"][nodes["left"] < 0])) > 256
    small = fitted(ctx, "dyadic", 2)
    g = nat.NativeForest.from_trees([small.tree(0)[0], nodes, small.tree(1)[0]], full_sub(3), VAR)
    dev, host, _ = check_stacked(ctx, X, y, g, False, code_bytes=2)
    assert dev.layout()[3] == 2  # (sbag_dataset_layout: not silently u8)
    free(dev, host, f, small, g)


# ---------------------------------------------------------------- 4. hand-built edges
def test_hand_built_edges(ctx):
    """A leaf no row reaches, a -0.0 leaf next to a 0.0 leaf, a single-leaf tree, equal
    predictions of different leaves."""
    X = XTEST[:257].copy()
    assert X[:, 0].min() > -50 and (X[:, 1] <= 0).any() and (X[:, 1] > 0).any()
    trees = [
        comb([-100.0, 0.0], [5.0, 1.0, 2.0]),            # leaf 5.0: x0 <= -100 never happens
        stump(0.0, -0.0, 0.0, feature=1),                # one value, +0.0
        leaf(3.25),                                      # a constant feature
        comb([-1.0, 0.0, 1.0], [7.0, -2.0, 7.0, -0.0]),  # 7.0 twice; -0.0 among others
    ]
    g = nat.NativeForest.from_trees(trees, full_sub(4), VAR)
    dev, host, P = check_stacked(ctx, X, labels("real", X), g, False, code_bytes=1)
    d, off, _ = dev.export()
    assert list(np.diff(off)) == [2, 1, 1, 3]
    assert list(d[off[0]:off[1]]) == [1.0, 2.0]          # no 5.0
    assert d[off[1]] == 0.0 and not np.signbit(d[off[1]])
    assert list(d[off[3]:off[4]]) == [-2.0, 0.0, 7.0] and not np.signbit(d[off[3] + 1])
    free(dev, host, g)


# ---------------------------------------------------------------- 5. several LDS chunks
def tiled_budget(S, code_bytes):
    fixed = (512 * (S * code_bytes + 4) + 15) & ~15
    return min(64 * 1024, 160 * 1024 - 512 - fixed) & ~15


def plan_chunks(sizes, budget):
    """plan_tiled's greedy chunking of trees of `sizes` bytes."""
    chunks, used = 0, 0
    for b in sizes:
        assert b <= budget
        if chunks == 0 or used + b > budget:
            chunks, used = chunks + 1, 0
        used += b
    return chunks


def test_trees_span_several_chunks(ctx):
    """Three combs of 1000 internal nodes (24 016 bytes each) and small trees between them do
    not fit one 64 KB chunk; each comb gives 1001 values, so the codes are u16 too."""
    n = 4099
    rng = np.random.default_rng(2)
    X = XTEST.copy()
    X[:, 0] = rng.integers(-20, 1030, n).astype(np.float64)
    X[:, 1] = rng.integers(0, 1000, n) / 8.0
    combs = [comb(np.arange(1000.0), np.arange(1001.0) * 0.5 - 3.0, feature=0),
             comb(np.arange(1000.0) / 8.0, -np.arange(1001.0), feature=1),
             comb(np.arange(1000.0) + 0.5, np.arange(1001.0) % 7, feature=0)]
    trees = [combs[0], stump(0.0, 1.0, 2.0, feature=2), combs[1], leaf(4.0), combs[2]]
    sizes = [(3 * int((t["left"] >= 0).sum()) + 2) * 8 for t in trees]
    assert X.shape[1] <= 16
    assert plan_chunks(sizes, tiled_budget(16, 1)) >= 2
    g = nat.NativeForest.from_trees(trees, full_sub(5), VAR)
    dev, host, _ = check_stacked(ctx, X, labels("real", X), g, False, code_bytes=2)
    free(dev, host, g)


# ---------------------------------------------------------------- 6. the stacker on it
def fit_stacker(ctx, ds, K, gini, part, depth, bins=32):
    return nat.fit_bag(ctx, ds, np.ones(ds.shape[0], np.uint8), np.arange(K, dtype=np.int32),
                       impurity=GINI if gini else VAR, partition_offsets=part, max_depth=depth, max_bins=bins)


@pytest.mark.parametrize("kind", ["gini", "real", "dyadic"])
def test_stacker_fits_equal_on_both_datasets_and_the_oracle(ctx, kind):
    """Real-valued labels and 3 partitions (one of a single row) carried through."""
    gini = kind == "gini"
    K, n = 5, 3000
    f = fitted(ctx, kind, K, depth=4)
    X = XTEST[:n]
    y = labels(kind, X)
    part = [0, 1100, 1101, n]
    dev, host, P = check_stacked(ctx, X, y, f, gini)
    a, b = fit_stacker(ctx, dev, K, gini, part, 4), fit_stacker(ctx, host, K, gini, part, 4)
    orf = oracle.fit(P, y, np.ones((1, n), np.uint8), [np.arange(K, dtype=np.int32)], max_depth=4,
                     max_bins=32, classification=gini, part=part)
    assert len(a.tree(0)[0]) > 3
    assert_forest_equal(a, orf)
    assert_forest_equal(b, orf)
    free(a, b, dev, host, f)


@pytest.mark.parametrize("kind", ["gini", "real"])
def test_stacker_replays_the_split_finding_sample(ctx, kind):
    """More than max(maxBins^2, 10^4) rows in 3 partitions: RandomForest.findSplits samples the
    level-1 rows, partition by partition; a deep base tree gives it more values than bins."""
    gini = kind == "gini"
    n = 12000
    X = features(n, seed=31)
    y = labels(kind, X)
    part = [0, 5000, 5000, n]
    f = fitted(ctx, kind, 3, depth=8, n=3000)
    dev, host, P = check_stacked(ctx, X, y, f, gini)
    if not gini:
        assert max(len(np.unique(P[:, k])) for k in range(3)) > 32
    a, b = fit_stacker(ctx, dev, 3, gini, part, 5), fit_stacker(ctx, host, 3, gini, part, 5)
    orf = oracle.fit(P, y, np.ones((1, n), np.uint8), [np.arange(3, dtype=np.int32)], max_depth=5,
                     max_bins=32, classification=gini, part=part)
    assert_forest_equal(a, orf)
    assert_forest_equal(b, orf)
    free(a, b, dev, host, f)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_context_usable(ctx, forest3):
    L = nat.lib()
    X = XTEST[:100]
    ds = nat.DeviceDataset.from_numpy(X, labels("real", X), ctx)
    narrow = nat.DeviceDataset.from_numpy(X[:, :2], labels("real", X), ctx)  # the trees test feature 5
    h = ctypes.c_void_p()
    assert L.sbag_dataset_create_stacked(None, ds.handle, forest3.handle, ctypes.byref(h)) == nat.SBAG_EINVAL
    assert L.sbag_dataset_create_stacked(ctx.handle, None, forest3.handle, ctypes.byref(h)) == nat.SBAG_EINVAL
    assert L.sbag_dataset_create_stacked(ctx.handle, ds.handle, None, ctypes.byref(h)) == nat.SBAG_EINVAL
    assert L.sbag_dataset_create_stacked(ctx.handle, ds.handle, forest3.handle, None) == nat.SBAG_EINVAL
    assert not h.value
    with pytest.raises(sb.IllegalArgumentException, match="fewer features"):
        narrow.stacked(forest3)
    nan = nat.NativeForest.from_trees([stump(0.0, np.nan, 1.0)], full_sub(1), VAR)
    with pytest.raises(sb.IllegalArgumentException, match="NaN"):
        ds.stacked(nan)
    free(*check_stacked(ctx, X, labels("real", X), forest3, False)[:2])
    free(ds, narrow, nan)
