"""GPU: sbag_predict_leaves / sbag_proximity / sbag_proximity_moments and their _dataset forms,
integer for integer against proximity_ref.py, through host rows and device datasets and both
stage-A paths (SBAG_PROX_FORCE_FALLBACK unset: k_leaf_tiled wherever the plan allows it; "1":
k_leaf_walk)."""
import numpy as np
import pytest

import proximity_ref as pr
import weighted_ref as wr
from test_gpu_quantiles import features

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

KNOB = "SBAG_PROX_FORCE_FALLBACK"
BM, BN = nat.proximity_tile()


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def check(ctx, monkeypatch, f, Xq, Xr, groups=None, G=0, repeat=1):
    """Leaves, counts and (with groups) moments of `repeat` copies of Xq against Xr: host rows
    and datasets, both paths, all equal to the reference.  Returns the reference's leaves and
    counts of one copy."""
    trees, subs = [f.tree(t)[0] for t in range(len(f))], [f.subspace(t) for t in range(len(f))]
    Lq, Lr = pr.leaves(trees, subs, Xq), pr.leaves(trees, subs, Xr)
    cnt = pr.counts(Lq, Lr)
    want = np.tile(cnt.astype(np.uint16), (repeat, 1))
    Xq = np.ascontiguousarray(np.tile(Xq, (repeat, 1)))
    dq, dr = (nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx) for X in (Xq, Xr))
    try:
        for force in (None, "1"):
            monkeypatch.delenv(KNOB, raising=False) if force is None else monkeypatch.setenv(KNOB, force)
            for label, got in (("host", nat.proximity(ctx, f, Xq, Xr)),
                               ("dataset", nat.proximity_dataset(ctx, f, dq, dr))):
                assert got.dtype == np.uint16
                np.testing.assert_array_equal(got, want, err_msg=f"counts, {label}, force={force}")
            np.testing.assert_array_equal(nat.predict_leaves(ctx, f, Xr), Lr)
            np.testing.assert_array_equal(nat.predict_leaves_dataset(ctx, f, dq)[:len(Lq)], Lq)
            if groups is not None:
                mom = np.tile(pr.moments(cnt, groups, G), (repeat, 1, 1))
                np.testing.assert_array_equal(nat.proximity_moments(ctx, f, Xq, Xr, groups, G), mom)
                np.testing.assert_array_equal(nat.proximity_moments_dataset(ctx, f, dq, dr, groups, G), mom)
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        dq.free()
        dr.free()
    return Lq, cnt


def fitted(ctx, X, L, cb=1, impurity=nat.IMPURITY_VARIANCE):
    rng = np.random.default_rng(L)
    y = rng.integers(0, 3, len(X)).astype(np.float64)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == cb
    try:
        return nat.fit(ctx, ds, replacement=True, sample_ratio=0.8, seed=11, learner_begin=0, learner_end=L,
                       max_depth=3, impurity=impurity)
    finally:
        ds.free()


@pytest.mark.parametrize("cb", [1, 2])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 15, 16, 17, 64, 65, 129])
def test_tree_counts(ctx, monkeypatch, L, cb):
    """Depth-3 fits of L trees on 300 x 6 rows: a signature that ends inside a dword, on one, on
    16 bytes and one past it, and a second K chunk (129).  The references are rows of the
    queries, so their pairs count every tree: a padding position that differed would show."""
    X = features(np.random.default_rng(L), 300, 6, cb)
    f = fitted(ctx, X, L, cb, nat.IMPURITY_GINI if L == 5 else nat.IMPURITY_VARIANCE)
    try:
        groups = np.arange(129) * 7 % 3
        _, cnt = check(ctx, monkeypatch, f, X, X[100:229], groups, 3)
        assert (cnt[np.arange(100, 229), np.arange(129)] == L).all() and cnt.max() == L
    finally:
        f.free()


@pytest.fixture(scope="module")
def forest17(ctx):
    X = features(np.random.default_rng(0), 300, 6, 1)
    f = fitted(ctx, X, 17)
    yield X, f
    f.free()


@pytest.mark.parametrize("nq,nr,repeat", [(1, 1, 1), (BM - 1, BN + 1, 1), (BM + 1, 2 * BN - 1, 1), (300, 7, 1),
                                          (300, 7, 467)])
def test_tile_edges(ctx, monkeypatch, forest17, nq, nr, repeat):
    """Row sets that straddle the block tile; 467 copies of 300 rows are three query batches of
    counts mode (two device buffers, so the third waits for the first one's copy)."""
    X, f = forest17
    check(ctx, monkeypatch, f, X[:nq], X[300 - nr:], repeat=repeat)


@pytest.mark.parametrize("G,repeat", [(1, 1), (3, 1), (16, 1), (16, 220)])
def test_moments(ctx, monkeypatch, forest17, G, repeat):
    """Interleaved group ids over 300 references: groups larger than a column block (G = 1),
    none a multiple of it, the last one empty.  220 copies of the queries are two query batches
    whose blocks each take several column blocks, so a block changes group on the way."""
    X, f = forest17
    groups = np.arange(300) * 7 % G
    groups[groups == G - 1] = 0
    check(ctx, monkeypatch, f, X, X, groups.astype(np.int32), G, repeat=repeat)


def complete(depth):
    """A complete tree over feature 0, pre-order, whose 2^depth leaves split the values 0, 1, ..."""
    a = wr._blank(2 ** (depth + 1) - 1)
    nxt = [0]

    def build(lo, hi):
        k = nxt[0]
        nxt[0] += 1
        if hi - lo > 1:
            mid = (lo + hi) // 2
            a["feature"][k], a["threshold"][k] = 0, mid - 0.5
            a["left"][k] = build(lo, mid)
            a["right"][k] = build(mid, hi)
        return k

    build(0, 2 ** depth)
    return a


FORESTS = {
    "root-only": lambda: [wr.leaf(1.0)],
    "256-leaves": lambda: [complete(8), wr.stump(9.5, 0.0, 1.0)],  # code 0xFF is a leaf, the codes still u8
    "chain-300": lambda: [wr.comb(np.arange(299) + 0.5, np.arange(300.0)), wr.stump(255.5, 0.0, 1.0)],  # u16
    "same-value": lambda: [wr.stump(99.5, 1.0, 1.0), wr.stump(199.5, 1.0, 1.0)],  # leaves, not values
}


@pytest.mark.parametrize("name", list(FORESTS))
def test_hand_built_forests(ctx, monkeypatch, name):
    X = np.arange(300.0)[:, None]
    trees = FORESTS[name]()
    f = nat.NativeForest.from_trees(trees, [[0]] * len(trees), nat.IMPURITY_VARIANCE)
    try:
        Lq, cnt = check(ctx, monkeypatch, f, X, np.ascontiguousarray(X[::-1][:140]), np.arange(140) % 2, 2)
        code = (np.cumsum(trees[0]["left"] < 0) - 1)[Lq[:, 0]]  # the first tree's leaf codes
        if name == "root-only":
            assert (cnt == 1).all()
        elif name == "256-leaves":
            assert code.max() == 255 and (code == 255).sum() == 45
        elif name == "chain-300":
            assert {255, 256, 299} <= set(code)
        else:
            assert cnt.min() == 0 and set(np.unique(cnt)) == {0, 1, 2}
    finally:
        f.free()


def test_outlier_measure(ctx):
    """A 200-row two-class set with one row moved far away: the model's outlierMeasure against
    the same formula over the reference counts."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(200, 4))
    y = (X[:, 0] + X[:, 1] + 0.5 * rng.normal(size=200) > 0).astype(np.float64)  # no clean split: deep trees
    X[10] += 40.0
    model = sb.BaggingClassifier().setNumBaseLearners(50).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(5)).fit(sb.Frame(X, y))
    cnt = pr.counts(*[pr.leaves([m.nodes for m in model.models], model.subspaces, X)] * 2)
    np.testing.assert_array_equal(model.proximity(X, counts=True), cnt)
    np.testing.assert_array_equal(model.proximity(X), cnt / 50.0)
    np.testing.assert_array_equal(model.predictLeaves(X), model.predictLeaves(sb.Frame(X, y)))
    want = pr.outlier(cnt, 50, y)
    assert np.isfinite(want).sum() > 50  # (a class whose median deviation is 0 gives inf and NaN on both sides)
    np.testing.assert_allclose(model.outlierMeasure(X, y), want, rtol=1e-12)
    with pytest.raises(sb.IllegalArgumentException):
        model.outlierMeasure(X)


@pytest.mark.parametrize("case", ["null", "group-id", "no-groups", "17-groups", "feature-counts", "short-rows"])
def test_refusals_leave_the_context_usable(ctx, forest17, case):
    X, f = forest17
    lib, P = nat.lib(), nat.ptr
    out = np.full((300, 300), 7, np.uint16)
    mom = np.full((300, 16, 2), 7, np.uint64)
    g = np.zeros(300, np.int32)
    pair = (ctx.handle, f.handle, P(X), 300, 6, P(X), 300, 6)
    narrow = np.ascontiguousarray(X[:, :1])
    rc = {"null": lambda: lib.sbag_proximity(ctx.handle, f.handle, P(X), 300, 6, None, 300, 6, P(out)),
          "group-id": lambda: lib.sbag_proximity_moments(*pair, P(np.full(300, 3, np.int32)), 3, P(mom)),
          "no-groups": lambda: lib.sbag_proximity_moments(*pair, P(g), 0, P(mom)),
          "17-groups": lambda: lib.sbag_proximity_moments(*pair, P(g), 17, P(mom)),
          "feature-counts": lambda: lib.sbag_proximity(ctx.handle, f.handle, P(X), 300, 6, P(narrow), 300, 1, P(out)),
          "short-rows": lambda: lib.sbag_predict_leaves(ctx.handle, f.handle, P(narrow), 300, 1, P(out))}[case]()
    assert rc == nat.SBAG_EINVAL and (out == 7).all() and (mom == 7).all()
    assert nat.proximity(ctx, f, X[:0], X).shape == (0, 300) and nat.proximity(ctx, f, X, X[:0]).shape == (300, 0)
    assert (np.diag(nat.proximity(ctx, f, X, X)) == 17).all()
