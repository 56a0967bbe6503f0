"""GPU: sbag_predict_contributions / _dataset, byte for byte (sign bits included) against
contrib_ref.restated.  Every check goes through both entry points (host rows: k_quantize + u16
codes; the dataset's own codes) and both paths (SBAG_CONTRIB_FORCE_FALLBACK unset: k_contrib_tiled
wherever the plan allows it; "1": k_contrib_walk) against one reference computed once."""
import math

import numpy as np
import pytest

import contrib_ref as cr
import weighted_ref as wr

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

KNOB = "SBAG_CONTRIB_FORCE_FALLBACK"


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def same_bits(got, want, label=""):
    np.testing.assert_array_equal(got, want, err_msg=label)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(want), err_msg=label)


def check(ctx, monkeypatch, f, X, ds, class_index=-1, weights=None):
    """ds None: host rows only (values a dataset's dictionary does not take)."""
    trees, stats = zip(*[f.tree(t) for t in range(len(f))])
    want = cr.restated(trees, stats, [f.subspace(t) for t in range(len(f))], X, class_index, weights)
    for force in (None, "1"):
        monkeypatch.delenv(KNOB, raising=False) if force is None else monkeypatch.setenv(KNOB, force)
        same_bits(nat.predict_contributions(ctx, f, X, class_index, weights), want, f"host rows, force={force}")
        if ds is not None:
            same_bits(nat.predict_contributions_dataset(ctx, f, ds, class_index, weights), want, f"dataset, force={force}")
    monkeypatch.delenv(KNOB, raising=False)
    return want


def features(rng, N, F, cb):
    """u8 codes: 50 distinct values a feature; u16: feature 0 has N distinct ones."""
    X = rng.integers(0, 50, size=(N, F)).astype(np.float64)
    X[:, 0] = rng.permutation(N) * 0.5 if cb == 2 else X[:, 0]
    return X


def fitted(ctx, X, y, cb, L, impurity):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == cb
    return ds, nat.fit(ctx, ds, max_depth=3, impurity=impurity, replacement=True, sample_ratio=0.8, seed=11,
                       learner_begin=0, learner_end=L, subspace_ratio=0.5, subspace_bug_compat=False)


def hand_forest(ctx, trees, stats, subs, X, impurity=nat.IMPURITY_VARIANCE):
    return (nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx),
            nat.NativeForest.from_trees(trees, subs, impurity, stats=stats))


@pytest.mark.parametrize("impurity", [nat.IMPURITY_VARIANCE, nat.IMPURITY_GINI])
@pytest.mark.parametrize("cb", [1, 2])
@pytest.mark.parametrize("L", [1, 3, 64])
def test_fitted_forests(ctx, monkeypatch, L, cb, impurity):
    """Depth-3 fits on 1000 x 6 rows at subspace ratio 0.5 (local and global feature indices
    differ, some features are in no tree), with weights and without; gini: class 0 and the last."""
    rng = np.random.default_rng(1000 * L + cb)
    X = features(rng, 1000, 6, cb)
    gini = impurity == nat.IMPURITY_GINI
    y = rng.integers(0, 3, 1000).astype(np.float64) if gini else X[:, 1] + rng.normal(size=1000)
    ds, f = fitted(ctx, X, y, cb, L, impurity)
    try:
        for ci, w in [(ci, w) for ci in ((0, 2) if gini else (-1,)) for w in (None, rng.normal(size=L))]:
            check(ctx, monkeypatch, f, X, ds, ci, w)
    finally:
        f.free()
        ds.free()


def tile_rows(F, M):
    """contrib_tile_rows of sbag_contrib_plan.h for host rows (u16 codes at stride host_stride(F))."""
    fits = lambda rows: (((rows * (wr.host_stride(F) * 2 + 4) + 15) & ~15) + rows * (F + 1) * 8 + (M + 2) ** 2 * 8
                         + max(rows * (8 if M <= 7 else 16), 256) * 8 <= wr.LDS_CAP)
    return next((rows for rows in (64, 32, 16) if fits(rows)), 0)


# (forest, features, rows, SBAG_PREDICT_BATCH_ROWS): every hand-built forest; the row seams of a
# 64-row tile, the last in batches that end inside a tile; the smallest F whose tile has 32 and 16
# rows (8-lane and 16-lane groups) and the smallest past the LDS: the general path by itself
SHAPES = [(case, 16, 130, None) for case in cr.HAND_BUILT]
SHAPES += [("merged", 6, N, None) for N in (1, 15, 17, 63, 65)] + [("merged", 6, 129, 37)]
SHAPES += [(f"chain {m}", next(F for F in range(16, 4096) if tile_rows(F, m) == rows), 40, None)
           for m, rows in ((7, 32), (7, 16), (7, 0), (15, 32), (15, 16))]


@pytest.mark.parametrize("case,F,N,batch", SHAPES)
def test_hand_built_forests(ctx, monkeypatch, case, F, N, batch):
    trees, stats, subs, X = cr.hand_built(case, F)
    if batch:
        monkeypatch.setenv("SBAG_PREDICT_BATCH_ROWS", str(batch))
    ds, f = hand_forest(ctx, trees, stats, subs, X[:N])
    try:
        got = check(ctx, monkeypatch, f, X[:N], ds)
        if case == "single leaf":
            assert (got[:, :-1] == 0.0).all() and not np.signbit(got).any() and (got[:, -1] == 2.5).all()
        if case == "cancel":
            assert (got[:, :-1] == 0.0).all()
        if case == "merged" and F == 6:  # NaN goes right at every test, -inf left, +inf right
            X[:6, 5], X[6:12, 4] = [[np.nan, -np.inf, np.inf, 3.0, np.nan, -np.inf]] * 2
            check(ctx, monkeypatch, f, X[:N], None)
    finally:
        f.free()
        ds.free()


@pytest.mark.parametrize("case", cr.EXACT_CASES + ["fit"])
def test_against_exact(ctx, case):
    """|out - exact| <= K 2^-53 sum |vw_l| on 40 rows, and each row's sum against nat.predict /
    predict_weighted within the same bound plus one ulp.  Measured scaled errors of `restated`
    against `exact`: hand-built forests 0.98 at most ("negative zero", unweighted); the fit 0.083
    (mean) and 0.16 (weighted).  K = 4 x the largest = contrib_ref.K = 3.93."""
    if case == "fit":
        X = features(np.random.default_rng(3), 1000, 6, 1)
        ds, f = fitted(ctx, X, X[:, 1] + np.random.default_rng(4).normal(size=1000), 1, 3, nat.IMPURITY_VARIANCE)
    else:
        ds, f = hand_forest(ctx, *cr.hand_built(case))
        X = cr.hand_built(case)[3]
    try:
        (trees, stats), subs, X = zip(*[f.tree(t) for t in range(len(f))]), [f.subspace(t) for t in range(len(f))], X[:40]
        for w in (None, np.random.default_rng(1).normal(size=len(f))):
            scale = cr.scale(trees, stats, subs, -1, w)
            got = nat.predict_contributions(ctx, f, X, -1, w)
            err = cr.scaled_error(got, cr.exact(trees, stats, subs, X, w), scale)
            pred = nat.predict(ctx, f, X, nat.AGG_MEAN) if w is None else nat.predict_weighted(ctx, f, X, nat.W_DOT, w)[:, 0]
            gap = max(abs(math.fsum(r) - p) - np.spacing(abs(p)) for r, p in zip(got, pred)) / (2.0 ** -53 * scale)
            print(f"{case}, weights={w is not None}: scaled error {err}, row sums {gap}, K {cr.K}")
            assert err <= cr.K and gap <= cr.K
    finally:
        f.free()
        ds.free()


def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    trees, stats, subs, X = cr.hand_built("merged", F=6)
    gtrees, gstats = [wr.stump(4.5, 0, 1)], [np.array([[6.0, 4.0], [5.0, 1.0], [1.0, 3.0]])]
    ds, var = hand_forest(ctx, trees, stats, subs, X)
    ds1, gin = hand_forest(ctx, gtrees, gstats, [[0, 1]], X[:, :1], nat.IMPURITY_GINI)
    bare = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_VARIANCE)
    zero = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_VARIANCE, stats=[s * (np.arange(len(s)) != 3)[:, None] for s in stats])
    try:
        good = check(ctx, monkeypatch, var, X, ds)
        cases = [(var, 0), (var, -2), (gin, -1), (gin, 2), (bare, -1), (zero, -1)]
        calls = [lambda f=f, ci=ci: nat.predict_contributions(ctx, f, X, ci) for f, ci in cases]
        calls += [lambda f=f, ci=ci: nat.predict_contributions_dataset(ctx, f, ds, ci) for f, ci in cases]
        calls += [lambda: nat.predict_contributions(ctx, var, X[:, :1]),         # a subspace past the features
                  lambda: nat.predict_contributions_dataset(ctx, var, ds1),
                  lambda: nat.check(nat.lib().sbag_predict_contributions(ctx.handle, var.handle, None, 5, 6, -1, None, nat.ptr(good))),
                  lambda: nat.check(nat.lib().sbag_predict_contributions_dataset(ctx.handle, var.handle, ds.handle, -1, None, None))]
        for k, call in enumerate(calls):
            with pytest.raises(nat.SbagError) as e:
                call()
            assert e.value.code == nat.SBAG_EINVAL, k
            same_bits(nat.predict_contributions_dataset(ctx, var, ds), good)
        assert nat.predict_contributions(ctx, var, X[:0]).shape == (0, 7)
        want = cr.restated(gtrees, gstats, [[0, 1]], X, 1)
        same_bits(nat.predict_contributions(ctx, gin, X, 1), want)
        assert (want[:, 1] == 0.0).all() and abs(want[0].sum() - (0.75 if X[0, 0] > 4.5 else 1 / 6)) < 1e-15
    finally:
        for h in (ds, ds1, var, gin, bare, zero):
            h.free()


def test_models(ctx):
    """predictContributions of the bagging models and the GBM regressor (4 boosters), from host
    rows and from a DeviceDataset; the GBM's rows sum to transform within K 2^-53 sum |vw_l| plus
    one ulp of the sum."""
    rng = np.random.default_rng(4)
    X = features(rng, 1000, 6, 1)
    y = X[:, 0] + rng.normal(size=1000)
    tree = sb.DecisionTreeRegressor().setMaxDepth(3)
    reg = sb.BaggingRegressor().setNumBaseLearners(5).setBaseLearner(tree).fit(sb.Frame(X, y))
    cls = sb.BaggingClassifier().setNumBaseLearners(3).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(2)).fit(sb.Frame(X, (y > 20).astype(np.float64)))
    gbm = sb.GBMRegressor().setBaseLearner(tree).fit(sb.Frame(X, y), params={"numBaseLearners": 4})
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        for model, kw, ci, w in ((reg, {}, -1, None), (cls, dict(classIndex=1), 1, None), (gbm, {}, -1, gbm.weights)):
            args = ([m.nodes for m in model.models], [m.stats for m in model.models], model.subspaces)
            want = cr.restated(*args, X, ci, w)
            want[:, -1] += gbm.const if model is gbm else 0.0
            got = model.predictContributions(X, **kw)
            same_bits(got, want)
            same_bits(model.predictContributions(ds, **kw), want)
        bound = cr.K * 2.0 ** -53 * cr.scale(*args, -1, gbm.weights)
        gap = max(abs(math.fsum(r) - p) - np.spacing(abs(p)) for r, p in zip(got, gbm.transform(X)))
        print(f"GBM row sums against transform, past one ulp: {gap}, bound {bound}")
        assert gap <= bound
    finally:
        ds.free()
