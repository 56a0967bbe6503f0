"""GPU: sbag_predict_weighted / sbag_predict_weighted_dataset on hand-built forests, at the
smallest shapes at which the fused pass (k_wpred_tiled) can go wrong, and the four boosted
models that now run through it.

Every output is defined bit for bit, so every assertion is assert_array_equal (plus the sign
bit where the value is no NaN) against weighted_ref.py, which test_weighted_ref_host.py holds
to the oracle.  Every case goes through both entry points (host rows: k_quantize + u16 codes;
a DeviceDataset: its own u8 / u16 / u32 codes) and both paths (SBAG_WPRED_FORCE_FALLBACK
unset: the fused pass wherever plan_tiled allows it; "1": k_wpred_walk), and is also held to
the composed path the models ran before: nat.predict(per_tree=True) plus the host loop."""
import os
from fractions import Fraction

import numpy as np
import pytest

import boosting_ref as br
import oracle
import predict_ref as ref
import weighted_ref as wr
from conftest import DATA

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

KNOB = "SBAG_WPRED_FORCE_FALLBACK"


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def same_bits(got, want):
    np.testing.assert_array_equal(got, want)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.signbit(got)[ok], np.signbit(want)[ok])


def run_all(ctx, f, X, ds, kind, w, nc, monkeypatch):
    """[(label, output)] of both entry points on both paths."""
    outs = []
    for force in (None, "1"):
        if force is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, force)
        outs.append((f"host rows, force={force}", nat.predict_weighted(ctx, f, X, kind, w, nc)))
        if ds is not None:
            outs.append((f"dataset, force={force}", nat.predict_weighted_dataset(ctx, f, ds, kind, w, nc)))
    monkeypatch.delenv(KNOB, raising=False)
    return outs


def check(ctx, monkeypatch, trees, subs, X, kind, w, nc, *, gini=False, code_bytes=None, pt=None,
          dataset=True):
    X = np.ascontiguousarray(X, np.float64)
    if pt is None:
        pt = ref.per_tree(trees, subs, X)
    rule = wr.dot if kind == nat.W_DOT else wr.cls
    want = rule(pt, w, nc)
    f = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_GINI if gini else nat.IMPURITY_VARIANCE)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx) if dataset else None
    try:
        if code_bytes is not None:
            assert ds.layout()[3] == code_bytes
        _, ptg = nat.predict(ctx, f, X, nat.AGG_MODE if gini else nat.AGG_MEAN, per_tree=True)
        same_bits(rule(ptg, w, nc), want)  # the composed path
        for label, got in run_all(ctx, f, X, ds, kind, w, nc, monkeypatch):
            assert got.shape == want.shape, label
            try:
                same_bits(got, want)
            except AssertionError as e:
                raise AssertionError(f"{label}: {e}") from None
    finally:
        if ds is not None:
            ds.free()
        f.free()
    return want


# ---------------------------------------------------------------- tile and thread edges
def _uneven_forest(depth=30):
    """A right-deep and a left-deep comb of depth 3 and of `depth`, every leaf its own value."""
    trees, nxt = [], 0
    for n in (3, depth):
        for left_deep in (False, True):
            thr = np.arange(n)[::-1] if left_deep else np.arange(n)
            trees.append(wr.comb(thr, 0.25 + nxt + np.arange(n + 1), left_deep=left_deep))
            nxt += n + 1
    return trees


@pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 512, 513, 1300])
def test_tile_and_thread_edges(ctx, monkeypatch, N):
    """Thread t of a 512-row tile walks rows t and t + 256: of each pair one row leaves a comb
    at depth 1 and the other at its end, in both orders; N covers a lone row, a missing second
    row, a partial tile and two tiles plus a tail."""
    r = np.arange(N)
    deep = ((r % 512) // 256 + r % 256) % 2 == 0
    x = np.where(deep, 31.0, -1.0)
    x[r % 7 == 3] = (r[r % 7 == 3] * 5) % 30
    X = x[:, None]
    trees = _uneven_forest()
    w = [0.3, 1.7, -0.9, 2.1]
    check(ctx, monkeypatch, trees, [[0]] * 4, X, nat.W_DOT, w, 1, code_bytes=1)
    check(ctx, monkeypatch, trees, [[0]] * 4, X, nat.W_DOT, w, 2, code_bytes=1)
    cl = [wr.comb(np.arange(30), np.arange(31) % 3), wr.comb(np.arange(3)[::-1], [2, 0, 1, 2], left_deep=True),
          wr.stump(10.5, 1, 0)]
    check(ctx, monkeypatch, cl, [[0]] * 3, X, nat.W_CLASS, [0.7, 1.1, 0.4], 3, gini=True, code_bytes=1)


# ---------------------------------------------------------------- column counts
S_HOST, S_U8 = wr.host_stride(1), 16                 # one feature: host rows (u16), a u8 dataset
COLS_HOST = wr.max_tiled_cols(S_HOST, 2)
COLS_U8 = wr.max_tiled_cols(S_U8, 1)
assert wr.weighted_budget(S_HOST, 2, COLS_HOST + 1) is None and wr.weighted_budget(S_U8, 1, COLS_U8 + 1) is None
assert COLS_HOST > 9 and COLS_U8 > 9
COL_COUNTS = sorted({1, 2, 5, 8, 9, COLS_HOST, COLS_HOST + 1, COLS_U8, COLS_U8 + 1})


@pytest.mark.parametrize("nc", COL_COUNTS)
def test_column_counts(ctx, monkeypatch, nc):
    """num_cols from one (the regressors' register path) to the largest count whose [num_cols][512]
    fp64 accumulators plan_tiled still places beside the row tile and a chunk -- computed from
    its formulas for host rows and for a u8 dataset -- and one more, which takes the general
    path.  W_DOT over three iterations of num_cols trees; W_CLASS over min(num_cols, 4)
    classes, so from num_cols = 5 on the columns past the class count must stay +0.0."""
    N = 700
    X = ((np.arange(N) * 7) % 23).astype(np.float64)[:, None]
    rng = np.random.default_rng(nc)
    L = 3 * nc
    trees = [wr.stump(t % 22 + 0.5, rng.normal() * 3, rng.normal() * 3) if t % 4 else
             wr.comb(np.arange(0, 22, 3), rng.normal(size=9)) for t in range(L)]
    w = np.abs(rng.normal(size=L)) + 0.05
    check(ctx, monkeypatch, trees, [[0]] * L, X, nat.W_DOT, w, nc, code_bytes=1)
    C = min(nc, 4)
    cl = [wr.stump(t % 22 + 0.5, t % C, (t // 2 + 1) % C) for t in range(12)]
    cl[5] = wr.comb(np.arange(0, 22, 3), np.arange(9) % C)
    want = check(ctx, monkeypatch, cl, [[0]] * 12, X, nat.W_CLASS, np.resize(w, 12), nc, gini=True,
                 code_bytes=1)
    if nc > C:
        assert not want[:, C:].any() and not np.signbit(want[:, C:]).any()
        assert want[:, :C].any()


# ---------------------------------------------------------------- chunks
def _chunk_forest(L, classes=0):
    rng = np.random.default_rng(L)
    trees = []
    for t in range(L):
        thr = np.sort(rng.permutation(1000)[:255]) / 4.0
        leaves = rng.integers(0, classes, 256) if classes else rng.normal(size=256) * 3 + 0.1
        trees.append(wr.comb(thr, leaves, left_deep=bool(t % 2)))
    return trees


@pytest.mark.parametrize("kind,L", [(nat.W_CLASS, 40), (nat.W_DOT, 42)], ids=["class40", "dot42"])
def test_chunk_boundary_inside_an_iteration(ctx, monkeypatch, kind, L):
    """Trees of 255 internal nodes each, num_cols = 3: the plan spans at least 3 chunks and a
    chunk holds a tree count that is no multiple of 3, so the column of W_DOT runs on across a
    chunk boundary.  40 trees are no multiple of 3, which W_DOT refuses: the 40 go through
    W_CLASS and W_DOT takes 42, the next multiple."""
    gini = kind == nat.W_CLASS
    trees = _chunk_forest(L, 3 if gini else 0)
    assert all(wr.n_internal(t) == 255 for t in trees)
    sizes = [wr.tree_bytes(255)] * L
    for S, cb in ((S_HOST, 2), (S_U8, 1)):
        chunks = wr.plan_chunks(sizes, wr.weighted_budget(S, cb, 3))
        assert len(chunks) >= 3
        assert any((b - a) % 3 for a, b in chunks[:-1])
    X = (np.random.default_rng(1).integers(0, 250, size=(700, 1)) * 1.0)
    w = np.abs(np.random.default_rng(2).normal(size=L)) + 0.05
    check(ctx, monkeypatch, trees, [[0]] * L, X, kind, w, 3, gini=gini, code_bytes=1)


# ---------------------------------------------------------------- order and rounding
def _order_case():
    rng = np.random.default_rng(7)
    trees = []
    for t in range(24):
        if t % 3 == 0:
            trees.append(wr.comb(np.arange(0, 40, 5), rng.normal(size=9) * 3 + 0.1))
        else:
            trees.append(wr.stump(t * 1.5 + 0.5, rng.normal() * 3 + 0.1, rng.normal() * 3 + 0.1))
    w = np.abs(rng.normal(size=24)) + 0.05
    X = rng.integers(0, 40, size=(1300, 1)) * 1.0
    return trees, w, X


def _unrounded_dot(pt, w):
    """The sum with the exact product added: s = fl(s + p * w), one rounding a step."""
    out = np.zeros(pt.shape[1])
    for r in range(pt.shape[1]):
        s = 0.0
        for t in range(pt.shape[0]):
            s = float(Fraction(s) + Fraction(float(pt[t, r])) * Fraction(float(w[t])))
        out[r] = s
    return out


def test_order_and_rounding(ctx, monkeypatch):
    """Leaf values normal * 3 + 0.1, weights |normal| + 0.05, 24 trees, 1300 rows.  The inputs
    discriminate (asserted before the GPU runs): the reversed-order sum differs from the
    in-order sum on 1155 of the 1300 rows, and a sum that adds the exact product differs on 230
    of the first 300 (this forest, seed 7).  Then weights 1e16, 1, -1e16, 1, ... over the same
    trees and over single-leaf trees of 1.0."""
    trees, w, X = _order_case()
    subs = [[0]] * 24
    pt = ref.per_tree(trees, subs, X)
    fwd = wr.dot(pt, w)[:, 0]
    rev = wr.dot(pt[::-1], w[::-1])[:, 0]
    unr = _unrounded_dot(pt[:, :300], w)
    n_rev, n_unr = int((fwd != rev).sum()), int((fwd[:300] != unr).sum())
    print(f"reversed order differs on {n_rev} of 1300 rows, unrounded product on {n_unr} of 300")
    assert n_rev > 0 and n_unr > 0
    check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 1, pt=pt, code_bytes=1)
    check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 4, pt=pt, code_bytes=1)
    big = np.array([1e16, 1.0, -1e16, 1.0] * 6)
    want = check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, big, 1, pt=pt, code_bytes=1)
    assert (want[:, 0] != wr.dot(pt[::-1], big[::-1])[:, 0]).any()
    ones = [wr.leaf(1.0)] * 24
    want = check(ctx, monkeypatch, ones, subs, X[:600], nat.W_DOT, big, 1, code_bytes=1)
    assert (want == 1.0).all()  # ((((1e16 + 1) - 1e16) + 1) ...: not the exact sum 12
    zero = [wr.leaf(0.0)] * 24
    want = check(ctx, monkeypatch, zero, subs, X[:600], nat.W_CLASS, big, 2, gini=True, code_bytes=1)
    assert (want[:, 0] == 1.0).all() and not want[:, 1].any()


# ---------------------------------------------------------------- special values
def test_special_values(ctx, monkeypatch):
    """A -0.0 leaf and a -0.0 weight (0.0 + -0.0 is +0.0: compared by sign bit too); a NaN
    leaf and infinite weights (inf * 0.0, inf - inf): the NaN positions must match."""
    X = (np.arange(600) % 4).astype(np.float64)[:, None]
    trees = [wr.stump(0.5, -0.0, 1.0), wr.stump(1.5, 2.0, -0.0), wr.stump(2.5, np.nan, 0.0),
             wr.stump(0.5, 0.0, -3.0), wr.leaf(-0.0), wr.stump(1.5, 1.0, -1.0)]
    subs = [[0]] * 6
    for w in ([1.0, -0.0, 1.0, np.inf, 2.0, -0.0], [-0.0] * 6, [np.inf, 1.0, 1.0, -np.inf, 1.0, np.inf],
              [np.nan, 1.0, 0.0, 1.0, 1.0, 1.0]):
        for nc in (1, 2, 3):
            want = check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, nc, code_bytes=1)
            assert not np.signbit(want[~np.isnan(want) & (want == 0)]).any()
    want = check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, [1.0, -0.0, 1.0, np.inf, 2.0, -0.0], 1)
    assert np.isnan(want).any() and not np.isnan(want).all()
    cl = [wr.stump(0.5, 0, 1), wr.stump(1.5, 1, 2), wr.stump(2.5, 0, 2), wr.leaf(1)]
    for w in ([-0.0, -0.0, -0.0, -0.0], [np.inf, 1.0, -np.inf, 2.0], [1.0, np.nan, 1.0, -0.0]):
        check(ctx, monkeypatch, cl, [[0]] * 4, X, nat.W_CLASS, w, 4, gini=True, code_bytes=1)


# ---------------------------------------------------------------- code widths, subspaces
def _width_forest(F, rng, top):
    trees = [wr.stump(rng.integers(0, top) + 0.5, rng.normal(), rng.normal(), feature=t % F) for t in range(9)]
    trees += [wr.comb(np.sort(rng.permutation(top)[:20]) + 0.25, rng.normal(size=21), feature=np.arange(20) % F)
              for _ in range(3)]
    return trees, [list(range(F))] * 12


@pytest.mark.parametrize("distinct,cb,N", [(200, 1, 1300), (300, 2, 1300), (65600, 4, 70000)],
                         ids=["u8", "u16", "u32"])
def test_code_widths(ctx, monkeypatch, distinct, cb, N):
    """A u8 dataset, a u16 dataset (a feature of 300 distinct values) and a u32 dataset (70 000
    rows x 2 features, 65 600 distinct values in one: the general path whatever the knob)."""
    rng = np.random.default_rng(distinct)
    X = np.column_stack([rng.permutation(N) % distinct, rng.integers(0, 50, N)]).astype(np.float64)
    assert len(np.unique(X[:, 0])) == distinct
    trees, subs = _width_forest(2, rng, min(distinct, 60000))
    w = np.abs(rng.normal(size=12)) + 0.05
    check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 1, code_bytes=cb)
    check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 3, code_bytes=cb)
    cl = [wr.stump(rng.integers(0, 50) + 0.5, t % 3, (t + 1) % 3, feature=t % 2) for t in range(7)]
    check(ctx, monkeypatch, cl, [[0, 1]] * 7, X, nat.W_CLASS, w[:7], 3, gini=True, code_bytes=cb)


def test_host_rows_in_batches(ctx, monkeypatch):
    """Host rows with SBAG_PREDICT_BATCH_ROWS=300 at N = 1300: four whole batches and a tail of
    100, each batch's block of out at its own offset (num_cols 1 and 5)."""
    rng = np.random.default_rng(11)
    X = rng.integers(0, 60, size=(1300, 3)) * 0.5
    trees, subs = _width_forest(3, rng, 30)
    w = np.abs(rng.normal(size=12)) + 0.05
    one = check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 1, dataset=False)
    monkeypatch.setenv("SBAG_PREDICT_BATCH_ROWS", "300")
    assert np.array_equal(check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, w, 1, dataset=False), one)
    trees15 = trees + trees[:3]
    check(ctx, monkeypatch, trees15, subs + subs[:3], X, nat.W_DOT, np.r_[w, w[:3]], 5, dataset=False)
    cl = [wr.stump(t + 0.5, t % 4, (t + 2) % 4, feature=t % 3) for t in range(8)]
    check(ctx, monkeypatch, cl, [[0, 1, 2]] * 8, X, nat.W_CLASS, w[:8], 6, gini=True, dataset=False)


def test_trees_with_different_subspaces(ctx, monkeypatch):
    """Trees over the subspaces [0, 2] and [1], as GBM's boosters have: a node's feature
    indexes its own tree's subspace."""
    rng = np.random.default_rng(3)
    X = rng.integers(0, 20, size=(700, 3)) * 1.0
    a = wr.comb([3.5, 9.5, 14.5], [1.0, 2.0, 3.0, 4.0], feature=[0, 1, 0])  # global 0, 2, 0
    b = wr.stump(7.5, -1.0, 5.0, feature=1)                                  # global 2
    c = wr.stump(11.5, 0.5, -0.5, feature=0)                                 # global 1
    trees, subs = [a, c, b, c, a, b], [[0, 2], [1], [0, 2], [1], [0, 2], [0, 2]]
    want = check(ctx, monkeypatch, trees, subs, X, nat.W_DOT, [0.5, 1.5, 2.5, 3.5, 4.5, 5.5], 2, code_bytes=1)
    wrong = wr.dot(ref.per_tree(trees, [[0, 1, 2]] * 6, X), [0.5, 1.5, 2.5, 3.5, 4.5, 5.5], 2)
    assert (want != wrong).any()  # the subspaces do matter here


# ---------------------------------------------------------------- errors
def test_every_einval_leaves_the_context_usable(ctx, monkeypatch):
    X = (np.arange(300) % 7).astype(np.float64)[:, None]
    X2 = np.column_stack([X[:, 0], X[:, 0]])
    var = nat.NativeForest.from_trees([wr.stump(2.5, 1.0, 2.0)] * 6, [[0]] * 6, nat.IMPURITY_VARIANCE)
    gin = nat.NativeForest.from_trees([wr.stump(2.5, 0, 2)] * 6, [[0]] * 6, nat.IMPURITY_GINI)
    far = nat.NativeForest.from_trees([wr.stump(2.5, 1.0, 2.0, feature=1)] * 6, [[0, 5]] * 6,
                                      nat.IMPURITY_VARIANCE)
    ds = nat.DeviceDataset.from_numpy(X2, np.zeros(300), ctx)
    w = np.arange(6) + 1.0
    good = wr.dot(ref.per_tree([wr.stump(2.5, 1.0, 2.0)] * 6, [[0]] * 6, X), w, 2)
    lib = nat.lib()

    def still_usable():
        np.testing.assert_array_equal(nat.predict_weighted(ctx, var, X2, nat.W_DOT, w, 2), good)
        np.testing.assert_array_equal(nat.predict_weighted_dataset(ctx, var, ds, nat.W_DOT, w, 2), good)

    def refused(forest, kind, weights, nc, rows=X2, dataset=ds):
        weights = np.asarray(weights, np.float64)
        out = np.full((300, max(nc, 1)), 7.0)
        for call in (lambda: lib.sbag_predict_weighted(ctx.handle, forest.handle, nat.ptr(rows), 300,
                                                       rows.shape[1], kind, nat.ptr(weights), len(weights), nc,
                                                       nat.ptr(out)),
                     lambda: lib.sbag_predict_weighted_dataset(ctx.handle, forest.handle, dataset.handle, kind,
                                                               nat.ptr(weights), len(weights), nc, nat.ptr(out))):
            assert call() == nat.SBAG_EINVAL
            assert (out == 7.0).all()  # nothing written
            still_usable()

    try:
        still_usable()
        out = np.full((300, 2), 7.0)
        full = [ctx.handle, var.handle, nat.ptr(X2), 300, 2, nat.W_DOT, nat.ptr(w), 6, 2, nat.ptr(out)]
        for null in (0, 1, 2, 6, 9):  # a null argument
            a = list(full)
            a[null] = None
            assert lib.sbag_predict_weighted(*a) == nat.SBAG_EINVAL
            still_usable()
        dfull = [ctx.handle, var.handle, ds.handle, nat.W_DOT, nat.ptr(w), 6, 2, nat.ptr(out)]
        for null in (0, 1, 2, 4, 7):
            a = list(dfull)
            a[null] = None
            assert lib.sbag_predict_weighted_dataset(*a) == nat.SBAG_EINVAL
            still_usable()
        assert (out == 7.0).all()
        refused(var, 2, w, 2)                     # an unknown kind
        refused(var, -1, w, 2)
        refused(var, nat.W_DOT, w[:5], 1)         # num_weights != tree count
        refused(var, nat.W_DOT, np.r_[w, 1.0], 1)
        refused(var, nat.W_DOT, w, 0)             # num_cols < 1
        refused(var, nat.W_DOT, w, -3)
        refused(var, nat.W_DOT, w, 4)             # 6 trees are no multiple of 4
        refused(var, nat.W_CLASS, w, 3)           # W_CLASS on a forest that is not gini
        refused(gin, nat.W_CLASS, w, 2)           # num_cols below the 3 classes
        refused(far, nat.W_DOT, w, 2)             # a subspace past the 2 features
        with pytest.raises(sb.IllegalArgumentException):
            nat.predict_weighted(ctx, var, X2, nat.W_DOT, w, 4)
        with pytest.raises(sb.IllegalArgumentException):
            nat.predict_weighted_dataset(ctx, gin, ds, nat.W_CLASS, w, 2)
        np.testing.assert_array_equal(nat.predict_weighted(ctx, gin, X2, nat.W_CLASS, w, 3),
                                      wr.cls(ref.per_tree([wr.stump(2.5, 0, 2)] * 6, [[0]] * 6, X), w, 3))
        assert nat.predict_weighted(ctx, var, np.zeros((0, 2)), nat.W_DOT, w, 2).shape == (0, 2)  # num_rows == 0
        if nat.device_count() >= 2:  # a dataset on another device (needs a second one to exist)
            other = nat.Context(1)
            try:
                out = np.full((300, 2), 7.0)
                assert lib.sbag_predict_weighted_dataset(other.handle, var.handle, ds.handle, nat.W_DOT,
                                                         nat.ptr(w), 6, 2, nat.ptr(out)) == nat.SBAG_EINVAL
                assert (out == 7.0).all()
            finally:
                other.close()
            still_usable()
    finally:
        ds.free()
        for f in (var, gin, far):
            f.free()


# ---------------------------------------------------------------- the four models
def _dense(X):
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X, np.float64)


@pytest.fixture(scope="module")
def cpusmall():
    X, y = sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))
    return _dense(X)[:1500], np.asarray(y, np.float64)[:1500]


@pytest.fixture(scope="module")
def vehicle():
    X, y = sb.load_libsvm(os.path.join(DATA, "vehicle.svm"))
    return _dense(X), np.asarray(y, np.float64)


@pytest.fixture
def resident(ctx, monkeypatch):
    """DeviceDatasets whose features() raises: a transform that downloads them fails."""
    made = []

    def make(X):
        ds = nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx)
        made.append(ds)
        return ds

    def no_features(self, *a, **k):
        raise AssertionError("the transform downloaded the dataset's features")

    monkeypatch.setattr(nat.DeviceDataset, "features", no_features)
    yield make
    for ds in made:
        ds.free()


def _no_per_tree(monkeypatch):
    real = nat.predict

    def guarded(ctx, forest, X, agg, per_tree=False):
        assert not per_tree, "the transform took the composed per-tree path"
        return real(ctx, forest, X, agg)

    monkeypatch.setattr(nat, "predict", guarded)


def test_gbm_regression_model(ctx, cpusmall, resident, monkeypatch, tmp_path):
    X, y = cpusmall
    kw = dict(num_base_learners=5, learning_rate=0.3, replacement=True, subspace_ratio=0.7, max_depth=3)
    model = sb.GBMRegressor().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(3)).fit(
        sb.Frame(X, y), params={"numBaseLearners": 5, "learningRate": 0.3, "replacement": True,
                                "subspaceRatio": 0.7})
    w, subs, trees, const = oracle.gbm_regressor_fit(X, y, **kw)
    assert model.weights == w and len(w) == 5
    want = oracle.gbm_predict(w, subs, trees, const, X)
    _no_per_tree(monkeypatch)
    np.testing.assert_array_equal(model.transform(X), want)
    np.testing.assert_array_equal(model.transform(resident(X)), want)
    model.save(str(tmp_path / "gbm"))
    back = sb.GBMRegressionModel.load(str(tmp_path / "gbm"))
    np.testing.assert_array_equal(back.transform(resident(X)), want)
    np.testing.assert_array_equal(back.transform(X), want)


def test_gbm_classification_model(ctx, vehicle, resident, monkeypatch):
    X, y = vehicle
    model = sb.GBMClassifier().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(3)).fit(
        sb.Frame(X, y), params={"numBaseLearners": 3, "learningRate": 0.5, "subspaceRatio": 0.7})
    K, w, subs, trees = oracle.gbm_classifier_fit(X, y, num_base_learners=3, learning_rate=0.5,
                                                  subspace_ratio=0.7, max_depth=3)
    assert model.numClasses == K == 5 and model.weights == w
    prob, votes = oracle.gbm_classifier_predict(K, w, subs, trees, X)
    _no_per_tree(monkeypatch)
    ds = resident(X)
    np.testing.assert_array_equal(model.predict_raw(X), prob)
    np.testing.assert_array_equal(model.predict_raw(ds), prob)
    np.testing.assert_array_equal(model.transform(X), votes)
    np.testing.assert_array_equal(model.transform(ds), votes)


def test_boosting_regression_model(ctx, cpusmall, resident, monkeypatch):
    X, y = cpusmall
    model = sb.BoostingRegressor().setNumBaseLearners(3).setBaseLearner(
        sb.DecisionTreeRegressor().setMaxDepth(3)).fit(sb.Frame(X, y))
    weights, trees, _, _ = br.boosting_fit(X, y, classification=False, num_base_learners=3, max_depth=3)
    assert model.weights == [float(v) for v in weights] and len(trees) == 3
    want = br.boosting_predict(weights, trees, X)[0]
    _no_per_tree(monkeypatch)
    np.testing.assert_array_equal(model.transform(X), want)
    np.testing.assert_array_equal(model.transform(resident(X)), want)


def test_boosting_classification_model(ctx, vehicle, resident, monkeypatch, tmp_path):
    X, y = vehicle
    model = sb.BoostingClassifier().setNumBaseLearners(4).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(3)).fit(sb.Frame(X, y))
    weights, trees, K, _ = br.boosting_fit(X, y, classification=True, num_base_learners=4, max_depth=3)
    assert model.weights == [float(v) for v in weights] and K == model.numClasses == 5
    want, want_raw = br.boosting_predict(weights, trees, X, K)
    _no_per_tree(monkeypatch)
    ds = resident(X)
    for m in (model,):
        np.testing.assert_array_equal(m.predict_raw(X), want_raw)
        np.testing.assert_array_equal(m.predict_raw(ds), want_raw)
        np.testing.assert_array_equal(m.transform(X), want)
        np.testing.assert_array_equal(m.transform(ds), want)
    model.save(str(tmp_path / "boost"))
    back = sb.BoostingClassificationModel.load(str(tmp_path / "boost"))
    np.testing.assert_array_equal(back.predict_raw(ds), want_raw)
    np.testing.assert_array_equal(back.transform(X), want)
