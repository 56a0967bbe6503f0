"""GPU: sbag_proximity_topk(_dataset) and model.nearestNeighbors, integer for integer against a
stable descending argsort of proximity_ref's counts under the key cnt * 2^32 + (2^32 - 1 - j):
host rows and datasets, both stage-A paths, and SBAG_PROX_TOPK_RUN (column blocks a run) where a
case needs several runs at a small size."""
import numpy as np
import pytest

import proximity_ref as pr
from test_gpu_proximity import BM, BN, FORESTS, KNOB, ctx, features, fitted, forest17  # noqa: F401 (fixtures)

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

RUN = "SBAG_PROX_TOPK_RUN"


def topk_ref(cnt, k, self_offset=-1):
    nq, nr = cnt.shape
    key = cnt.astype(np.int64) * 2**32 + (2**32 - 1 - np.arange(nr))
    idx, top = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.uint16)
    for i in range(nq):
        order = np.argsort(-key[i], kind="stable")
        order = order[order != i + self_offset][:k] if self_offset >= 0 else order[:k]
        idx[i, :len(order)], top[i, :len(order)] = order, cnt[i, order]
    return idx, top


def check(ctx, monkeypatch, f, Xq, Xr, k, self_offset=-1, repeat=1, run=None):
    """The top k of `repeat` copies of Xq against Xr: host rows and (with reference rows)
    datasets, stage-A fallback off and on, all equal to the reference, which is returned."""
    trees, subs = [f.tree(t)[0] for t in range(len(f))], [f.subspace(t) for t in range(len(f))]
    cnt = pr.counts(pr.leaves(trees, subs, Xq), pr.leaves(trees, subs, Xr))
    want = tuple(np.tile(a, (repeat, 1)) for a in topk_ref(cnt, k, self_offset))
    Xq = np.ascontiguousarray(np.tile(Xq, (repeat, 1)))
    ds = [nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx) for X in (Xq, Xr)] if len(Xr) else []
    monkeypatch.delenv(RUN, raising=False) if run is None else monkeypatch.setenv(RUN, str(run))
    try:
        for force in (None, "1"):
            monkeypatch.delenv(KNOB, raising=False) if force is None else monkeypatch.setenv(KNOB, force)
            got = {"host": nat.proximity_topk(ctx, f, Xq, Xr, k, self_offset)}
            if ds:
                got["dataset"] = nat.proximity_topk_dataset(ctx, f, ds[0], ds[1], k, self_offset)
            for label, (idx, top) in got.items():
                assert idx.dtype == np.int32 and top.dtype == np.uint16
                np.testing.assert_array_equal(idx, want[0], err_msg=f"indices, {label}, force={force}, run={run}")
                np.testing.assert_array_equal(top, want[1], err_msg=f"counts, {label}, force={force}, run={run}")
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        monkeypatch.delenv(RUN, raising=False)
        for d in ds:
            d.free()
    return want


@pytest.mark.parametrize("nq", [1, BM + 1])
@pytest.mark.parametrize("k", [1, 2, 10, 63, 64])
def test_k_and_reference_edges(ctx, monkeypatch, forest17, k, nq):
    """Fewer references than k (tails; none at all for k = 1), exactly k, one short of a column
    block and one past it, and three blocks."""
    X, f = forest17
    for nr in sorted({1, k - 1, k, BN - 1, BN + 1, 300}):
        idx, _ = check(ctx, monkeypatch, f, X[:nq], X[300 - nr:] if nr else X[:0], k)
        assert ((idx >= 0).sum(1) == min(k, nr)).all()


@pytest.mark.parametrize("self_offset", [-1, 3])
@pytest.mark.parametrize("name", ["root-only", "same-value"])
def test_ties_of_hand_built_forests(ctx, monkeypatch, name, self_offset):
    """Every count equal (the result is 0 ... k - 1, skipping the excluded row), and counts in
    {0, 1, 2}."""
    X = np.arange(300.0)[:, None]
    trees = FORESTS[name]()
    f = nat.NativeForest.from_trees(trees, [[0]] * len(trees), nat.IMPURITY_VARIANCE)
    try:
        idx, top = check(ctx, monkeypatch, f, X, np.ascontiguousarray(X[::-1][:140]), 10, self_offset)
        if name == "root-only":
            assert (top == 1).all() and (idx[299] == np.arange(10)).all()
            assert (idx[2] == ([0, 1, 2, 3, 4, 6, 7, 8, 9, 10] if self_offset == 3 else np.arange(10))).all()
    finally:
        f.free()


@pytest.mark.parametrize("run", [1, 2, None])
@pytest.mark.parametrize("nq", [1, 300])
def test_tiled_references_and_runs(ctx, monkeypatch, forest17, nq, run):
    """3 000 references that repeat 300 rows: exact ties 300 columns apart, across column blocks
    and, with 24 or 12 runs, across the lists that k_topk_merge joins; the smaller j wins."""
    X, f = forest17
    idx, top = check(ctx, monkeypatch, f, X[:nq], np.tile(X, (10, 1)), 10, run=run)
    assert (top == 17).all()  # the ten copies of the row itself, at least


@pytest.mark.parametrize("k", [10, 64])
def test_staging_overflow(ctx, monkeypatch, forest17, k):
    """References ordered so that the counts of query 0 rise with j: every column of every tile
    beats its bound, so the staging area fills and merges many times inside a tile."""
    X, f = forest17
    trees, subs = [f.tree(t)[0] for t in range(17)], [f.subspace(t) for t in range(17)]
    Xr = np.tile(X, (10, 1))
    order = np.argsort(pr.counts(pr.leaves(trees, subs, X[:1]), pr.leaves(trees, subs, Xr))[0], kind="stable")
    check(ctx, monkeypatch, f, X[:BM + 1], np.ascontiguousarray(Xr[order]), k)


@pytest.mark.parametrize("lo,hi,self_offset", [(0, 300, 0), (100, 229, 100), (100, 229, 400)])
def test_self_exclusion(ctx, monkeypatch, forest17, lo, hi, self_offset):
    """Queries that are a slice of the references: with the slice's offset no row is its own
    neighbour; without it, or with an offset past the references, the best count is the trees'."""
    X, f = forest17
    idx, top = check(ctx, monkeypatch, f, X[lo:hi], X, 10, self_offset)
    plain = topk_ref(pr.counts(*[pr.leaves([f.tree(t)[0] for t in range(17)], [f.subspace(t) for t in range(17)], Z)
                                 for Z in (X[lo:hi], X)]), 10)
    assert (plain[1][:, 0] == 17).all()
    if self_offset < 300:
        assert (idx != np.arange(lo, hi)[:, None]).all()
    else:
        assert np.array_equal(idx, plain[0]) and np.array_equal(top, plain[1])


@pytest.mark.parametrize("case", ["chain-300", "129-trees"])
def test_u16_codes_and_a_second_chunk(ctx, monkeypatch, case):
    if case == "chain-300":
        X = np.arange(300.0)[:, None]
        trees = FORESTS[case]()
        f = nat.NativeForest.from_trees(trees, [[0]] * len(trees), nat.IMPURITY_VARIANCE)
    else:
        X = features(np.random.default_rng(129), 300, 6, 1)
        f = fitted(ctx, X, 129)
    try:
        check(ctx, monkeypatch, f, X, np.ascontiguousarray(X[::-1][:140]), 10)
    finally:
        f.free()


def test_query_batches(ctx, monkeypatch, forest17):
    """110 copies of 300 queries are 33 000 rows: two batches; 7 references leave tails."""
    X, f = forest17
    check(ctx, monkeypatch, f, X, X[293:], 10, repeat=110)


@pytest.mark.parametrize("case", ["k=0", "k=65", "self_offset=-2", "null"])
def test_refusals_leave_the_context_usable(ctx, forest17, case):
    X, f = forest17
    lib, P = nat.lib(), nat.ptr
    idx, top = np.full((300, 64), 7, np.int32), np.full((300, 64), 7, np.uint16)
    k, off, out = {"k=0": (0, -1, P(top)), "k=65": (65, -1, P(top)), "self_offset=-2": (10, -2, P(top)),
                   "null": (10, -1, None)}[case]
    rc = lib.sbag_proximity_topk(ctx.handle, f.handle, P(X), 300, 6, P(X), 300, 6, k, off, P(idx), out)
    assert rc == nat.SBAG_EINVAL and (idx == 7).all() and (top == 7).all()
    assert (nat.proximity_topk(ctx, f, X, X, 1)[1] == 17).all()
    assert nat.proximity_topk(ctx, f, X[:0], X, 3)[0].shape == (0, 3)


def test_nearest_neighbors():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(200, 4))
    y = (X[:, 0] + X[:, 1] + 0.5 * rng.normal(size=200) > 0).astype(np.float64)
    model = sb.BaggingClassifier().setNumBaseLearners(50).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(5)).fit(sb.Frame(X, y))
    cnt = pr.counts(*[pr.leaves([m.nodes for m in model.models], model.subspaces, X)] * 2)
    want_idx, want_cnt = topk_ref(cnt, 5, 0)
    idx, prox = model.nearestNeighbors(X, k=5)
    assert idx.dtype == np.int32 and prox.dtype == np.float64
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(prox, want_cnt / 50.0)
    idx, prox = model.nearestNeighbors(X, X, excludeSelf=False)
    assert idx.shape == (200, 10) and (prox[:, 0] == 1.0).all()
