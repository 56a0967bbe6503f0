"""The resident boosting state of GBMRegressor (sbag_gbm_state, k_gbm_step) against NumPy fp64:
gbm.py's loss_function / grad_function and predict_ref's per-row tree walk, byte for byte, at
the edges of the step's row tile, on both sides of its LDS plan, with u8 and u16 codes."""
import functools
import os

import numpy as np
import pytest

import predict_ref
from conftest import DATA

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd import gbm

pytestmark = pytest.mark.gpu

WEIGHT, CONST, F = 0.1, 0.7, 6
LOSSES = [("squared", 0.9), ("absolute", 0.9), ("huber", 0.9), ("huber", 1.0 / 3.0), ("quantile", 0.9)]
ROWS = {"1": (0, 1), "T-1": (1, -1), "T": (1, 0), "T+1": (1, 1), "2T+3": (2, 3)}  # a T + b


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


@functools.lru_cache(maxsize=None)
def rows_of(n, wide):
    """Few distinct values per feature (u8 codes) or, `wide`, one continuous feature (u16)."""
    rng = np.random.default_rng(1000 + n + wide)
    X = np.round(rng.normal(size=(n, F)) * 5) / 3
    if wide:
        X[:, 2] = rng.normal(size=n)
    return X, rng.normal(size=n) * 3.1 + X[:, 0] / 7


@functools.lru_cache(maxsize=None)
def hand_tree(depth):
    """A full tree of `depth` in pre-order over all F features, non-dyadic leaf values."""
    rng = np.random.default_rng(depth)
    nodes = np.zeros(2 ** (depth + 1) - 1, nat.NODE_DTYPE)
    nodes["id"] = np.arange(len(nodes))
    nodes["left"] = nodes["right"] = nodes["feature"] = -1
    nodes["prediction"] = rng.normal(size=len(nodes)) / 3
    stack = [(0, 0)]
    while stack:
        i, d = stack.pop()
        if d == depth:
            continue
        size = 2 ** (depth - d) - 1  # nodes of a child's subtree
        nodes[i]["left"], nodes[i]["right"] = i + 1, i + 1 + size
        nodes[i]["feature"], nodes[i]["threshold"] = (i + d) % F, rng.normal() * 1.5
        stack += [(i + 1, d + 1), (i + 1 + size, d + 1)]
    return nodes


def reference(loss, alpha, mode, y, S, const):
    fn = (gbm.grad_function if mode == nat.GBM_RESIDUAL else gbm.loss_function)(loss, alpha)
    with np.errstate(all="ignore"):
        v = fn(y, S + const)
        return -v if mode == nat.GBM_RESIDUAL else v


@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("tree", ["leaf", "fit5", "deep"])
@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("loss,alpha", LOSSES)
def test_step_against_numpy(ctx, loss, alpha, rows, tree, wide):
    """S and the residuals / losses after create and after each of three steps."""
    n = ROWS[rows][0] * nat.gbm_plan(1)[0] + ROWS[rows][1]  # T: the plan's row tile
    X, y = rows_of(n, wide)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    states, forest = [], None
    try:
        if n > 256:
            assert ds.layout()[3] == (2 if wide else 1)  # code_bytes
        modes = (nat.GBM_RESIDUAL, nat.GBM_LOSS)
        states = [nat.GbmState.create(ctx, ds, loss, alpha, CONST, m) for m in modes]
        S = np.zeros(n)
        if tree != "fit5":
            nodes = hand_tree(0 if tree == "leaf" else 12)
            assert nat.gbm_plan(len(nodes))[1] == (tree == "leaf")
            sub = np.arange(F, dtype=np.int32)
            forest = nat.NativeForest.from_trees([nodes], [sub], nat.IMPURITY_VARIANCE)
        for step in range(4):
            for mode, st in zip(modes, states):
                got_S, got_v = st.read()
                assert np.array_equal(bits(got_S), bits(S)), (step, "S")
                assert np.array_equal(bits(got_v), bits(reference(loss, alpha, mode, y, S, CONST))), (step, mode)
            if step == 3:
                break
            if tree == "fit5":  # a proper subspace: local and dataset feature indices differ
                sub = np.array([1, 2, 4], np.int32)
                forest = states[0].fit_next(np.ones(n, np.uint8), sub, max_depth=5)
                nodes = forest.tree(0)[0]
            for st in states:
                st.advance(forest, WEIGHT)
            S = S + nodes["prediction"][predict_ref.walk(nodes, sub, X)] * WEIGHT
            if tree == "fit5":
                forest.free()
    finally:
        for h in states + [ds]:
            h.free()


@pytest.mark.parametrize("loss,alpha", LOSSES)
def test_edge_values(ctx, loss, alpha):
    """y - S = +0.0 and -0.0 (signum), p == y exactly (quantile), subnormal huber quotients:
    before and after a step of a stump with non-dyadic leaves."""
    stump = np.zeros(3, nat.NODE_DTYPE)
    stump["left"], stump["right"], stump["feature"] = [1, -1, -1], [2, -1, -1], [0, -1, -1]
    stump["threshold"], stump["prediction"] = [3.5, 0, 0], [0, 0.3, -0.7]
    y = np.array([0.0, -0.0, 1e-310, -3e-310, 5e-324, 0.3 * WEIGHT, -0.7 * WEIGHT, 1 / 3, 2.5e-308])
    X = np.arange(len(y), dtype=np.float64)[:, None]
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = nat.NativeForest.from_trees([stump], [np.zeros(1, np.int32)], nat.IMPURITY_VARIANCE)
    try:
        for mode in (nat.GBM_RESIDUAL, nat.GBM_LOSS):
            st = nat.GbmState.create(ctx, ds, loss, alpha, 0.0, mode)
            S = np.zeros(len(y))
            for step in range(2):
                got_S, got_v = st.read()
                want = reference(loss, alpha, mode, y, S, 0.0)
                assert np.array_equal(bits(got_S), bits(S)) and np.array_equal(bits(got_v), bits(want)), (mode, step)
                st.advance(forest, WEIGHT)
                S = S + stump["prediction"][predict_ref.walk(stump, [0], X)] * WEIGHT
            st.free()
    finally:
        ds.free()


@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_infinite_label_is_refused(ctx, loss):
    """y = inf reaches the residuals (huber: inf / inf = NaN) and the not-finite flag: fit_next
    refuses as fit_booster does, and the context serves the next call."""
    X, y = rows_of(300, False)
    y = y.copy()
    y[17] = np.inf
    counts, sub = np.ones(len(y), np.uint8), np.arange(F, dtype=np.int32)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    good = nat.DeviceDataset.from_numpy(*rows_of(300, False), ctx)
    st = nat.GbmState.create(ctx, ds, loss, 0.9, 0.0, nat.GBM_RESIDUAL)
    try:
        r = st.read()[1]
        assert not np.isfinite(r[17]) and np.isfinite(np.delete(r, 17)).all()
        with pytest.raises(nat.SparkException, match="booster labels must be finite") as e:
            st.fit_next(counts, sub)
        assert e.value.code == nat.SBAG_EUNSUPPORTED
        st2 = nat.GbmState.create(ctx, good, loss, 0.9, 0.0, nat.GBM_RESIDUAL)
        f = st2.fit_next(counts, sub)
        assert len(f.tree(0)[0]) > 1
        f.free()
        st2.free()
    finally:
        for h in (st, ds, good):
            h.free()


@pytest.mark.parametrize("labels", ["dyadic", "real", "large_integers"])
def test_fused_label_analysis(ctx, labels):
    """fit_next gives fit_booster's tree on the same residuals sent from the host, nodes and
    stats: the six fused reductions, the image and the engine they select."""
    rng = np.random.default_rng(17)
    n = 120_000 if labels == "large_integers" else 3000  # (test_booster_large_integer_labels' rows)
    X = np.round(rng.normal(size=(n, F)) * 3) / 3
    y = {"dyadic": np.round(rng.normal(size=n) * 8) / 4, "real": rng.normal(size=n) * 13.7,
         "large_integers": np.round(rng.normal(size=n) * 4e4 + 1e5 + X[:, 1] * 2e4)}[labels]
    counts = nat.sample(ctx, True, 1.0, 21, 0, 1, n)[0]
    sub = np.arange(F, dtype=np.int32)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    st = nat.GbmState.create(ctx, ds, "squared", 0.9, 0.0, nat.GBM_RESIDUAL)
    try:
        for step in range(2):
            r = st.read()[1]
            assert step or np.array_equal(bits(r), bits(y))
            f = st.fit_next(counts, sub, max_depth=6)
            g = nat.fit_booster(ctx, ds, r, counts, sub, max_depth=6)
            (fn, fs), (gn, gs) = f.tree(0), g.tree(0)
            assert len(fn) > 1 and fn.tobytes() == gn.tobytes() and bits(fs).tobytes() == bits(gs).tobytes()
            st.advance(f, WEIGHT)
            f.free()
            g.free()
    finally:
        st.free()
        ds.free()


def host_loop_fit(est, X, y, vmask):
    """GBMRegressor._train as it ran with S and the residuals in NumPy (one partition)."""
    ctx, bl = nat.default_context(0), sb.DecisionTreeRegressor()
    Xt, yt, Xv, yv = X[~vmask], y[~vmask], X[vmask], y[vmask]
    L, lr = est.getNumBaseLearners(), est.getLearningRate()
    lossf = gbm.loss_function(est.getLoss(), est.getAlpha())
    grad = gbm.grad_function(est.getLoss(), est.getAlpha())
    ds = nat.DeviceDataset.from_numpy(Xt, yt, ctx)
    counts = nat.sample(ctx, est.getReplacement(), est.getSampleRatio(), est.getSeed(), 0, L, len(yt))
    weights, subs, trees = [], [], []
    S, SV = np.zeros(len(yt)), np.zeros(len(yv))
    it, error, num_try, seed = L, gbm.DOUBLE_MAX, 0, est.getSeed()
    while it != 0:
        sub = nat.subspace(est.getSubspaceRatio(), X.shape[1], seed)
        f = nat.fit_booster(ctx, ds, -grad(yt, S + 0.0), counts[L - it], sub, max_depth=bl.getMaxDepth(),
                            max_bins=bl.getMaxBins(), tree_seed=bl.getSeed())
        trees.append(f.tree(0))
        S = S + nat.predict_dataset(ctx, f, ds, nat.AGG_MEAN) * lr
        SV = SV + nat.predict(ctx, f, Xv, nat.AGG_MEAN) * lr
        f.free()
        weights.append(lr)
        subs.append(sub)
        old_it = it
        it, error, num_try = gbm.terminate(lr, lr, True, error, gbm.seq_sum(lossf(yv, SV + 0.0)), est.getTol(),
                                           est.getNumRound(), num_try, it)
        seed = seed + old_it
    ds.free()
    keep = len(trees) - num_try
    return weights[:keep], subs[:keep], trees[:keep]


@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_estimator_matches_host_loop(loss):
    """The resident fit keeps the host loop's boosters, weights, subspaces and early stop."""
    X, y = sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))
    X, y = np.asarray(X, np.float64)[:400], y[:400]
    vmask = np.arange(len(y)) % 4 == 3
    L = 20
    est = (sb.GBMRegressor().setNumBaseLearners(L).setLearningRate(0.5).setTol(0.1).setLoss(loss)
           .setValidationIndicatorCol("val").set("numRound", 2).set("subspaceRatio", 0.7)
           .set("sampleRatio", 0.8).set("replacement", True))
    model = est.fit((X, y), validation=vmask)
    weights, subs, trees = host_loop_fit(est, X, y, vmask)
    assert 0 < len(trees) < L  # early stopping made the decision
    assert model.weights == weights and model.numBaseModels == len(trees)
    for m, s, (nodes, stats), ms in zip(model.models, subs, trees, model.subspaces):
        assert np.array_equal(ms, s) and m.nodes.tobytes() == nodes.tobytes()
        assert bits(m.stats).tobytes() == bits(stats).tobytes()
