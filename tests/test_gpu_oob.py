"""GPU: out-of-bag predictions (sbag_predict_oob) against the CPU oracle.

Expected values are composed in the test from the oracle's own pieces: oracle.bag (the
counts), oracle.predict(per_tree=True) on the oracle's forest, and a row-by-row Python
loop that follows the rule literally: row r is out of bag for learner i iff
counts[i][r] == 0; regression: s = 0.0, s = s + tree_i(row) in learner order, s / n_oob;
classification: breeze's mode of the out-of-bag votes in learner order (the first class to
reach the final maximum count); NaN where n_oob == 0.  Everything is compared bit for bit
(assert_array_equal treats NaNs as equal).
"""
import numpy as np
import pytest

import oracle
from parity_utils import oracle_forest

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_metrics

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def oob_by_rows(counts, per_tree, cls):
    """The rule, literally, one row at a time: (pred, n_oob)."""
    L, N = counts.shape
    pred = np.full(N, np.nan)
    n_oob = np.zeros(N, np.int32)
    ct, pt = counts.T.tolist(), np.ascontiguousarray(per_tree.T).tolist()
    for r in range(N):
        votes = [pt[r][i] for i in range(L) if ct[r][i] == 0]
        n_oob[r] = len(votes)
        if not votes:
            continue
        if cls:
            final = {}
            for v in votes:
                final[v] = final.get(v, 0) + 1
            top = max(final.values())
            run = {}
            for v in votes:
                run[v] = run.get(v, 0) + 1
                if run[v] == top:
                    pred[r] = v
                    break
        else:
            s = 0.0
            for v in votes:
                s = s + v
            pred[r] = s / float(len(votes))
    return pred, n_oob


def oob_vectorised(counts, votes, cls):
    """The same rule with the learner loop outside (numpy over rows), for large N."""
    L, N = counts.shape
    n_oob = (counts == 0).sum(axis=0).astype(np.int32)
    rows = np.arange(N)
    if cls:
        C = int(votes.max()) + 1
        cnt = np.zeros((C, N), np.int32)
        best = np.zeros(N, np.int32)
        acc = np.full(N, np.nan)
        for i in range(L):
            oob = counts[i] == 0
            v = votes[i].astype(np.int64)
            k = cnt[v, rows] + 1
            cnt[v[oob], rows[oob]] = k[oob]
            upd = oob & (k > best)
            best = np.where(upd, k, best)
            acc = np.where(upd, votes[i], acc)
        return acc, n_oob
    s = np.zeros(N)
    for i in range(L):
        s = np.where(counts[i] == 0, s + votes[i], s)
    with np.errstate(invalid="ignore", divide="ignore"):
        pred = np.where(n_oob > 0, s / n_oob.astype(np.float64), np.nan)
    return pred, n_oob


def fit_native(ctx, ds, *, cls, replacement, ratio, seed, lb, L, depth, part, bins=32):
    return nat.fit(ctx, ds, replacement=replacement, sample_ratio=ratio, seed=seed, learner_begin=lb,
                   learner_end=lb + L, partition_offsets=part, max_depth=depth, max_bins=bins,
                   impurity=nat.IMPURITY_GINI if cls else nat.IMPURITY_VARIANCE)


def oracle_side(X, y, *, cls, replacement, ratio, seed, lb, L, depth, part, bins=32):
    """(oracle forest, counts, per-tree predictions, plain transform)."""
    N, F = X.shape
    counts = oracle.bag(replacement, ratio, lb, lb + L, seed, part, N)
    subs = [oracle.subspace(ratio, F, seed + i) for i in range(lb, lb + L)]
    orf = oracle_forest(X, y, counts, subs, depth, bins, cls, part=part)
    plain, per_tree = oracle.predict(orf, X, cls, per_tree=True)
    return orf, counts, per_tree, plain


def native_oob(ctx, forest, ds, *, cls, replacement, ratio, seed, lb, L, part, **_):
    return nat.predict_oob(ctx, forest, ds, replacement=replacement, sample_ratio=ratio, seed=seed,
                           learner_begin=lb, learner_end=lb + L, partition_offsets=part,
                           agg=nat.AGG_MODE if cls else nat.AGG_MEAN)


def assert_oob_equal(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    assert got[1].dtype == np.int32
    np.testing.assert_array_equal(got[0], want[0])


def tree_bytes(orf):
    """8 * (nodes + leaves) of every tree: what the LDS-tiled plan stages per tree."""
    out = []
    for t in range(orf.nodes.shape[0]):
        nodes, _ = orf.tree(t)
        out.append(8 * (len(nodes) + int((nodes["left"] < 0).sum())))
    return out


# ---------------------------------------------------------------- 1. sampler regimes x impurity
N1, F1 = 1300, 9  # two full 512-row tiles + a 276-row tail (the last tile's second walk partly empty)
PART1 = [0, 300, 300, 811, 1300]  # an empty partition; boundaries off the 256-row sampler blocks
REGIMES = [(True, 1.0, 8, 0), (False, 0.5, 8, 0), (True, 0.63, 5, 3), (False, 1.0, 3, 0)]


@pytest.fixture(scope="module")
def data1():
    rng = np.random.default_rng(11)
    X = np.round(rng.normal(size=(N1, F1)) * 6) / 8  # u8 codes
    kc = rng.integers(0, 3, N1)
    kr = rng.integers(-400, 400, N1)
    return X, {False: kr / 16 + X[:, 0] / 4, True: ((np.floor(3 * np.abs(X[:, 0])) + kc) % 7).astype(np.float64)}


_cases1 = {}


def case1(ctx, data1, regime, cls):
    """One fit of a regime on both sides, shared by the tests that use it."""
    key = (regime, cls)
    if key not in _cases1:
        X, ys = data1
        replacement, ratio, L, lb = regime
        p = dict(cls=cls, replacement=replacement, ratio=ratio, seed=SEED_CLS if cls else SEED_REG, lb=lb,
                 L=L, depth=6, part=PART1)
        ds = nat.DeviceDataset.from_numpy(X, ys[cls], ctx)
        assert ds.layout()[3] == 1
        forest = fit_native(ctx, ds, **p)
        _, counts, per_tree, plain = oracle_side(X, ys[cls], **p)
        _cases1[key] = (ds, forest, p, oob_by_rows(counts, per_tree, cls), plain)
    return _cases1[key]


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
def test_sampler_regimes(ctx, data1, regime, cls):
    ds, forest, p, want, plain = case1(ctx, data1, regime, cls)
    covered = want[1] > 0
    if regime == (False, 1.0, 3, 0):  # every count is 1: no row is ever out of bag; not an error
        assert not covered.any() and np.isnan(want[0]).all()
    else:
        assert covered.any() and (~covered).any()
        assert (want[0][covered] != plain[covered]).sum() >= 100
    assert_oob_equal(native_oob(ctx, forest, ds, **p), want)


@pytest.mark.parametrize("cls", [False, True])
def test_learner_batches_carry_the_row_state(ctx, data1, monkeypatch, cls):
    """Batches of 3, 3 and 2 learners (sum and n_oob, or counters, running maximum and
    running mode, carried in global memory) give the bytes of the single batch."""
    ds, forest, p, want, _ = case1(ctx, data1, REGIMES[0], cls)
    monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", "3")
    got = native_oob(ctx, forest, ds, **p)
    monkeypatch.delenv("SBAG_OOB_BATCH_LEARNERS")
    one = native_oob(ctx, forest, ds, **p)
    assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
    assert_oob_equal(got, want)


# ---------------------------------------------------------------- 2-5. the other kernel paths
def _dyadic_labels(rng, X):
    return rng.integers(-400, 400, X.shape[0]) / 16 + np.round(X[:, 0] * 8) / 32


@pytest.mark.parametrize("batch", [None, "7"])
def test_several_lds_chunks_u16_codes(ctx, monkeypatch, batch):
    """24 depth-9 trees take several LDS chunks; a batch of 7 learners ends inside a chunk."""
    rng = np.random.default_rng(12)
    N = 20000
    X = np.round(rng.normal(size=(N, 6)), 3)
    y = _dyadic_labels(rng, X)
    p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=24, depth=9, part=[0, N // 3, N])
    orf, counts, per_tree, _ = oracle_side(X, y, **p)
    tb = tree_bytes(orf)
    assert sum(tb) > 2 * 65536 and max(tb) <= 65536
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 2
    forest = fit_native(ctx, ds, **p)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    assert_oob_equal(native_oob(ctx, forest, ds, **p), oob_by_rows(counts, per_tree, False))


def test_trees_past_the_lds_chunk_walk_global_memory(ctx):
    rng = np.random.default_rng(12)
    N = 40000
    X = np.round(rng.normal(size=(N, 4)), 3)
    y = _dyadic_labels(rng, X)
    p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=3, depth=14, part=[0, N // 3, N])
    orf, counts, per_tree, _ = oracle_side(X, y, **p)
    assert max(tree_bytes(orf)) > 65536  # plan_tiled must refuse
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = fit_native(ctx, ds, **p)
    assert_oob_equal(native_oob(ctx, forest, ds, **p), oob_by_rows(counts, per_tree, False))


@pytest.mark.parametrize("batch", [None, "2"])
def test_u32_codes(ctx, monkeypatch, batch):
    rng = np.random.default_rng(13)
    N = 70000
    X = np.stack([rng.permutation(N) / 4.0, rng.permutation(N) * 1.0], axis=1)  # distinct values
    y = rng.integers(-400, 400, N) / 16 + np.floor(X[:, 0] / 2048)
    p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=3, depth=5, part=[0, 30001, N])
    _, counts, per_tree, _ = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 4
    forest = fit_native(ctx, ds, **p)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    assert_oob_equal(native_oob(ctx, forest, ds, **p), oob_by_rows(counts, per_tree, False))


@pytest.mark.parametrize("batch", [None, "4"])
def test_more_classes_than_the_lds_counters(ctx, monkeypatch, batch):
    """400 classes (kLdsModeClasses = 320).  The oracle's calculators hold 256 classes, so
    its gini trees are grown on the 200 label pairs y // 2 and every leaf then names one
    class of its pair (2 c + leaf id % 2): 6 depth-5 trees voting over 400 classes, loaded
    into the engine from the oracle's node arrays."""
    rng = np.random.default_rng(14)
    N, L = 3000, 6
    X = np.round(rng.normal(size=(N, 5)) * 6) / 8
    y = rng.integers(0, 400, N).astype(np.float64)
    p = dict(cls=True, replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=L, depth=5, part=[0, 1000, N])
    orf, counts, _, _ = oracle_side(X, np.floor(y / 2), **p)
    for t in range(L):
        nodes, _ = orf.tree(t)
        leaf = nodes["left"] < 0
        nodes["prediction"][leaf] = 2 * nodes["prediction"][leaf] + nodes["id"][leaf] % 2
    first = orf.tree(0)[0]
    first["prediction"][np.flatnonzero(first["left"] < 0)[0]] = 399.0
    _, per_tree = oracle.predict(orf, X, True, per_tree=True)
    assert per_tree.max() == 399.0 and len(np.unique(per_tree)) > 50 and (per_tree >= 320).mean() > 0.1
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = nat.NativeForest.from_trees([orf.tree(t)[0].astype(nat.NODE_DTYPE) for t in range(L)],
                                         orf.subspaces, nat.IMPURITY_GINI)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    assert_oob_equal(native_oob(ctx, forest, ds, **p), oob_by_rows(counts, per_tree, True))


# ---------------------------------------------------------------- 6. composed cross-check
@pytest.mark.parametrize("classes", [0, 5])
def test_equals_composed_sample_and_votes_at_the_bench_layout(ctx, classes):
    import torch

    N, L, P = 100_000, 16, 4
    part = sb.even_partitions(N, P)
    ds = nat.DeviceDataset.synthetic(N, 100, num_classes=classes, ctx=ctx)
    cls = classes > 0
    seed = SEED_CLS if cls else SEED_REG
    forest = fit_native(ctx, ds, cls=cls, replacement=True, ratio=1.0, seed=seed, lb=0, L=L, depth=8, part=part)
    counts = nat.sample(ctx, True, 1.0, seed, 0, L, N, part)
    dev = torch.device("cuda", ctx.device)
    buf = torch.empty((L, N), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    nat.predict_dataset_device(ctx, forest, ds, nat.OUT_VOTES, 8, buf.data_ptr())
    torch.cuda.synchronize(dev)
    want = oob_vectorised(counts, buf.cpu().numpy(), cls)
    assert (want[1] > 0).any() and (want[1] == 0).any()
    got = nat.predict_oob(ctx, forest, ds, replacement=True, sample_ratio=1.0, seed=seed, learner_begin=0,
                          learner_end=L, partition_offsets=part, agg=nat.AGG_MODE if cls else nat.AGG_MEAN)
    assert_oob_equal(got, want)
    ds.free()


# ---------------------------------------------------------------- 7. model API
@pytest.mark.parametrize("cls", [False, True])
def test_model_api(ctx, data1, tmp_path, cls):
    X, ys = data1
    y = ys[cls]
    part = [0, 300, 811, 1300]
    frame = sb.Frame(X, y, partition_offsets=part)
    if cls:
        est = sb.BaggingClassifier().setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(6))
        est.setReplacement(False).setSampleRatio(0.6)
        seed, metrics, model_cls = SEED_CLS, ["accuracy"], sb.BaggingClassificationModel
    else:
        est = sb.BaggingRegressor().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(6))
        est.setReplacement(True)
        seed, metrics, model_cls = SEED_REG, ["rmse", "mse", "mae", "r2"], sb.BaggingRegressionModel
    est.setNumBaseLearners(8)
    p = dict(cls=cls, replacement=est.getReplacement(), ratio=est.getSampleRatio(), seed=seed, depth=6, part=part)

    def want_for(lb, L):
        _, counts, per_tree, _ = oracle_side(X, y, lb=lb, L=L, **p)
        return oob_by_rows(counts, per_tree, cls)

    model = est.fit(frame)
    assert model.learner_range == (0, 8)
    want = want_for(0, 8)
    assert (want[1] > 0).any() and (want[1] == 0).any()
    assert_oob_equal(model.oobPredictions(frame), want)
    for m in metrics:
        assert model.oobScore(frame, m) == oob_metrics(want[0], want[1], y, cls, m)
    assert model.oobScore(frame) == oob_metrics(want[0], want[1], y, cls)
    # the fitted device dataset serves as well, with the fit's partitions
    ds = frame.device_dataset(ctx)
    assert_oob_equal(model.oobPredictions(ds, part), want)
    ds.free()
    # save / load: the range is (0, numBaseModels), the sampler params come back with the model
    path = str(tmp_path / "model")
    model.save(path)
    back = model_cls.load(path)
    assert back.learner_range is None
    assert_oob_equal(back.oobPredictions(frame), want)
    assert back.oobScore(frame) == model.oobScore(frame)
    # a fit_range shard: learners 2..5 with their own bags (rows 2..5 of the ensemble's)
    shard = est.fit_range(frame, 2, 6)
    assert shard.learner_range == (2, 6)
    assert_oob_equal(shard.oobPredictions(frame), want_for(2, 4))


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_context_usable(ctx, data1):
    X, ys = data1
    N = len(X)
    ds = nat.DeviceDataset.from_numpy(X, ys[False], ctx)
    kw = dict(replacement=True, sample_ratio=1.0, seed=SEED_REG, agg=nat.AGG_MEAN)
    forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED_REG, learner_begin=0,
                     learner_end=4, partition_offsets=PART1, max_depth=4)
    with pytest.raises(sb.IllegalArgumentException):  # 5 learners for a 4-tree forest
        nat.predict_oob(ctx, forest, ds, learner_begin=0, learner_end=5, partition_offsets=PART1, **kw)
    with pytest.raises(sb.IllegalArgumentException):  # offsets ending at N - 1
        nat.predict_oob(ctx, forest, ds, learner_begin=0, learner_end=4,
                        partition_offsets=[0, 300, N - 1], **kw)
    with pytest.raises(sb.IllegalArgumentException):
        nat.predict_oob(ctx, forest, ds, learner_begin=0, learner_end=4, partition_offsets=[0, N - 1], **kw)
    pred, n_oob = nat.predict_oob(ctx, forest, ds, learner_begin=0, learner_end=4, partition_offsets=PART1, **kw)
    counts = oracle.bag(True, 1.0, 0, 4, SEED_REG, PART1, N)
    np.testing.assert_array_equal(n_oob, (counts == 0).sum(axis=0))
    assert np.array_equal(np.isnan(pred), n_oob == 0)
    ds.free()
