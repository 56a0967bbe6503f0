"""GPU: per-class raw predictions (sbag_predict_raw, sbag_predict_raw_dataset,
sbag_predict_oob_raw) against proba_ref on the oracle's forests and oracle.bag's counts.

proba_ref (held to the oracle in test_proba_host.py) follows the rule of include/sbag.h
literally; everything is compared bit for bit (assert_array_equal)."""
import os

import numpy as np
import pytest

from conftest import ROOT

import oracle
import proba_ref
from parity_utils import oracle_forest

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_log_loss, raw_to_probability

pytestmark = pytest.mark.gpu

SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER
SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
KINDS = [nat.RAW_VOTES, nat.RAW_LEAF]
CHUNK = 65536  # the LDS chunk of the fused pass (plan_tiled's budget at these row widths)


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def fit_native(ctx, ds, *, replacement, ratio, seed, lb, L, depth, part, bins=32, **_):
    return nat.fit(ctx, ds, replacement=replacement, sample_ratio=ratio, seed=seed, learner_begin=lb,
                   learner_end=lb + L, partition_offsets=part, max_depth=depth, max_bins=bins,
                   impurity=nat.IMPURITY_GINI)


def oracle_side(X, y, *, replacement, ratio, seed, lb, L, depth, part, bins=32, **_):
    """(counts, trees, stats, subspaces) of the oracle's gini forest."""
    N, F = X.shape
    counts = oracle.bag(replacement, ratio, lb, lb + L, seed, part, N)
    subs = [oracle.subspace(ratio, F, seed + i) for i in range(lb, lb + L)]
    orf = oracle_forest(X, y, counts, subs, depth, bins, True, part=part)
    return counts, [orf.tree(t)[0] for t in range(L)], [orf.tree(t)[1] for t in range(L)], orf.subspaces


def native_oob(ctx, forest, ds, kind, *, replacement, ratio, seed, lb, L, part, num_classes=None, **_):
    return nat.predict_oob_raw(ctx, forest, ds, replacement=replacement, sample_ratio=ratio, seed=seed,
                               learner_begin=lb, learner_end=lb + L, partition_offsets=part, kind=kind,
                               num_classes=num_classes)


def assert_raw_equal(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def assert_oob_equal(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    assert got[1].dtype == np.int32
    assert_raw_equal(got[0], want[0])
    assert not np.isnan(got[0]).any()
    assert (got[0][want[1] == 0] == 0.0).all()


def payload_bytes(trees, C):
    """Per tree, what the fused pass stages: 8 bytes per node + (soft) C fractions per leaf."""
    return [8 * len(t) + 8 * C * int((t["left"] < 0).sum()) for t in trees]


# ---------------------------------------------------------------- 1. vehicle.svm
def test_vehicle_all_calls_both_kinds(ctx):
    X, y = sb.load_libsvm(os.path.join(ROOT, "tests", "golden", "data", "vehicle.svm"))
    N = len(y)
    p = dict(replacement=True, ratio=0.7, seed=SEED_CLS, lb=0, L=8, depth=5, part=[0, 300, 300, N])
    counts, trees, stats, subs = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = fit_native(ctx, ds, **p)
    C = forest.num_classes
    assert C == 5 == max(s.shape[1] for s in stats)
    want = {k: proba_ref.raw(trees, stats, subs, X, k, C) for k in KINDS}
    want_oob = {k: proba_ref.raw(trees, stats, subs, X, k, C, counts=counts) for k in KINDS}
    # the inputs discriminate: hard and soft voting disagree on some rows, some rows are uncovered
    assert (want[0].argmax(axis=1) != want[1].argmax(axis=1)).sum() == 56
    assert (want_oob[0][0].argmax(axis=1) != want_oob[1][0].argmax(axis=1)).sum() == 102
    assert (want_oob[0][1] == 0).sum() == 7
    for k in KINDS:
        assert_raw_equal(nat.predict_raw(ctx, forest, X, k), want[k])
        assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, k), want[k])
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), want_oob[k])
    # against the existing calls
    votes = nat.predict_raw(ctx, forest, X, nat.RAW_VOTES)
    mode, per_tree = nat.predict(ctx, forest, X, nat.AGG_MODE, per_tree=True)
    np.testing.assert_array_equal(
        votes, np.stack([np.bincount(per_tree[:, r].astype(np.int64), minlength=C) for r in range(N)]))
    np.testing.assert_array_equal(votes.sum(axis=1), np.full(N, 8.0))
    unique_top = (votes == votes.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique_top.sum() > N // 2
    np.testing.assert_array_equal(votes.argmax(axis=1)[unique_top], mode[unique_top])
    _, n_oob = nat.predict_oob(ctx, forest, ds, replacement=True, sample_ratio=0.7, seed=SEED_CLS, learner_begin=0,
                               learner_end=8, partition_offsets=p["part"], agg=nat.AGG_MODE)
    raw_oob, n_oob_raw = native_oob(ctx, forest, ds, nat.RAW_VOTES, **p)
    assert n_oob.tobytes() == n_oob_raw.tobytes()
    np.testing.assert_array_equal(raw_oob.sum(axis=1), n_oob)
    forest.free()
    ds.free()


# ---------------------------------------------------------------- 2. sampler regimes, 4. learner batches
N1, F1 = 1300, 9  # two full 512-row tiles + a 276-row tail
PART1 = [0, 300, 300, 811, 1300]  # an empty partition
REGIMES = [(True, 1.0, 8, 0), (False, 0.5, 8, 0), (True, 0.63, 5, 3), (False, 1.0, 3, 0)]


@pytest.fixture(scope="module")
def data1():
    rng = np.random.default_rng(11)
    X = np.round(rng.normal(size=(N1, F1)) * 6) / 8  # u8 codes
    kc = rng.integers(0, 3, N1)
    return X, ((np.floor(3 * np.abs(X[:, 0])) + kc) % 7).astype(np.float64)


_cases1 = {}


def case1(ctx, data1, regime):
    """One fit of a regime on both sides, shared by the tests that use it."""
    if regime not in _cases1:
        X, y = data1
        replacement, ratio, L, lb = regime
        p = dict(replacement=replacement, ratio=ratio, seed=SEED_CLS, lb=lb, L=L, depth=6, part=PART1)
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        assert ds.layout()[3] == 1
        forest = fit_native(ctx, ds, **p)
        assert forest.num_classes == 7
        counts, trees, stats, subs = oracle_side(X, y, **p)
        want = {k: proba_ref.raw(trees, stats, subs, X, k, 7, counts=counts) for k in KINDS}
        plain = {k: proba_ref.raw(trees, stats, subs, X, k, 7) for k in KINDS}
        _cases1[regime] = (ds, forest, p, want, plain)
    return _cases1[regime]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("regime", REGIMES)
def test_sampler_regimes(ctx, data1, regime, kind):
    ds, forest, p, want, plain = case1(ctx, data1, regime)
    covered = want[kind][1] > 0
    if regime == (False, 1.0, 3, 0):  # every count is 1: no row is ever out of bag; all zeros
        assert not covered.any() and (want[kind][0] == 0.0).all()
    else:
        assert covered.any() and (~covered).any()
        assert (want[kind][0] != plain[kind]).any(axis=1).sum() >= 100
    assert_oob_equal(native_oob(ctx, forest, ds, kind, **p), want[kind])
    assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, kind), plain[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_learner_batches_carry_raw_and_n_oob(ctx, data1, monkeypatch, kind):
    """Batches of 3, 3 and 2 learners, the rows' state carried in raw itself."""
    ds, forest, p, want, _ = case1(ctx, data1, REGIMES[0])
    monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", "3")
    got = native_oob(ctx, forest, ds, kind, **p)
    monkeypatch.delenv("SBAG_OOB_BATCH_LEARNERS")
    one = native_oob(ctx, forest, ds, kind, **p)
    assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
    assert_oob_equal(got, want[kind])


@pytest.mark.parametrize("batch", [None, "3"])
def test_soft_sums_in_lds_past_eight_classes(ctx, data1, monkeypatch, batch):
    """Up to 8 classes the fused soft pass keeps a row's sums in registers; 12 classes take
    its LDS accumulators (still the fused pass: 12 x 4 KB beside a 64 KB chunk)."""
    X, _ = data1
    rng = np.random.default_rng(15)
    y = ((3 * np.floor(3 * np.abs(X[:, 0])) + rng.integers(0, 3, N1)) % 12).astype(np.float64)
    assert y.max() == 11
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=8, depth=6, part=PART1)
    counts, trees, stats, subs = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 1
    forest = fit_native(ctx, ds, **p)
    assert forest.num_classes == 12
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    for k in KINDS:
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), proba_ref.raw(trees, stats, subs, X, k, 12, counts=counts))
        assert_raw_equal(nat.predict_raw(ctx, forest, X, k), proba_ref.raw(trees, stats, subs, X, k, 12))
    forest.free()
    ds.free()


# ---------------------------------------------------------------- 3. row-tile edges
@pytest.fixture(scope="module")
def edge_forest(ctx):
    rng = np.random.default_rng(21)
    X = rng.integers(0, 32, size=(1025, 5)).astype(np.float64)
    y = ((X[:, 0] // 8 + X[:, 1] // 16 + rng.integers(0, 2, 1025)) % 3).astype(np.float64)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=5, depth=4, part=[0, 1025])
    _, trees, stats, subs = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = fit_native(ctx, ds, **p)
    ds.free()
    assert forest.num_classes == 3
    return X, forest, proba_ref.raw(trees, stats, subs, X, proba_ref.LEAF, 3)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_row_tile_edges_and_row_batches(ctx, edge_forest, monkeypatch, n):
    X, forest, want = edge_forest
    one = nat.predict_raw(ctx, forest, X[:n], nat.RAW_LEAF)
    monkeypatch.setenv("SBAG_PREDICT_BATCH_ROWS", "300")  # a batch ends inside a tile
    got = nat.predict_raw(ctx, forest, X[:n], nat.RAW_LEAF)
    monkeypatch.delenv("SBAG_PREDICT_BATCH_ROWS")
    assert got.tobytes() == one.tobytes()
    assert_raw_equal(got, want[:n])
    ds = nat.DeviceDataset.from_numpy(X[:n], np.zeros(n), ctx)
    assert ds.layout()[3] == 1
    assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF), want[:n])
    ds.free()


# ---------------------------------------------------------------- 5-7. the other kernel paths
def _noisy_classes(rng, X, C):
    return ((np.floor(np.abs(X[:, 0]) * 2) + rng.integers(0, 2, X.shape[0])) % C).astype(np.float64)


@pytest.mark.parametrize("batch", [None, "7"])
def test_several_lds_chunks_u16_codes(ctx, monkeypatch, batch):
    """24 depth-9 trees take several LDS chunks; a batch of 7 learners ends inside a chunk."""
    rng = np.random.default_rng(12)
    N = 20000
    X = np.round(rng.normal(size=(N, 6)), 3)
    y = _noisy_classes(rng, X, 4)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=24, depth=9, part=[0, N // 3, N])
    counts, trees, stats, subs = oracle_side(X, y, **p)
    tb = payload_bytes(trees, 4)
    assert sum(tb) > 2 * CHUNK and max(tb) <= CHUNK
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 2
    forest = fit_native(ctx, ds, **p)
    assert forest.num_classes == 4
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    for k in KINDS:
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), proba_ref.raw(trees, stats, subs, X, k, 4, counts=counts))
    assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF),
                     proba_ref.raw(trees, stats, subs, X, proba_ref.LEAF, 4))
    forest.free()
    ds.free()


def test_a_tree_past_the_lds_chunk_walks_global_memory(ctx):
    rng = np.random.default_rng(12)
    N = 40000
    X = np.round(rng.normal(size=(N, 4)), 3)
    y = _noisy_classes(rng, X, 4)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=3, depth=14, part=[0, N // 3, N])
    counts, trees, stats, subs = oracle_side(X, y, **p)
    assert max(payload_bytes(trees, 4)) > CHUNK  # the soft plan must refuse
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = fit_native(ctx, ds, **p)
    for k in KINDS:
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), proba_ref.raw(trees, stats, subs, X, k, 4, counts=counts))
    want = proba_ref.raw(trees, stats, subs, X, proba_ref.LEAF, 4)
    assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF), want)
    assert_raw_equal(nat.predict_raw(ctx, forest, X, nat.RAW_LEAF), want)
    forest.free()
    ds.free()


@pytest.mark.parametrize("batch", [None, "2"])
def test_u32_codes(ctx, monkeypatch, batch):
    rng = np.random.default_rng(13)
    N = 70000
    X = np.stack([rng.permutation(N) / 4.0, rng.permutation(N) * 1.0], axis=1)  # distinct values
    y = ((np.floor(X[:, 0] / 2048) + rng.integers(0, 2, N)) % 3).astype(np.float64)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=3, depth=5, part=[0, 30001, N])
    counts, trees, stats, subs = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 4
    forest = fit_native(ctx, ds, **p)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    for k in KINDS:
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), proba_ref.raw(trees, stats, subs, X, k, 3, counts=counts))
        assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, k), proba_ref.raw(trees, stats, subs, X, k, 3))
    forest.free()
    ds.free()


# ---------------------------------------------------------------- 8. many classes
@pytest.mark.parametrize("batch", [None, "4"])
def test_more_classes_than_the_lds_holds(ctx, monkeypatch, batch):
    """400 classes.  The oracle's calculators hold 256 classes, so its gini trees are grown
    on the 200 label pairs y // 2; every node then splits each pair's count onto one class of
    the pair (2 c + node id % 2), predictions and stats alike: 6 depth-5 trees over 400
    classes, loaded with their stats through sbag_forest_create_stats."""
    rng = np.random.default_rng(14)
    N, L = 3000, 6
    X = np.round(rng.normal(size=(N, 5)) * 6) / 8
    y = rng.integers(0, 400, N).astype(np.float64)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=L, depth=5, part=[0, 1000, N])
    counts, trees, stats, subs = oracle_side(X, np.floor(y / 2), **p)
    wide_trees, wide_stats = [], []
    for nodes, st in zip(trees, stats):
        nodes = nodes.copy().astype(nat.NODE_DTYPE)
        b = nodes["id"] % 2
        leaf = nodes["left"] < 0
        nodes["prediction"][leaf] = 2 * nodes["prediction"][leaf] + b[leaf]
        ws = np.zeros((len(nodes), 400))
        for i in range(len(nodes)):
            ws[i, 2 * np.arange(st.shape[1]) + b[i]] = st[i]
        wide_trees.append(nodes)
        wide_stats.append(ws)
    forest = nat.NativeForest.from_trees(wide_trees, subs, nat.IMPURITY_GINI, stats=wide_stats)
    assert forest.num_classes == 400
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    for k in KINDS:
        want = proba_ref.raw(wide_trees, wide_stats, subs, X, k, 400, counts=counts)
        assert (want[0][:, 320:] != 0).any(axis=1).mean() > 0.1 and (want[0] != 0).any(axis=0).sum() > 50
        assert_oob_equal(native_oob(ctx, forest, ds, k, **p), want)
        assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, k), proba_ref.raw(wide_trees, wide_stats, subs, X, k, 400))
    forest.free()
    ds.free()


# ---------------------------------------------------------------- 9. hand-built edge forests
def _tree(rows):
    """rows: (left, right, feature, threshold, prediction) per pre-order node."""
    t = np.zeros(len(rows), nat.NODE_DTYPE)
    t["id"] = np.arange(len(rows))
    for f, col in zip(("left", "right", "feature", "threshold", "prediction"), zip(*rows)):
        t[f] = col
    return t


def test_hand_built_edge_forests(ctx):
    rng = np.random.default_rng(31)
    N = 603
    X = rng.integers(0, 16, size=(N, 3)).astype(np.float64)
    trees = [
        # num_stats 2, below the forest's 4 classes: columns 2 and 3 unchanged by this tree
        _tree([(1, 2, 0, 7.0, 0.0), (-1, -1, -1, 0.0, 0.0), (-1, -1, -1, 0.0, 1.0)]),
        # a leaf with all-zero stats (node 3) contributes nothing to the soft sum
        _tree([(1, 4, 1, 5.0, 3.0), (2, 3, 0, 3.0, 3.0), (-1, -1, -1, 0.0, 3.0), (-1, -1, -1, 0.0, 2.0),
               (-1, -1, -1, 0.0, 1.0)]),
        # a single leaf
        _tree([(-1, -1, -1, 0.0, 2.0)]),
        _tree([(1, 2, 0, 11.0, 1.0), (-1, -1, -1, 0.0, 1.0), (-1, -1, -1, 0.0, 0.0)]),
    ]
    stats = [np.array([[5.0, 3.0], [4.0, 1.0], [1.0, 2.0]]),
             np.array([[1.0, 2.0, 3.0, 7.0], [0.0, 1.0, 2.0, 7.0], [0.0, 0.0, 1.0, 6.0], [0.0, 0.0, 0.0, 0.0],
                       [1.0, 3.0, 1.0, 0.0]]),
             np.array([[0.1, 0.2, 0.7]]),
             np.array([[3.0, 6.0, 0.0], [1.0, 6.0, 0.0], [2.0, 0.0, 0.0]])]
    subs = [[0], [1, 2], [1], [2]]
    forest = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_GINI, stats=stats)
    assert forest.num_classes == 4
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=4, part=[0, 200, N])
    counts = oracle.bag(True, 1.0, 0, 4, SEED_CLS, p["part"], N)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(N), ctx)
    for k in KINDS:
        for C in (4, 6):  # num_classes past the forest's: the extra columns are 0.0
            want = proba_ref.raw(trees, stats, subs, X, k, C)
            assert (want[:, 4:] == 0.0).all() and (want[:, :4] != 0).any(axis=0).all()
            assert_raw_equal(nat.predict_raw(ctx, forest, X, k, num_classes=C), want)
            assert_raw_equal(nat.predict_raw_dataset(ctx, forest, ds, k, num_classes=C), want)
            assert_oob_equal(native_oob(ctx, forest, ds, k, num_classes=C, **p),
                             proba_ref.raw(trees, stats, subs, X, k, C, counts=counts))
    soft = proba_ref.raw(trees, stats, subs, X, proba_ref.LEAF, 4)
    empty_leaf = (X[:, 2] <= 5.0) & (X[:, 1] > 3.0)  # tree 1's all-zero leaf: three trees' worth
    assert empty_leaf.any() and np.abs(soft[empty_leaf].sum(axis=1) - 3.0).max() < 1e-12
    assert np.abs(soft[~empty_leaf].sum(axis=1) - 4.0).max() < 1e-12
    forest.free()
    ds.free()


# ---------------------------------------------------------------- 10. model API
def _sparse(X):
    mask = X != 0
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))])
    return sb.SparseRows(indptr, np.nonzero(mask)[1], X[mask], X.shape)


def test_model_api(ctx, data1, tmp_path):
    X, y = data1
    part = [0, 300, 811, 1300]
    frame = sb.Frame(X, y, partition_offsets=part)
    est = sb.BaggingClassifier().setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(6))
    est.setReplacement(True).setSampleRatio(0.8).setNumBaseLearners(8)
    model = est.fit(frame)
    p = dict(replacement=True, ratio=0.8, seed=SEED_CLS, lb=0, L=8, depth=6, part=part)
    counts, trees, stats, subs = oracle_side(X, y, **p)
    assert model.numClasses == 7
    for strategy, k in (("hard", proba_ref.VOTES), ("soft", proba_ref.LEAF)):
        want = proba_ref.raw(trees, stats, subs, X, k, 7)
        want_oob, n_oob = proba_ref.raw(trees, stats, subs, X, k, 7, counts=counts)
        assert (n_oob == 0).any() and (n_oob > 0).any()
        assert_raw_equal(model.predictRaw(frame, strategy), want)
        assert_raw_equal(model.predictRaw(X, strategy), want)
        assert_raw_equal(model.predictRaw(_sparse(X), strategy), want)
        ds = frame.device_dataset(ctx)
        assert_raw_equal(model.predictRaw(ds, strategy), want)
        np.testing.assert_array_equal(model.predictProbability(frame, strategy), raw_to_probability(want))
        got = model.oobProbabilities(frame, strategy)
        np.testing.assert_array_equal(got[1], n_oob)
        np.testing.assert_array_equal(got[0], raw_to_probability(want_oob))
        assert np.array_equal(np.isnan(got[0]).all(axis=1), n_oob == 0)
        got_ds = model.oobProbabilities(ds, strategy, partition_offsets=part)
        assert got_ds[0].tobytes() == got[0].tobytes() and got_ds[1].tobytes() == got[1].tobytes()
        ds.free()
        ll = model.oobLogLoss(frame, strategy)
        assert ll == oob_log_loss(raw_to_probability(want_oob), n_oob, y)
        assert ll["metric"] == "logLoss" and 0 < ll["value"] < 40 and ll["coverage"] == (n_oob > 0).mean()
    assert model.predictRaw(frame).tobytes() == model.predictRaw(frame, "soft").tobytes()  # the default
    # save -> load: the stats come back with the model and reach the device
    path = str(tmp_path / "model")
    model.save(path)
    back = sb.BaggingClassificationModel.load(path)
    assert back.numClasses == 7
    for strategy in ("hard", "soft"):
        assert back.predictRaw(frame, strategy).tobytes() == model.predictRaw(frame, strategy).tobytes()
        a, b = back.oobProbabilities(frame, strategy), model.oobProbabilities(frame, strategy)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert back.oobLogLoss(frame, strategy) == model.oobLogLoss(frame, strategy)
    with pytest.raises(sb.IllegalArgumentException):
        model.predictRaw(frame, "weighted")
    # a regression model has no class probabilities
    reg = sb.BaggingRegressor().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(3)).setNumBaseLearners(2)
    rmodel = reg.fit(sb.Frame(X, X[:, 0] * 2.0))
    for name in ("predictRaw", "predictProbability", "oobProbabilities", "oobLogLoss"):
        with pytest.raises(sb.IllegalArgumentException):
            getattr(rmodel, name)(frame)
    assert rmodel.transform(X).shape == (N1,)


# ---------------------------------------------------------------- 11. refusals
def test_refusals_leave_the_context_usable(ctx, data1):
    X, y = data1
    N = len(X)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    p = dict(replacement=True, ratio=1.0, seed=SEED_CLS, lb=0, L=4, depth=4, part=PART1)
    forest = fit_native(ctx, ds, **p)
    C = forest.num_classes
    ok = nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF)

    def still_works():
        assert nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF).tobytes() == ok.tobytes()

    calls = {
        "rows": lambda f, kind, nc: nat.predict_raw(ctx, f, X, kind, num_classes=nc),
        "dataset": lambda f, kind, nc: nat.predict_raw_dataset(ctx, f, ds, kind, num_classes=nc),
        "oob": lambda f, kind, nc: native_oob(ctx, f, ds, kind, num_classes=nc, **p),
    }
    nostats = nat.NativeForest.from_trees([forest.tree(t)[0] for t in range(4)], [forest.subspace(t) for t in range(4)],
                                          nat.IMPURITY_GINI)
    assert nostats.num_classes == C
    rds = nat.DeviceDataset.from_numpy(X, X[:, 0], ctx)
    variance = nat.fit(ctx, rds, replacement=True, sample_ratio=1.0, seed=SEED_REG, learner_begin=0, learner_end=4,
                       partition_offsets=PART1, max_depth=4)
    for name, call in calls.items():
        for f, kind, nc in [(forest, 2, C), (forest, -1, C),        # an unknown kind
                            (variance, nat.RAW_VOTES, C),            # not a gini forest
                            (forest, nat.RAW_VOTES, C - 1), (forest, nat.RAW_LEAF, 0),  # too few columns
                            (nostats, nat.RAW_LEAF, C)]:             # soft voting without stats
            with pytest.raises(sb.IllegalArgumentException):
                call(f, kind, nc)
            still_works()
        # hard voting needs no stats
        got = call(nostats, nat.RAW_VOTES, C)
        want = call(forest, nat.RAW_VOTES, C)
        got, want = (got[0], want[0]) if name == "oob" else (got, want)
        assert got.tobytes() == want.tobytes()
    # null arguments
    lib = nat.lib()
    out = np.zeros((N, C))
    assert lib.sbag_predict_raw(ctx.handle, forest.handle, None, N, F1, nat.RAW_VOTES, C, nat.ptr(out)) == nat.SBAG_EINVAL
    assert lib.sbag_predict_raw_dataset(ctx.handle, forest.handle, ds.handle, nat.RAW_VOTES, C, None) == nat.SBAG_EINVAL
    assert lib.sbag_predict_oob_raw(ctx.handle, forest.handle, ds.handle, None, None, 1, nat.RAW_VOTES, C, nat.ptr(out),
                                    None) == nat.SBAG_EINVAL
    assert (out == 0).all()
    still_works()
    # the out-of-bag call's own refusals are sbag_predict_oob's
    with pytest.raises(sb.IllegalArgumentException):  # 5 learners for a 4-tree forest
        native_oob(ctx, forest, ds, nat.RAW_LEAF, **dict(p, L=5))
    with pytest.raises(sb.IllegalArgumentException):  # offsets ending at N - 1
        native_oob(ctx, forest, ds, nat.RAW_LEAF, **dict(p, part=[0, 300, N - 1]))
    still_works()
    raw, n_oob = native_oob(ctx, forest, ds, nat.RAW_VOTES, **p)
    counts = oracle.bag(True, 1.0, 0, 4, SEED_CLS, PART1, N)
    np.testing.assert_array_equal(n_oob, (counts == 0).sum(axis=0))
    np.testing.assert_array_equal(raw.sum(axis=1), n_oob)
    # no rows: SBAG_OK, nothing written
    assert nat.predict_raw(ctx, forest, np.zeros((0, F1)), nat.RAW_LEAF).shape == (0, C)
    for f in (forest, nostats, variance):
        f.free()
    rds.free()
    ds.free()
