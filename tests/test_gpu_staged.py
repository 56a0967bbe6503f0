"""GPU: staged evaluation (sbag_eval_staged) against the CPU oracle.

Expected values come from the oracle's pieces, as in tests/test_gpu_oob.py: oracle.bag (the
counts), the oracle's forest and oracle.predict(per_tree=True), put through
tests/staged_ref.py (the NumPy restatement of the header's rule, itself checked against a
literal loop in tests/test_staged_host.py).  covered and correct must be equal, sum_se and
sum_ae bit for bit.  The engine evaluates the oracle's own trees (loaded from its node
arrays), so nothing here depends on the fit; a staged evaluation takes any sampler, so one
forest serves every sampler regime and every row count (the bags are drawn again for the
rows at hand, on both sides).
"""
import numpy as np
import pytest

import oracle
from parity_utils import oracle_forest
from staged_ref import (ORDER_SEEDS, assert_stats_equal, order_case, staged_ref, stats_of_prediction,
                        STAGE_DTYPE)

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_metrics

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def tree_bytes(orf):
    """8 * (nodes + leaves) of every tree: what the LDS-tiled plan stages per tree (the
    helper of tests/test_gpu_oob.py)."""
    out = []
    for t in range(orf.nodes.shape[0]):
        nodes, _ = orf.tree(t)
        out.append(8 * (len(nodes) + int((nodes["left"] < 0).sum())))
    return out


def engine_forest(orf, cls, first=None):
    """The oracle's first `first` trees (default: all) as an engine forest."""
    L = orf.nodes.shape[0] if first is None else first
    return nat.NativeForest.from_trees([orf.tree(t)[0].astype(nat.NODE_DTYPE) for t in range(L)],
                                       orf.subspaces[:L], nat.IMPURITY_GINI if cls else nat.IMPURITY_VARIANCE)


def staged(ctx, forest, ds, cls, sampler=None, part=None):
    """nat.eval_staged; sampler = (replacement, ratio, seed, learner_begin) or None."""
    agg = nat.AGG_MODE if cls else nat.AGG_MEAN
    if sampler is None:
        return nat.eval_staged(ctx, forest, ds, agg=agg)
    rep, ratio, seed, lb = sampler
    return nat.eval_staged(ctx, forest, ds, agg=agg, replacement=rep, sample_ratio=ratio, seed=seed,
                           learner_begin=lb, learner_end=lb + len(forest), partition_offsets=part)


def bags(sampler, L, part, N):
    rep, ratio, seed, lb = sampler
    return oracle.bag(rep, ratio, lb, lb + L, seed, part if part is not None else [0, N], N)


# ---------------------------------------------------------------- the shared cases
_cases = {}


def gini_case():
    """1,500 rows, 3 classes, u8 codes, the oracle's 8 depth-5 gini trees."""
    if "gini" not in _cases:
        rng = np.random.default_rng(31)
        N, L = 1500, 8
        X = np.round(rng.normal(size=(N, 6)) * 6) / 8
        y = ((np.floor(2 * np.abs(X[:, 0])) + rng.integers(0, 2, N)) % 3).astype(np.float64)
        part = [0, 700, N]
        counts = oracle.bag(True, 1.0, 0, L, SEED_CLS, part, N)
        subs = [oracle.subspace(1.0, X.shape[1], SEED_CLS + i) for i in range(L)]
        orf = oracle_forest(X, y, counts, subs, 5, 32, True, part=part)
        _, per_tree = oracle.predict(orf, X, True, per_tree=True)
        _cases["gini"] = (X, y, orf, per_tree)
    return _cases["gini"]


def base_case(ctx, cls, seed=ORDER_SEEDS[0]):
    """(X, y, oracle forest, per-tree predictions, engine forest, device dataset, the fit's
    sampler and partitions) of the regression (order_case: real-valued labels) or gini case."""
    key = ("base", cls, seed)
    if key not in _cases:
        if cls:
            X, y, orf, per_tree = gini_case()
        else:
            X, y, _, orf, _, per_tree = order_case(seed)
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        assert ds.layout()[3] == 1
        _cases[key] = (X, y, orf, per_tree, engine_forest(orf, cls), ds,
                       (True, 1.0, SEED_CLS if cls else SEED_REG, 0), [0, 700, len(y)])
    return _cases[key]


def check(ctx, forest, ds, y, per_tree, cls, sampler, part):
    """One call against staged_ref; returns (got, want)."""
    L, N = per_tree.shape
    counts = None if sampler is None else bags(sampler, L, part, N)
    want = staged_ref(counts, per_tree, y, cls)
    got = staged(ctx, forest, ds, cls, sampler, part)
    assert got.dtype == STAGE_DTYPE
    assert_stats_equal(got, want)
    return got, want


# ---------------------------------------------------------------- 1. the order, on inputs that show it
@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_real_valued_labels_in_the_documented_order(ctx, seed):
    """Two full tiles and a 476-row tail; tests/test_staged_host.py asserts that on these
    inputs the tile order differs from the sequential sum and from np.sum."""
    X, y, orf, per_tree, forest, ds, sampler, part = base_case(ctx, False, seed)
    got, want = check(ctx, forest, ds, y, per_tree, False, sampler, part)
    assert 0 < want["covered"][0] < len(y) and (np.diff(want["covered"]) >= 0).all()
    assert (want["sum_se"] > 0).all() and (want["correct"] == 0).all()


def test_gini_three_classes(ctx):
    X, y, orf, per_tree, forest, ds, sampler, part = base_case(ctx, True)
    got, want = check(ctx, forest, ds, y, per_tree, True, sampler, part)
    assert (want["correct"] > 0).all() and (want["correct"] < want["covered"]).all()
    assert (got["sum_se"] == 0).all() and (got["sum_ae"] == 0).all()


# ---------------------------------------------------------------- 2. tile edges
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("N", [1, 511, 512, 513, 1025, 1300])
def test_tile_edges(ctx, N, cls):
    """A short last tile and the rows past N: the +0.0 padding and the ballots' tails."""
    X, y, orf, per_tree, forest, _, sampler, _ = base_case(ctx, cls)
    ds = nat.DeviceDataset.from_numpy(X[:N], y[:N], ctx)
    part = [0, N // 3, N]
    for s in (sampler, None):
        check(ctx, forest, ds, y[:N], per_tree[:, :N], cls, s, part)
    ds.free()


# ---------------------------------------------------------------- 3. learner counts
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("L", [1, 2])
def test_one_and_two_learners(ctx, L, cls):
    X, y, orf, per_tree, _, ds, sampler, part = base_case(ctx, cls)
    forest = engine_forest(orf, cls, L)
    check(ctx, forest, ds, y, per_tree[:L], cls, sampler, part)
    forest.free()


def chunk_case(ctx):
    """12 trees whose summed bytes pass the 64 KB LDS chunk, on u16 codes.  Depth-5 trees
    (at most 760 bytes each) cannot pass it at any L the suite affords, so this one case
    grows depth-10 trees on 3,000 rows."""
    if "chunk" not in _cases:
        rng = np.random.default_rng(32)
        N, L = 3000, 12
        X = np.round(rng.normal(size=(N, 5)), 3)
        y = rng.normal(size=N) + X[:, 0] / 4
        part = [0, 1000, N]
        counts = oracle.bag(True, 1.0, 0, L, SEED_REG, part, N)
        subs = [oracle.subspace(1.0, X.shape[1], SEED_REG + i) for i in range(L)]
        orf = oracle_forest(X, y, counts, subs, 10, 32, False, part=part)
        tb = tree_bytes(orf)
        assert sum(tb) > 65536 and max(tb) <= 32768  # at least two chunks, every tree within one
        _, per_tree = oracle.predict(orf, X, False, per_tree=True)
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        assert ds.layout()[3] == 2
        _cases["chunk"] = (y, per_tree, engine_forest(orf, False), ds, (True, 1.0, SEED_REG, 0), part)
    return _cases["chunk"]


@pytest.mark.parametrize("batch", [None, "5"])
def test_several_lds_chunks_u16_codes(ctx, monkeypatch, batch):
    """The stage groups run across the chunk loads; a batch of 5 learners ends inside a chunk
    and inside a group."""
    y, per_tree, forest, ds, sampler, part = chunk_case(ctx)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    check(ctx, forest, ds, y, per_tree, False, sampler, part)


# ---------------------------------------------------------------- 4. learner batches
@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("cls", [False, True])
def test_learner_batches_give_the_bytes_of_one_batch(ctx, monkeypatch, cls, fallback):
    X, y, orf, per_tree, _, ds, sampler, part = base_case(ctx, cls)
    forest = engine_forest(orf, cls, 7)
    if fallback:
        monkeypatch.setenv("SBAG_STAGED_FORCE_FALLBACK", "1")
    one, _ = check(ctx, forest, ds, y, per_tree[:7], cls, sampler, part)
    for b in ("1", "3"):
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", b)
        assert staged(ctx, forest, ds, cls, sampler, part).tobytes() == one.tobytes()
        assert staged(ctx, forest, ds, cls).tobytes() == staged_ref(None, per_tree[:7], y, cls).tobytes()
    forest.free()


# ---------------------------------------------------------------- 5. sampler regimes
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("regime", ["poisson", "bernoulli", "partitions", "learner_begin"])
def test_sampler_regimes(ctx, regime, cls):
    X, y, orf, per_tree, forest, ds, (rep, ratio, seed, lb), part = base_case(ctx, cls)
    N = len(y)
    sampler, p = {"poisson": ((True, 1.0, seed, 0), None),
                  "bernoulli": ((False, 0.5, seed, 0), None),
                  "partitions": ((True, 0.63, seed, 0), [0, 300, 300, 811, N]),  # one empty
                  "learner_begin": ((False, 0.5, seed, 3), [0, 700, N])}[regime]
    got, want = check(ctx, forest, ds, y, per_tree, cls, sampler, p)
    assert 0 < want["covered"][0] < N


@pytest.mark.parametrize("cls", [False, True])
def test_nothing_is_ever_covered_without_replacement_at_ratio_one(ctx, cls):
    X, y, orf, per_tree, forest, ds, (_, _, seed, _), part = base_case(ctx, cls)
    got, _ = check(ctx, forest, ds, y, per_tree, cls, (False, 1.0, seed, 0), part)
    assert got.tobytes() == np.zeros(len(forest), STAGE_DTYPE).tobytes()  # every field zero, sums +0.0


# ---------------------------------------------------------------- 6. code kinds and the general path
def u16_case(ctx, cls):
    key = ("u16", cls)
    if key not in _cases:
        rng = np.random.default_rng(33)
        N, L = 1300, 5
        X = np.round(rng.normal(size=(N, 5)), 3)
        y = ((np.floor(2 * np.abs(X[:, 0])) + rng.integers(0, 2, N)) % 3).astype(np.float64) if cls \
            else rng.normal(size=N) + X[:, 0] / 4
        seed = SEED_CLS if cls else SEED_REG
        part = [0, 500, N]
        counts = oracle.bag(True, 1.0, 0, L, seed, part, N)
        subs = [oracle.subspace(1.0, X.shape[1], seed + i) for i in range(L)]
        orf = oracle_forest(X, y, counts, subs, 5, 32, cls, part=part)
        _, per_tree = oracle.predict(orf, X, cls, per_tree=True)
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        assert ds.layout()[3] == 2
        _cases[key] = (y, per_tree, engine_forest(orf, cls), ds, (True, 1.0, seed, 0), part)
    return _cases[key]


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("codes", ["u8", "u16"])
def test_forced_fallback_equals_the_fused_pass(ctx, monkeypatch, codes, cls):
    if codes == "u8":
        X, y, orf, per_tree, forest, ds, sampler, part = base_case(ctx, cls)
    else:
        y, per_tree, forest, ds, sampler, part = u16_case(ctx, cls)
    fused, _ = check(ctx, forest, ds, y, per_tree, cls, sampler, part)
    fused_plain, _ = check(ctx, forest, ds, y, per_tree, cls, None, None)
    monkeypatch.setenv("SBAG_STAGED_FORCE_FALLBACK", "1")
    assert staged(ctx, forest, ds, cls, sampler, part).tobytes() == fused.tobytes()
    assert staged(ctx, forest, ds, cls).tobytes() == fused_plain.tobytes()


@pytest.mark.parametrize("batch", [None, "2"])
def test_u32_codes_take_the_general_path(ctx, monkeypatch, batch):
    """u32 codes need a feature with more than 65,536 distinct values, so this case has
    66,000 rows; 3 depth-4 trees."""
    rng = np.random.default_rng(34)
    N, L = 66000, 3
    X = np.stack([rng.permutation(N) / 4.0, rng.permutation(N) * 1.0], axis=1)  # distinct values
    y = rng.normal(size=N) + np.floor(X[:, 0] / 2048)
    part = [0, 30001, N]
    sampler = (True, 1.0, SEED_REG, 0)
    counts = bags(sampler, L, part, N)
    subs = [oracle.subspace(1.0, 2, SEED_REG + i) for i in range(L)]
    orf = oracle_forest(X, y, counts, subs, 4, 32, False, part=part)
    _, per_tree = oracle.predict(orf, X, False, per_tree=True)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 4
    forest = engine_forest(orf, False)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    check(ctx, forest, ds, y, per_tree, False, sampler, part)
    check(ctx, forest, ds, y, per_tree, False, None, None)
    ds.free()
    forest.free()


@pytest.mark.parametrize("batch", [None, "4"])
def test_more_classes_than_the_lds_counters_take_the_general_path(ctx, monkeypatch, batch):
    """400 classes, built as in tests/test_gpu_oob.py: gini trees on the 200 label pairs
    y // 2, every leaf then naming one class of its pair."""
    rng = np.random.default_rng(14)
    N, L = 3000, 6
    X = np.round(rng.normal(size=(N, 5)) * 6) / 8
    y = rng.integers(0, 400, N).astype(np.float64)
    part = [0, 1000, N]
    sampler = (True, 1.0, SEED_CLS, 0)
    counts = bags(sampler, L, part, N)
    subs = [oracle.subspace(1.0, 5, SEED_CLS + i) for i in range(L)]
    orf = oracle_forest(X, np.floor(y / 2), counts, subs, 5, 32, True, part=part)
    for t in range(L):
        nodes, _ = orf.tree(t)
        leaf = nodes["left"] < 0
        nodes["prediction"][leaf] = 2 * nodes["prediction"][leaf] + nodes["id"][leaf] % 2
    first = orf.tree(0)[0]
    first["prediction"][np.flatnonzero(first["left"] < 0)[0]] = 399.0
    _, per_tree = oracle.predict(orf, X, True, per_tree=True)
    assert per_tree.max() == 399.0 and (per_tree >= 320).mean() > 0.1
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = engine_forest(orf, True)
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    got, want = check(ctx, forest, ds, y, per_tree, True, sampler, part)
    assert want["correct"][-1] > 0
    ds.free()
    forest.free()


# ---------------------------------------------------------------- 7. against the merged out-of-bag pass
@pytest.mark.parametrize("cls", [False, True])
def test_every_stage_equals_predict_oob_of_the_cut_forest(ctx, cls):
    """Independent of staged_ref: stage l's fields are those of nat.predict_oob on the first
    l + 1 trees with the learner range [lb, lb + l + 1)."""
    X, y, orf, per_tree, forest, ds, _, part = base_case(ctx, cls)
    rep, ratio, seed, lb = sampler = (True, 1.0, SEED_CLS if cls else SEED_REG, 2)
    got = staged(ctx, forest, ds, cls, sampler, part)
    for l in range(len(forest)):
        cut = engine_forest(orf, cls, l + 1)
        pred, n_oob = nat.predict_oob(ctx, cut, ds, replacement=rep, sample_ratio=ratio, seed=seed,
                                      learner_begin=lb, learner_end=lb + l + 1, partition_offsets=part,
                                      agg=nat.AGG_MODE if cls else nat.AGG_MEAN)
        want = np.zeros(1, STAGE_DTYPE)
        want[0] = stats_of_prediction(pred, n_oob, y, cls)
        assert_stats_equal(got[l:l + 1], want)
        cut.free()


# ---------------------------------------------------------------- 8. no mask
@pytest.mark.parametrize("cls", [False, True])
def test_no_mask_is_the_plain_transform_of_every_prefix(ctx, cls):
    X, y, orf, per_tree, forest, ds, _, _ = base_case(ctx, cls)
    N, L = len(y), len(forest)
    got, _ = check(ctx, forest, ds, y, per_tree, cls, None, None)
    assert (got["covered"] == N).all()
    agg = nat.AGG_MODE if cls else nat.AGG_MEAN
    ones = np.ones(N, np.int32)
    for l in range(L):
        cut = forest if l == L - 1 else engine_forest(orf, cls, l + 1)
        want = np.zeros(1, STAGE_DTYPE)
        want[0] = stats_of_prediction(nat.predict_dataset(ctx, cut, ds, agg), ones, y, cls)
        assert_stats_equal(got[l:l + 1], want)
        if cut is not forest:
            cut.free()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_context_usable(ctx):
    X, y, orf, per_tree, forest, ds, sampler, part = base_case(ctx, False)
    N, L = len(y), len(forest)
    rep, ratio, seed, lb = sampler
    lib = nat.lib()
    good = staged(ctx, forest, ds, False, sampler, part)

    def still_good():
        assert staged(ctx, forest, ds, False, sampler, part).tobytes() == good.tobytes()

    out = np.full(L, 7, STAGE_DTYPE)
    untouched = out.tobytes()
    p = nat.SamplerParams(1, 0, 1.0, seed, 0, L)
    import ctypes
    for args in ((None, forest.handle, ds.handle), (ctx.handle, None, ds.handle), (ctx.handle, forest.handle, None)):
        assert lib.sbag_eval_staged(*args, ctypes.byref(p), None, 1, nat.AGG_MEAN, nat.ptr(out)) == nat.SBAG_EINVAL
    assert lib.sbag_eval_staged(ctx.handle, forest.handle, ds.handle, ctypes.byref(p), None, 1, nat.AGG_MEAN,
                                None) == nat.SBAG_EINVAL
    still_good()
    kw = dict(replacement=rep, sample_ratio=ratio, seed=seed, agg=nat.AGG_MEAN)
    with pytest.raises(sb.IllegalArgumentException):  # 9 learners for an 8-tree forest
        nat.eval_staged(ctx, forest, ds, learner_begin=0, learner_end=L + 1, partition_offsets=part, **kw)
    still_good()
    with pytest.raises(sb.IllegalArgumentException):  # MODE on a variance forest
        nat.eval_staged(ctx, forest, ds, learner_begin=0, learner_end=L, partition_offsets=part,
                        **dict(kw, agg=nat.AGG_MODE))
    with pytest.raises(sb.IllegalArgumentException):
        nat.eval_staged(ctx, forest, ds, agg=nat.AGG_MODE)
    with pytest.raises(sb.IllegalArgumentException):
        nat.eval_staged(ctx, forest, ds, agg=5)
    still_good()
    narrow = nat.DeviceDataset.from_numpy(X[:, :2], y, ctx)  # the trees test features past column 1
    for s in (sampler, None):
        with pytest.raises(sb.IllegalArgumentException):
            staged(ctx, forest, narrow, False, s, part)
    narrow.free()
    still_good()
    for bad in ([0, 300, N - 1], [0, N - 1], [5, 300, N], [0, 900, 800, N]):
        with pytest.raises(sb.IllegalArgumentException):
            nat.eval_staged(ctx, forest, ds, learner_begin=0, learner_end=L, partition_offsets=bad, **kw)
    with pytest.raises(sb.IllegalArgumentException):  # sampleRatio outside (0, 1]
        nat.eval_staged(ctx, forest, ds, learner_begin=0, learner_end=L, **dict(kw, sample_ratio=0.0))
    assert out.tobytes() == untouched
    still_good()
    # no rows: the entry point answers SBAG_OK with every stage zeroed, but no public call
    # builds a dataset without rows (SBAG_EEMPTY, as Spark's "empty dataset"), so the
    # nearest reachable case is pinned instead: the refusal, and a one-row dataset no learner
    # leaves out (every stage zeroed)
    with pytest.raises(sb.SparkException):
        nat.DeviceDataset.from_numpy(X[:0], y[:0], ctx)
    one = nat.DeviceDataset.from_numpy(X[:1], y[:1], ctx)
    assert staged(ctx, forest, one, False, (False, 1.0, seed, 0), None).tobytes() == \
        np.zeros(L, STAGE_DTYPE).tobytes()
    one.free()
    still_good()


# ---------------------------------------------------------------- 10. model methods
@pytest.mark.parametrize("cls", [False, True])
def test_model_methods(ctx, cls):
    if cls:  # (9 features: at sampleRatio 0.6 every learner's subspace keeps a feature)
        rng = np.random.default_rng(11)
        X = np.round(rng.normal(size=(1500, 9)) * 6) / 8
        y = ((np.floor(3 * np.abs(X[:, 0])) + rng.integers(0, 3, 1500)) % 7).astype(np.float64)
        est = sb.BaggingClassifier().setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(5))
        est.setReplacement(False).setSampleRatio(0.6)
        metrics = ["accuracy"]
    else:
        X, y = order_case(ORDER_SEEDS[0])[:2]
        est = sb.BaggingRegressor().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(5))
        est.setReplacement(True)
        metrics = ["rmse", "mse", "mae"]
    est.setNumBaseLearners(6)
    N = len(y)
    frame = sb.Frame(X, y, partition_offsets=[0, 700, N])
    model = est.fit(frame)
    bound = 2 * (N - 1) * 2.0 ** -53  # two summation orders of N non-negative terms
    for m in metrics + [None]:
        curve = model.oobScoreCurve(frame, m)
        score = model.oobScore(frame, m)
        assert curve["metric"] == score["metric"] and curve["numRows"] == N
        assert curve["values"].shape == curve["coverage"].shape == (model.numBaseModels,)
        assert curve["coverage"][-1] == score["coverage"]
        assert abs(curve["values"][-1] - score["value"]) <= bound * abs(score["value"])
        assert (np.diff(curve["coverage"]) >= 0).all()
    with pytest.raises(sb.IllegalArgumentException):
        model.oobScoreCurve(frame, "r2")
    # the unmasked curve: a Frame, (X, y) and a DeviceDataset give the same curve; its last
    # entry is the plain transform's score
    held = model.evaluateEachIteration(frame)
    assert held["values"].shape == (model.numBaseModels,) and (held["coverage"] == 1.0).all()
    ds = frame.device_dataset(ctx)
    for other in (model.evaluateEachIteration((X, y)), model.evaluateEachIteration(ds)):
        np.testing.assert_array_equal(other["values"], held["values"])
    # (as oobScoreCurve on the fitted device dataset, with the fit's partitions)
    np.testing.assert_array_equal(model.oobScoreCurve(ds, None, [0, 700, N])["values"],
                                  model.oobScoreCurve(frame)["values"])
    ds.free()
    plain = oob_metrics(model.transform(X), np.ones(N, np.int32), y, cls)
    assert abs(held["values"][-1] - plain["value"]) <= bound * abs(plain["value"])
