"""GPU: out-of-bag predictions under permuted features (sbag_predict_oob_permuted) against
the CPU oracle.

Expected values are composed from the oracle's own pieces, as tests/test_gpu_oob.py does:
for slot k, Xp = X.copy(); Xp[:, j] = X[src[k], j]; the oracle forest's per-tree predictions
of Xp; and the literal row-by-row out-of-bag rule (test_gpu_oob.oob_by_rows) over
oracle.bag's counts.  Everything is compared bit for bit (assert_array_equal treats NaNs as
equal)."""
import numpy as np
import pytest

import oracle
from test_gpu_oob import fit_native, oob_by_rows, oracle_side, tree_bytes

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_permutation_importance, permutation_source_rows

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def composed(orf, X, counts, cls, feats, src):
    """[K, N]: the oracle's out-of-bag predictions with feature feats[k] read from rows src[k]."""
    out = []
    for j, s in zip(feats, src):
        Xp = X.copy()
        Xp[:, j] = X[s, j]
        _, per_tree = oracle.predict(orf, Xp, cls, per_tree=True)
        out.append(oob_by_rows(counts, per_tree, cls)[0])
    return np.stack(out)


def native_perm(ctx, forest, ds, feats, src, *, cls, replacement, ratio, seed, lb, L, part, **_):
    return nat.predict_oob_permuted(ctx, forest, ds, replacement=replacement, sample_ratio=ratio, seed=seed,
                                    learner_begin=lb, learner_end=lb + L, partition_offsets=part,
                                    agg=nat.AGG_MODE if cls else nat.AGG_MEAN, features=feats, src_rows=src)


def native_plain(ctx, forest, ds, *, cls, replacement, ratio, seed, lb, L, part, **_):
    return nat.predict_oob(ctx, forest, ds, replacement=replacement, sample_ratio=ratio, seed=seed,
                           learner_begin=lb, learner_end=lb + L, partition_offsets=part,
                           agg=nat.AGG_MODE if cls else nat.AGG_MEAN)


def assert_perm_equal(got, want_perm, want_base):
    perm, base, n_oob = got
    assert perm.dtype == np.float64 and base.dtype == np.float64 and n_oob.dtype == np.int32
    np.testing.assert_array_equal(n_oob, want_base[1])
    np.testing.assert_array_equal(base, want_base[0])
    np.testing.assert_array_equal(perm, want_perm)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. sampler regimes x impurity
N1, F1 = 1300, 10  # two full 512-row tiles + a 276-row tail
PART1 = [0, 300, 300, 811, 1300]
REGIMES = [(True, 1.0, 8, 0), (False, 0.5, 8, 0), (True, 0.63, 5, 3)]
FEATS1 = list(range(F1))
SRC1 = np.stack([np.random.default_rng(100 + j).permutation(N1) for j in FEATS1]).astype(np.int32)


@pytest.fixture(scope="module")
def data1():
    rng = np.random.default_rng(11)
    X = np.round(rng.normal(size=(N1, F1)) * 6) / 8  # u8 codes
    X[:, 9] = 0.375  # constant: no tree can test it
    kc = rng.integers(0, 3, N1)
    kr = rng.integers(-400, 400, N1)
    reg = kr / 16 + X[:, 0] / 4 + 8 * X[:, 3]
    cls = ((np.floor(3 * np.abs(X[:, 0])) + np.floor(2 * np.abs(X[:, 3])) + kc) % 7).astype(np.float64)
    return X, {False: reg, True: cls}


_cases1 = {}


def case1(ctx, data1, regime, cls):
    """One fit of a regime on both sides and its composed expectation, shared by the tests."""
    key = (regime, cls)
    if key not in _cases1:
        X, ys = data1
        replacement, ratio, L, lb = regime
        p = dict(cls=cls, replacement=replacement, ratio=ratio, seed=SEED_CLS if cls else SEED_REG, lb=lb,
                 L=L, depth=6, part=PART1)
        ds = nat.DeviceDataset.from_numpy(X, ys[cls], ctx)
        assert ds.layout()[3] == 1
        forest = fit_native(ctx, ds, **p)
        orf, counts, per_tree, _ = oracle_side(X, ys[cls], **p)
        base = oob_by_rows(counts, per_tree, cls)
        _cases1[key] = (ds, forest, p, orf, counts, base, composed(orf, X, counts, cls, FEATS1, SRC1))
    return _cases1[key]


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
def test_sampler_regimes(ctx, data1, regime, cls):
    ds, forest, p, _, _, base, want = case1(ctx, data1, regime, cls)
    covered = base[1] > 0
    assert covered.any() and (~covered).any()
    changed = [(want[k][covered] != base[0][covered]).sum() for k in range(F1)]
    assert changed[3] >= 300
    assert all(changed[k] >= 1 for k in range(9))
    assert want[9].tobytes() == base[0].tobytes()
    assert_perm_equal(native_perm(ctx, forest, ds, FEATS1, SRC1, **p), want, base)


# ---------------------------------------------------------------- 2. identity and constant maps
@pytest.mark.parametrize("cls", [False, True])
def test_identity_and_constant_maps(ctx, data1, cls):
    ds, forest, p, orf, counts, base, _ = case1(ctx, data1, REGIMES[0], cls)
    X = data1[0]
    feats = [0, 3, 5, 9]
    ident = np.tile(np.arange(N1, dtype=np.int32), (len(feats), 1))
    perm, b, n = native_perm(ctx, forest, ds, feats, ident, **p)
    plain = native_plain(ctx, forest, ds, **p)
    assert b.tobytes() == plain[0].tobytes() and n.tobytes() == plain[1].tobytes()
    for k in range(len(feats)):
        assert perm[k].tobytes() == b.tobytes()
    const = np.zeros((len(feats), N1), np.int32)  # every row reads the feature from row 0
    want = composed(orf, X, counts, cls, feats, const)
    assert ((want[1] != base[0]) & (base[1] > 0)).any()
    assert_perm_equal(native_perm(ctx, forest, ds, feats, const, **p), want, base)


# ---------------------------------------------------------------- 3. one feature in several slots
@pytest.mark.parametrize("cls", [False, True])
def test_the_same_feature_in_three_slots(ctx, data1, cls):
    """A slot set with several bits for one feature, next to a slot of another feature."""
    ds, forest, p, orf, counts, base, want1 = case1(ctx, data1, REGIMES[0], cls)
    feats = [3, 0, 3, 3]
    src = np.stack([SRC1[3], SRC1[0], SRC1[5], SRC1[7]])
    want = composed(orf, data1[0], counts, cls, feats, src)
    assert want[0].tobytes() == want1[3].tobytes() and want[1].tobytes() == want1[0].tobytes()
    covered = base[1] > 0
    assert (want[0][covered] != want[2][covered]).any() and (want[2][covered] != want[3][covered]).any()
    assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want, base)


# ---------------------------------------------------------------- 4. feature and learner batches
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("knobs", [{"SBAG_OOBP_BATCH_FEATURES": "1"}, {"SBAG_OOBP_BATCH_FEATURES": "3"},
                                   {"SBAG_OOB_BATCH_LEARNERS": "3"},
                                   {"SBAG_OOBP_BATCH_FEATURES": "3", "SBAG_OOB_BATCH_LEARNERS": "3"}],
                         ids=lambda k: ",".join(f"{a[5:]}={b}" for a, b in k.items()))
def test_batching_gives_the_same_bytes(ctx, data1, monkeypatch, knobs, cls):
    ds, forest, p, _, _, base, want = case1(ctx, data1, REGIMES[0], cls)
    one = native_perm(ctx, forest, ds, FEATS1, SRC1, **p)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    got = native_perm(ctx, forest, ds, FEATS1, SRC1, **p)
    assert same_bytes(got, one)
    assert_perm_equal(got, want, base)


@pytest.mark.parametrize("cls", [False, True])
def test_more_slots_than_one_launch_holds(ctx, data1, cls):
    """40 slots (every feature four times, each with its own permutation).  A slot takes at
    least 512 x 9 bytes of LDS, so beside a 16 KB chunk no launch holds more than 31: the
    host splits the slots into feature batches on its own."""
    ds, forest, p, orf, counts, base, want1 = case1(ctx, data1, REGIMES[0], cls)
    feats = [k % F1 for k in range(40)]
    src = np.stack([SRC1[k] if k < F1 else np.random.default_rng(600 + k).permutation(N1) for k in range(40)])
    src = src.astype(np.int32)
    want = composed(orf, data1[0], counts, cls, feats, src)
    np.testing.assert_array_equal(want[:F1], want1)
    covered = base[1] > 0
    assert (want[13][covered] != want[3][covered]).any() and (want[33][covered] != want[23][covered]).any()
    assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want, base)


# ---------------------------------------------------------------- 5. u16 codes, several LDS chunks
_case_u16 = {}


@pytest.mark.parametrize("batch", [None, "7"])
def test_several_lds_chunks_u16_codes(ctx, monkeypatch, batch):
    """24 depth-9 trees take several LDS chunks; a batch of 7 learners ends inside a chunk."""
    if not _case_u16:
        rng = np.random.default_rng(12)
        N = 20000
        X = np.round(rng.normal(size=(N, 6)), 3)
        y = rng.integers(-400, 400, N) / 16 + np.round(X[:, 0] * 8) / 32
        p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=24, depth=9, part=[0, N // 3, N])
        orf, counts, per_tree, _ = oracle_side(X, y, **p)
        tb = tree_bytes(orf)
        assert sum(tb) > 2 * 65536 and max(tb) <= 65536
        feats = [0, 4]
        src = np.stack([np.random.default_rng(200 + j).permutation(N) for j in feats]).astype(np.int32)
        base = oob_by_rows(counts, per_tree, False)
        want = composed(orf, X, counts, False, feats, src)
        assert all(((want[k] != base[0]) & (base[1] > 0)).sum() >= 100 for k in range(2))
        _case_u16.update(X=X, y=y, p=p, feats=feats, src=src, base=base, want=want)
    c = _case_u16
    ds = nat.DeviceDataset.from_numpy(c["X"], c["y"], ctx)
    assert ds.layout()[3] == 2
    forest = fit_native(ctx, ds, **c["p"])
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    assert_perm_equal(native_perm(ctx, forest, ds, c["feats"], c["src"], **c["p"]), c["want"], c["base"])
    ds.free()


# ---------------------------------------------------------------- 6. the fallback
def _perms(N, feats, seed):
    return np.stack([np.random.default_rng(seed + j).permutation(N) for j in feats]).astype(np.int32)


def test_fallback_u32_codes(ctx):
    rng = np.random.default_rng(13)
    N = 70000
    X = np.stack([rng.permutation(N) / 4.0, rng.permutation(N) * 1.0], axis=1)  # distinct values
    y = rng.integers(-400, 400, N) / 16 + np.floor(X[:, 0] / 2048)
    p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=3, depth=5, part=[0, 30001, N])
    orf, counts, per_tree, _ = oracle_side(X, y, **p)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    assert ds.layout()[3] == 4
    forest = fit_native(ctx, ds, **p)
    feats, src = [0, 1], _perms(N, [0, 1], 300)
    base = oob_by_rows(counts, per_tree, False)
    want = composed(orf, X, counts, False, feats, src)
    assert ((want[0] != base[0]) & (base[1] > 0)).sum() >= 100
    assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want, base)
    ds.free()


def test_fallback_trees_past_the_lds_chunk(ctx):
    rng = np.random.default_rng(12)
    N = 40000
    X = np.round(rng.normal(size=(N, 4)), 3)
    y = rng.integers(-400, 400, N) / 16 + np.round(X[:, 0] * 8) / 32
    p = dict(cls=False, replacement=True, ratio=1.0, seed=SEED_REG, lb=0, L=3, depth=14, part=[0, N // 3, N])
    orf, counts, per_tree, _ = oracle_side(X, y, **p)
    assert max(tree_bytes(orf)) > 65536  # plan_tiled must refuse
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = fit_native(ctx, ds, **p)
    feats, src = [0, 2], _perms(N, [0, 2], 400)
    base = oob_by_rows(counts, per_tree, False)
    want = composed(orf, X, counts, False, feats, src)
    assert all(((want[k] != base[0]) & (base[1] > 0)).sum() >= 100 for k in range(2))
    assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want, base)
    ds.free()


@pytest.mark.parametrize("batch", [None, "4"])
def test_fallback_more_classes_than_the_lds_counters(ctx, monkeypatch, batch):
    """400 classes, built as test_gpu_oob.test_more_classes_than_the_lds_counters builds them."""
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
    assert per_tree.max() == 399.0 and (per_tree >= 320).mean() > 0.1
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    forest = nat.NativeForest.from_trees([orf.tree(t)[0].astype(nat.NODE_DTYPE) for t in range(L)],
                                         orf.subspaces, nat.IMPURITY_GINI)
    tested = sorted({int(orf.subspaces[t][f]) for t in range(L)
                     for f in orf.tree(t)[0]["feature"][orf.tree(t)[0]["left"] >= 0]})
    feats = tested[:2]
    src = _perms(N, feats, 500)
    base = oob_by_rows(counts, per_tree, True)
    want = composed(orf, X, counts, True, feats, src)
    assert all(((want[k] != base[0]) & (base[1] > 0)).sum() >= 20 for k in range(2))
    if batch:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", batch)
    assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want, base)
    ds.free()


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("learners", [None, "3"])
def test_forced_fallback_equals_the_fused_pass(ctx, data1, monkeypatch, cls, learners):
    ds, forest, p, _, _, base, want = case1(ctx, data1, REGIMES[0], cls)
    fused = native_perm(ctx, forest, ds, FEATS1, SRC1, **p)
    monkeypatch.setenv("SBAG_OOBP_FORCE_FALLBACK", "1")
    if learners:
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", learners)
    slow = native_perm(ctx, forest, ds, FEATS1, SRC1, **p)
    assert same_bytes(slow, fused)
    assert_perm_equal(slow, want, base)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_context_usable(ctx, data1):
    ds, forest, p, _, _, base, want = case1(ctx, data1, REGIMES[0], False)
    feats, src = [3, 0], SRC1[[3, 0]]

    def good():
        assert_perm_equal(native_perm(ctx, forest, ds, feats, src, **p), want[[3, 0]], base)

    for bad_row in (N1, -1):
        bad = src.copy()
        bad[1, 777] = bad_row
        with pytest.raises(sb.IllegalArgumentException):
            native_perm(ctx, forest, ds, feats, bad, **p)
        good()
    for bad_feat in (F1, -1):
        with pytest.raises(sb.IllegalArgumentException):
            native_perm(ctx, forest, ds, [3, bad_feat], src, **p)
        good()
    perm, b, n = native_perm(ctx, forest, ds, [], np.zeros((0, N1), np.int32), **p)
    assert perm.shape == (0, N1)
    np.testing.assert_array_equal(b, base[0])
    np.testing.assert_array_equal(n, base[1])


# ---------------------------------------------------------------- 8. model API
@pytest.mark.parametrize("cls", [False, True])
def test_model_api(ctx, data1, tmp_path, monkeypatch, cls):
    X, ys = data1
    y = ys[cls]
    part = [0, 300, 811, 1300]
    frame = sb.Frame(X, y, partition_offsets=part)
    if cls:
        est = sb.BaggingClassifier().setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(6))
        est.setReplacement(False).setSampleRatio(0.6)
        seed, model_cls = SEED_CLS, sb.BaggingClassificationModel
    else:
        est = sb.BaggingRegressor().setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(6))
        est.setReplacement(True)
        seed, model_cls = SEED_REG, sb.BaggingRegressionModel
    est.setNumBaseLearners(8)
    p = dict(cls=cls, replacement=est.getReplacement(), ratio=est.getSampleRatio(), seed=seed, depth=6, part=part)
    PSEED = 5

    def want_for(lb, L, feats, repeats, metric=None):
        orf, counts, per_tree, _ = oracle_side(X, y, lb=lb, L=L, **p)
        base = oob_by_rows(counts, per_tree, cls)
        per = []
        for r in range(repeats):
            src = [permutation_source_rows(PSEED, r, j, N1) for j in feats]
            res = oob_permutation_importance(base[0], composed(orf, X, counts, cls, feats, src), base[1], y, cls,
                                             metric)
            per.append(res["importance"])
        return res["metric"], res["baseline"], np.stack(per)

    def check(got, want, feats):
        metric, baseline, per = want
        assert got["metric"] == metric and got["baseline"] == baseline
        assert got["features"] == feats
        np.testing.assert_array_equal(got["perRepeat"], per)
        total = np.zeros(len(feats))
        for r in range(len(per)):
            total = total + per[r]
        np.testing.assert_array_equal(got["importances"], total / len(per))
        np.testing.assert_array_equal(got["std"], per.std(axis=0))

    sent = []
    real = nat.predict_oob_permuted

    def recording(*a, **kw):
        sent.extend(int(j) for j in kw["features"])
        return real(*a, **kw)

    monkeypatch.setattr(nat, "predict_oob_permuted", recording)
    model = est.fit(frame)
    want = want_for(0, 8, FEATS1, 2)
    got = model.permutationImportances(frame, numRepeats=2, seed=PSEED)
    check(got, want, FEATS1)
    assert got["metric"] == ("accuracy" if cls else "rmse")
    assert got["importances"][9] == 0.0 and (got["perRepeat"][:, 9] == 0.0).all()
    assert 9 not in sent and 3 in sent  # the constant feature never reaches the device
    assert got["importances"][3] > 0.0
    if not cls:  # another metric, a subset of the features in their own order
        check(model.permutationImportances(frame, features=[3, 9, 0], seed=PSEED, metricName="r2"),
              want_for(0, 8, [3, 9, 0], 1, "r2"), [3, 9, 0])
    # the fitted device dataset serves as well, with the fit's partitions
    ds = frame.device_dataset(ctx)
    check(model.permutationImportances(ds, numRepeats=2, seed=PSEED, partition_offsets=part), want, FEATS1)
    ds.free()
    # save / load
    path = str(tmp_path / "model")
    model.save(path)
    back = model_cls.load(path)
    check(back.permutationImportances(frame, numRepeats=2, seed=PSEED), want, FEATS1)
    # a fit_range shard: learners 2..5 with their own bags
    shard = est.fit_range(frame, 2, 6)
    check(shard.permutationImportances(frame, features=[0, 3, 9], seed=PSEED), want_for(2, 4, [0, 3, 9], 1),
          [0, 3, 9])
