"""GPU: the bags' Gram matrix (sbag_bag_gram / sbag_counts_gram, exact integers, k_gram_mfma and
k_gram_dot) and the infinitesimal-jackknife variance (sbag_predict_variance / _dataset, bit for bit
against ij_ref.py over nat.predict(per_tree=True), k_ij_tiled and the general path)."""
from fractions import Fraction

import numpy as np
import pytest

import ij_ref
import weighted_ref as wr

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

GRAM_KNOB, IJ_KNOB = "SBAG_GRAM_FORCE_FALLBACK", "SBAG_IJ_FORCE_FALLBACK"
SLICE = 65536


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def same_bits(got, want, label=""):
    np.testing.assert_array_equal(got, want, err_msg=label)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.signbit(got)[ok], np.signbit(want)[ok], err_msg=label)


def knob(monkeypatch, name, force):
    monkeypatch.delenv(name, raising=False) if force is None else monkeypatch.setenv(name, force)


def check_gram(monkeypatch, call, C, label=""):
    want = C.astype(np.int64) @ C.astype(np.int64).T
    for force in (None, "1"):
        knob(monkeypatch, GRAM_KNOB, force)
        got = call()
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want, err_msg=f"{label} force={force}")
    knob(monkeypatch, GRAM_KNOB, None)


@pytest.mark.parametrize("N", [1, 15, 255, 256, 257, SLICE + 17])
def test_counts_gram_random(ctx, monkeypatch, N):
    rng = np.random.default_rng(N)
    for T in [1, 2, 31, 32, 33, 64, 65] + ([129] if N > SLICE else []):
        C = rng.integers(0, 6, size=(T, N)).astype(np.uint8)
        check_gram(monkeypatch, lambda: nat.counts_gram(ctx, C), C, f"T={T}")


def test_counts_gram_int32_edge(ctx, monkeypatch):
    """All bytes 127 over a full slice plus 17 rows: 127 * 127 * 65 536 is the largest sum an int32
    accumulator of k_gram_mfma has to hold."""
    C = np.full((33, SLICE + 17), 127, np.uint8)
    check_gram(monkeypatch, lambda: nat.counts_gram(ctx, C), C)
    assert nat.counts_gram(ctx, np.zeros((3, 0), np.uint8)).tolist() == [[0] * 3] * 3


@pytest.mark.parametrize("byte", [128, 255])
def test_counts_gram_past_int8(ctx, monkeypatch, byte):
    """One byte the int8 kernel cannot take, in the first row, the last one and on either side of
    the slice edge: the flag, then k_gram_dot."""
    N = SLICE + 17
    base = np.random.default_rng(byte).integers(0, 6, size=(33, N)).astype(np.uint8)
    for learner, row in [(0, 0), (32, N - 1), (7, SLICE - 1), (31, SLICE)]:
        C = base.copy()
        C[learner, row] = byte
        check_gram(monkeypatch, lambda: nat.counts_gram(ctx, C), C, f"at {(learner, row)}")


@pytest.mark.parametrize("replacement,ratio,parts,lb", [
    (True, 1.0, None, 0), (True, 0.3, None, 0), (False, 0.5, None, 0), (False, 1.0, None, 0),
    (True, 1.0, [0, 400, 400, 1003], 0), (True, 0.3, None, 5)],
    ids=["poisson", "poisson-0.3", "bernoulli", "all-in-bag", "P3-one-empty", "learner-begin"])
def test_bag_gram(ctx, monkeypatch, replacement, ratio, parts, lb):
    N, T = 1003, 33
    C = nat.sample(ctx, replacement, ratio, 11, lb, lb + T, N, parts)
    check_gram(monkeypatch, lambda: nat.bag_gram(ctx, replacement=replacement, sample_ratio=ratio, seed=11,
                                                 learner_begin=lb, learner_end=lb + T, num_rows=N,
                                                 partition_offsets=parts), C)
    if not replacement and ratio == 1.0:
        assert (C.astype(np.int64) @ C.astype(np.int64).T == N).all()


def check_variance(ctx, monkeypatch, f, X, ds, gram):
    """Host rows and the dataset, the tiled and the general path: all equal to the reference, and
    the mean byte for byte nat.predict's."""
    X = np.ascontiguousarray(X, np.float64)
    mean, pt = nat.predict(ctx, f, X, nat.AGG_MEAN, per_tree=True)
    m, v_ij, v_iju, _ = ij_ref.variance(pt, gram)
    want = np.column_stack([m, v_ij, v_iju])
    assert m.tobytes() == mean.tobytes()
    for force in (None, "1"):
        knob(monkeypatch, IJ_KNOB, force)
        same_bits(nat.predict_variance(ctx, f, X, gram), want, f"host rows, force={force}")
        if ds is not None:
            same_bits(nat.predict_variance_dataset(ctx, f, ds, gram), want, f"dataset, force={force}")
    knob(monkeypatch, IJ_KNOB, None)
    return want


def features(rng, N, F, cb):
    """u8 codes: 50 distinct values a feature; u16: feature 0 has N distinct ones."""
    X = rng.integers(0, 50, size=(N, F)).astype(np.float64)
    if cb == 2:
        X[:, 0] = rng.permutation(N) * 0.5
    return X


SAMPLER = dict(replacement=True, sample_ratio=0.8, seed=11, learner_begin=0)


def fitted(ctx, X, y, L):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    f = nat.fit(ctx, ds, max_depth=3, impurity=nat.IMPURITY_VARIANCE, learner_end=L, **SAMPLER)
    return ds, f


@pytest.mark.parametrize("labels", ["integer", "normal"])
@pytest.mark.parametrize("L", [1, 2, 31, 33, 64, 65, 129])
def test_tree_counts(ctx, monkeypatch, L, labels):
    """Depth-3 fits of L trees on 1000 x 6 rows: a short last tile, a last group of 1, 2 and 3
    chains, one to four units a pass; integer labels give many d = 0."""
    rng = np.random.default_rng(L)
    gram = nat.bag_gram(ctx, learner_end=L, num_rows=1000, **SAMPLER)
    for cb in (1, 2):
        X = features(rng, 1000, 6, cb)
        y = rng.integers(0, 4, 1000).astype(np.float64) if labels == "integer" else rng.normal(size=1000)
        ds, f = fitted(ctx, X, y, L)
        try:
            assert ds.layout()[3] == cb
            check_variance(ctx, monkeypatch, f, X, ds, gram)
        finally:
            f.free()
            ds.free()


def test_hand_built_forests(ctx, monkeypatch):
    X = (np.arange(700) % 10).astype(np.float64)[:, None]
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(700), ctx)

    def run(trees, gram):
        f = nat.NativeForest.from_trees(trees, [[0]] * len(trees), nat.IMPURITY_VARIANCE)
        try:
            return check_variance(ctx, monkeypatch, f, X, ds, gram)
        finally:
            f.free()

    try:
        C = np.random.default_rng(1).integers(0, 4, size=(3, 50)).astype(np.int64)
        z = run([wr.stump(4.5, 2.5, 2.5), wr.leaf(2.5), wr.stump(1.5, 2.5, 2.5)], C @ C.T)
        assert (z[:, 0] == 2.5).all() and (z[:, 1:] == 0).all() and not np.signbit(z[:, 1:]).any()
        # rows 1 .. 8 see both leaves: every d_a * u_a is about 2^50 * 1e300 and q overflows to
        # +inf; rows 0 and 9 see one leaf from every tree (d = 0)
        big = run([wr.stump(t + 0.5, -1e150, 1e150) for t in range(9)],
                  np.ones((9, 9), np.int64) + (np.eye(9, dtype=np.int64) << 50))
        mixed = (X[:, 0] > 0) & (X[:, 0] < 9)
        assert np.isposinf(big[mixed, 1]).all() and (big[~mixed, 1] == 0).all()
    finally:
        ds.free()


def test_against_the_definition(ctx):
    """v_ij against sum_i (sum_b c[b][i] d_b)^2 / T^2 in exact arithmetic, straight from the
    counts and the rule's fp64 d_b (neither G nor the triangle form): within
    gamma * sum_ab |d_a| G[a][b] |d_b| / T^2, gamma = k u / (1 - k u), k = 2 T + 2, u = 2^-53: a
    term d_a G[a][b] d_b goes through at most T + 2 + a <= k rounded operations."""
    T, N, NQ = 33, 300, 64
    rng = np.random.default_rng(5)
    X = features(rng, N, 6, 1)
    ds, f = fitted(ctx, X, rng.normal(size=N), T)
    try:
        C = nat.sample(ctx, True, 0.8, 11, 0, T, N).astype(np.int64)
        gram = nat.bag_gram(ctx, learner_end=T, num_rows=N, **SAMPLER)
        Xq = np.ascontiguousarray(X[:NQ])
        out = nat.predict_variance(ctx, f, Xq, gram)
        _, pt = nat.predict(ctx, f, Xq, nat.AGG_MEAN, per_tree=True)
    finally:
        f.free()
        ds.free()
    d = pt - out[:, 0]
    ku = Fraction(2 * T + 2, 2 ** 53)
    gamma = ku / (1 - ku)
    G = [[int(v) for v in row] for row in gram]
    cols = [[int(v) for v in C[:, i]] for i in range(N)]
    for r in range(NQ):
        D = [int(Fraction(float(v)) * 2 ** 1074) for v in d[:, r]]  # exact: d_b * 2^1074
        exact = sum(sum(c * x for c, x in zip(col, D)) ** 2 for col in cols)
        bound = gamma * sum(abs(D[a]) * G[a][b] * abs(D[b]) for a in range(T) for b in range(T))
        got = Fraction(float(out[r, 1])) * T * T * 2 ** 2148
        assert abs(got - exact) <= bound, (r, float(abs(got - exact) / bound))
    # centring the counts is moot once d is centred about the exact mean (row 0)
    t = [Fraction(float(v)) for v in pt[:, 0]]
    mean = sum(t) / T
    dc = [v - mean for v in t]
    plain = sum(sum(c * x for c, x in zip(col, dc)) ** 2 for col in cols)
    centred = sum(sum((c - Fraction(sum(col), T)) * x for c, x in zip(col, dc)) ** 2 for col in cols)
    assert abs(plain - centred) <= gamma * sum(abs(dc[a]) * G[a][b] * abs(dc[b]) for a in range(T) for b in range(T))


def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    X = (np.arange(300) % 7).astype(np.float64)[:, None]
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(300), ctx)
    var = nat.NativeForest.from_trees([wr.stump(2.5, 1.0, 2.0), wr.stump(4.5, 0.0, 5.0)], [[0]] * 2,
                                      nat.IMPURITY_VARIANCE)
    gin = nat.NativeForest.from_trees([wr.stump(2.5, 0, 2)] * 2, [[0]] * 2, nat.IMPURITY_GINI)
    nan = nat.NativeForest.from_trees([wr.stump(2.5, 1.0, np.nan)] * 2, [[0]] * 2, nat.IMPURITY_VARIANCE)
    big = nat.NativeForest.from_trees([wr.stump(2.5, 1.0, 2.0)] * 1025, [[0]] * 1025, nat.IMPURITY_VARIANCE)
    g2 = np.array([[300, 90], [90, 280]], np.int64)
    try:
        good = check_variance(ctx, monkeypatch, var, X, ds, g2)
        cases = [(gin, g2, nat.SBAG_EINVAL), (nan, g2, nat.SBAG_EINVAL),
                 (var, np.array([[1 << 53, 0], [0, 1]], np.int64), nat.SBAG_EINVAL),
                 (var, np.array([[1, 0], [-1, 1]], np.int64), nat.SBAG_EINVAL),
                 (big, np.zeros((1025, 1025), np.int64), nat.SBAG_EUNSUPPORTED)]
        sampler = dict(replacement=True, sample_ratio=1.0, seed=1, learner_begin=0, num_rows=300)
        calls = [(lambda f=f, g=g: nat.predict_variance(ctx, f, X, g), code) for f, g, code in cases]
        calls += [(lambda f=f, g=g: nat.predict_variance_dataset(ctx, f, ds, g), code) for f, g, code in cases]
        calls += [(lambda: nat.bag_gram(ctx, learner_end=1025, **sampler), nat.SBAG_EUNSUPPORTED),
                  (lambda: nat.counts_gram(ctx, np.zeros((1025, 4), np.uint8)), nat.SBAG_EUNSUPPORTED),
                  (lambda: nat.bag_gram(ctx, learner_end=0, **sampler), nat.SBAG_EINVAL)]
        for call, code in calls:
            with pytest.raises(nat.SbagError) as e:
                call()
            assert e.value.code == code
            same_bits(nat.predict_variance_dataset(ctx, var, ds, g2), good)
        monkeypatch.setenv("SBAG_OOB_BATCH_LEARNERS", "3")
        with pytest.raises(nat.SbagError) as e:
            nat.bag_gram(ctx, learner_end=4, **sampler)
        assert e.value.code == nat.SBAG_EUNSUPPORTED
        assert nat.bag_gram(ctx, learner_end=3, **sampler).shape == (3, 3)
        monkeypatch.delenv("SBAG_OOB_BATCH_LEARNERS")
        assert nat.predict_variance(ctx, var, np.zeros((0, 1)), g2).shape == (0, 3)
    finally:
        ds.free()
        for f in (var, gin, nan, big):
            f.free()


def test_models(ctx):
    """The public interface: bagGram / predictVariance / predictStdError of a fitted regression
    model; the classification model refuses all three."""
    rng = np.random.default_rng(4)
    X = features(rng, 1000, 6, 1)
    y = X[:, 0] + rng.normal(size=1000)
    frame = sb.Frame(X, y)
    model = sb.BaggingRegressor().setNumBaseLearners(20).setBaseLearner(
        sb.DecisionTreeRegressor().setMaxDepth(3)).fit(frame)
    gram = model.bagGram(frame)
    assert gram.shape == (20, 20) and gram.dtype == np.int64 and (gram == gram.T).all()
    _, pt = model.transform(X, per_tree=True)
    m, v_ij, v_iju, _ = ij_ref.variance(pt, gram)
    same_bits(np.column_stack(model.predictVariance(X, gram)), np.column_stack([m, v_ij, v_iju]))
    same_bits(model.predictStdError(X, gram), np.sqrt(np.maximum(v_iju, 0.0)))
    same_bits(model.predictStdError(X, gram, corrected=False), np.sqrt(np.maximum(v_ij, 0.0)))
    assert (v_ij >= 0).all() and (v_ij > 0).any()
    cls = sb.BaggingClassifier().setNumBaseLearners(3).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(2)).fit(sb.Frame(X, (y > 20).astype(np.float64)))
    for call in (lambda: cls.bagGram(frame), lambda: cls.predictVariance(X, gram),
                 lambda: cls.predictStdError(X, gram)):
        with pytest.raises(sb.IllegalArgumentException):
            call()
