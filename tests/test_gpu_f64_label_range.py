"""GPU: the fp64 label engine (sbag_f64s.hip) across the whole range of label magnitudes,
and the label classes (dyadic / approximate image / integer engine) at their boundaries.

The screen (k_f64_screen) decides a node from integer histograms of the labels' fixed-point
image, which does not change when the labels are scaled by a power of two; Spark's sums of
y*y do change once they underflow (max|y| below about 1e-153) or overflow.  Every case here
is one fit compared bit for bit with the oracle (test_label_scale_host.py holds the oracle
itself to Python floats at these scales and records that its trees do change inside the
window).  No tolerance anywhere.

Overflow: the engine serves labels while draws x max|y| <= 2^511 (draws: the largest
in-bag size of the fit's learners), so that no sum, sum*sum or sum of squares of Spark's
can overflow, and refuses larger labels with SBAG_EUNSUPPORTED."""
import contextlib
import os

import numpy as np
import pytest

import oracle
from conftest import DATA
from parity_utils import assert_forest_equal, assert_tree_equal

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED = oracle.DEFAULT_SEED_REGRESSOR
L, DEPTH, BINS = 6, 9, 32
PARTS = {"p1": None, "p4": [0, 1000, 3000, 5000, 8192]}
KNOBS = ("SBAG_F64_SCREEN", "SBAG_F64_FALLBACK", "SBAG_F64_NO_CARRY", "SBAG_F64")


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


@pytest.fixture(scope="module")
def cpusmall():
    return sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))


@contextlib.contextmanager
def _env(**kw):
    """The library reads its knobs per fit: set them for one block, all others unset."""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _fit(ctx, X, y, part=None, learners=L, depth=DEPTH, min_inst=1, min_gain=0.0):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        return nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0,
                       learner_end=learners, partition_offsets=part, max_depth=depth, max_bins=BINS,
                       min_instances_per_node=min_inst, min_info_gain=min_gain,
                       impurity=nat.IMPURITY_VARIANCE)
    finally:
        ds.free()


def _bags(X, part, learners=L):
    N, F = X.shape
    counts = oracle.bag(True, 1.0, 0, learners, SEED, part if part is not None else [0, N], N)
    subs = [oracle.subspace(1.0, F, SEED + i) for i in range(learners)]
    return counts, subs


def _oracle(X, y, part=None, learners=L, depth=DEPTH, min_inst=1, min_gain=0.0):
    counts, subs = _bags(X, part, learners)
    return oracle.fit(X, y, counts, subs, max_depth=depth, max_bins=BINS, part=part,
                      min_instances_per_node=min_inst, min_info_gain=min_gain)


def _forest_bytes(forest):
    return [tuple(a.tobytes() for a in forest.tree(t)) for t in range(len(forest))]


def _check(ctx, forest, orf, X):
    """The forest equals the oracle's in every field, and so do the ensemble's predictions
    (NaN where the oracle has NaN)."""
    assert_forest_equal(forest, orf)
    got = nat.predict(ctx, forest, X, nat.AGG_MEAN)
    want = oracle.predict(orf, X)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)


def _scaled(y, k):
    return np.ldexp(y * np.pi, k)


# ------------------------------------------------------------------ 2. the exponent range
@pytest.fixture(scope="module")
def base_fallbacks(ctx, cpusmall):
    """exact_fallbacks of the k = 0 fit, screened and unscreened, per partitioning."""
    X, y = cpusmall
    out = {}
    for name, part in PARTS.items():
        with _env():
            screened = _fit(ctx, X, _scaled(y, 0), part).timing()["exact_fallbacks"]
        with _env(SBAG_F64_SCREEN="0"):
            unscreened = _fit(ctx, X, _scaled(y, 0), part).timing()["exact_fallbacks"]
        out[name] = (screened, unscreened)
    return out


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k", [-505, -100, 0, 100, 480])
def test_ordinary_range_equals_oracle_and_screens_alike(ctx, cpusmall, base_fallbacks, k, part):
    """Nothing under- or overflows in Spark's arithmetic: the oracle's forest, and exactly as
    many nodes sent to the exact fallback as at k = 0 -- the screen and its bound must not
    depend on the magnitude here -- which is below half of the unscreened engine's count."""
    X, y = cpusmall
    yk = _scaled(y, k)
    with _env():
        forest = _fit(ctx, X, yk, PARTS[part])
    _check(ctx, forest, _oracle(X, yk, PARTS[part]), X)
    screened, unscreened = base_fallbacks[part]
    print(f"k = {k} {part}: exact_fallbacks {forest.timing()['exact_fallbacks']}, k = 0: {screened}, "
          f"unscreened {unscreened}")
    assert forest.timing()["exact_fallbacks"] == screened
    assert screened < unscreened / 2


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k", [-512, -515, -518, -520, -523, -525, -526, -530, -535, -537, -540])
def test_underflow_window_equals_oracle(ctx, cpusmall, k, part):
    """max|y| in about [1e-161, 1e-153]: y*y and Spark's sums of squares are subnormal, its
    gains lose bits to gradual underflow and its trees are not the rescaled k = 0 trees.
    (-525 and -537 at one partition hold a node whose child impurity is an exact tie between
    two subnormals, 2027840901.5 and 7.5 ulps: Variance.calculate's division rounds it to
    even, the GPU's own division sequence did not.)"""
    X, y = cpusmall
    yk = _scaled(y, k)
    with _env():
        forest = _fit(ctx, X, yk, PARTS[part])
    print(f"k = {k} {part}: exact_fallbacks {forest.timing()['exact_fallbacks']}")
    _check(ctx, forest, _oracle(X, yk, PARTS[part]), X)


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k", [-560, -1040, -1065])
def test_below_the_window_equals_oracle(ctx, cpusmall, k, part):
    """Every y*y is 0 (-560: single-leaf trees), every label is subnormal (-1040), the labels
    are within a few ulps of the smallest subnormal (-1065)."""
    X, y = cpusmall
    yk = _scaled(y, k)
    assert np.abs(yk).max() > 0.0
    with _env():
        forest = _fit(ctx, X, yk, PARTS[part])
    orf = _oracle(X, yk, PARTS[part])
    _check(ctx, forest, orf, X)
    assert all(len(orf.tree(t)[0]) == 1 for t in range(L))


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k", [-520, -530])
def test_engines_agree_inside_the_window(ctx, cpusmall, k, part):
    """The unscreened engine, both exact fallbacks and the row-gathered labels give the
    default fit's bytes: if only the default fit differs from the oracle the screen is at
    fault, if all of them do the exact kernels are."""
    X, y = cpusmall
    yk = _scaled(y, k)
    with _env():
        default = _forest_bytes(_fit(ctx, X, yk, PARTS[part]))
    for knob in (dict(SBAG_F64_SCREEN="0"), dict(SBAG_F64_FALLBACK="hist"),
                 dict(SBAG_F64_FALLBACK="chain"), dict(SBAG_F64_NO_CARRY="1"),
                 dict(SBAG_F64_SCREEN="0", SBAG_F64_FALLBACK="hist"),
                 dict(SBAG_F64_SCREEN="0", SBAG_F64_FALLBACK="chain")):
        with _env(**knob):
            other = _fit(ctx, X, yk, PARTS[part])
        assert _forest_bytes(other) == default, knob
    assert_forest_equal(other, _oracle(X, yk, PARTS[part]))


def _largest_served_k(X, y, part):
    """The rule of DESIGN.md §4.7, restated: served while draws x max|y| <= 2^511."""
    counts, _ = _bags(X, part)
    draws = float(max(int(c.sum(dtype=np.int64)) for c in counts))
    k = 400
    while draws * float(np.abs(_scaled(y, k + 1)).max()) <= 2.0 ** 511:
        k += 1
    return k


@pytest.mark.parametrize("part", list(PARTS))
def test_largest_served_magnitude_equals_oracle(ctx, cpusmall, part):
    """The largest k the overflow rule serves: the oracle's forest, no NaN or inf in it; one
    more doubling is refused."""
    X, y = cpusmall
    k = _largest_served_k(X, y, PARTS[part])
    assert 480 < k < 495
    yk = _scaled(y, k)
    with _env():
        forest = _fit(ctx, X, yk, PARTS[part])
    orf = _oracle(X, yk, PARTS[part])
    for t in range(L):
        nodes, stats = orf.tree(t)
        assert np.isfinite(stats).all() and np.isfinite(nodes["gain"]).all() and np.isfinite(nodes["impurity"]).all()
    _check(ctx, forest, orf, X)
    with _env(), pytest.raises(nat.SparkException, match=r"max\|y\|") as ei:
        _fit(ctx, X, _scaled(y, k + 1), PARTS[part])
    assert ei.value.code == nat.SBAG_EUNSUPPORTED


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k", [495, 500, 1000])
def test_overflowing_labels_are_refused(ctx, cpusmall, k, part):
    """n max|y|^2 (495, 500) or y*y itself (1000) is infinite in Spark's arithmetic; its trees
    there are 3-node stumps with NaN gains.  The engine refuses such labels rather than
    return any forest, and names the label magnitude."""
    X, y = cpusmall
    yk = _scaled(y, k)
    assert np.isfinite(yk).all()
    with _env(), pytest.raises(nat.SparkException, match=r"max\|y\|") as ei:
        _fit(ctx, X, yk, PARTS[part])
    assert ei.value.code == nat.SBAG_EUNSUPPORTED


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("case", ["outliers_1e9", "window_inside_one_column"])
def test_mixed_magnitudes_equal_oracle(ctx, cpusmall, case, part):
    """Three outliers 1e12 (1e15) times the other labels: most of the image is 0 and its
    rounding error dominates every gain but those of the splits that isolate the outliers.
    The second set puts the outliers at 1e-150 and the rest at 1e-165 y, so the squares of
    one column span normal, subnormal and zero."""
    X, y = cpusmall
    if case == "outliers_1e9":
        y2 = 1e-3 * y
        y2[[7, 4000, 8191]] = [1e9, -1e9, 3e8]
    else:
        y2 = 1e-165 * y
        y2[[7, 4000, 8191]] = [1e-150, -1e-150, 3e-151]
    with _env():
        forest = _fit(ctx, X, y2, PARTS[part])
    _check(ctx, forest, _oracle(X, y2, PARTS[part]), X)


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("k,min_gain", [(0, 3.0), (-100, 3.0 * 2.0 ** -200), (-520, 3.0 * 2.0 ** -1040),
                                        (480, 3.0 * 2.0 ** 960), (480, 1e-30), (0, 5e-324), (-600, 0.5)],
                         ids=["k0", "k-100", "k-520", "k480", "k480-tiny-gain", "k0-smallest-gain",
                              "k-600-huge-gain"])
def test_min_info_gain_at_every_scale(ctx, cpusmall, k, min_gain, part):
    """minInfoGain is an absolute threshold on Spark's gain, and the screen compares it in
    the labels' own units: thresholds that scale with the labels exactly (the first four: 3.0
    prunes much of the k = 0 forest), one that is far below every gain and is rounded in
    those units, the smallest positive Double, and one far above every gain of labels so
    small that it overflows in them.  minInstancesPerNode 5."""
    X, y = cpusmall
    yk = _scaled(y, k)
    with _env():
        forest = _fit(ctx, X, yk, PARTS[part], min_inst=5, min_gain=min_gain)
    orf = _oracle(X, yk, PARTS[part], min_inst=5, min_gain=min_gain)
    print(f"k = {k} min_gain {min_gain} {part}: nodes {[len(orf.tree(t)[0]) for t in range(L)]}, "
          f"exact_fallbacks {forest.timing()['exact_fallbacks']}")
    _check(ctx, forest, orf, X)


@pytest.mark.parametrize("learners", [2, 6])
def test_mean_of_subnormal_predictions(ctx, learners):
    """transform's mean where it is subnormal (trees fitted on labels below 2^-1022 predict
    such values): one comb tree whose leaf for x = j predicts j ulps and learners - 1 leaves
    of 1 ulp, so the sums (j + learners - 1) ulps over `learners` hit every remainder, exact
    ties among them, which IEEE division rounds to even."""
    ulp = 5e-324
    n = 64
    comb = np.zeros(2 * (n - 1) + 1, nat.NODE_DTYPE)
    comb["id"] = np.arange(len(comb))
    comb["left"] = comb["right"] = comb["feature"] = -1
    i = 2 * np.arange(n - 1)
    comb["left"][i], comb["right"][i], comb["feature"][i] = i + 1, i + 2, 0
    comb["threshold"][i] = np.arange(n - 1)
    comb["prediction"][np.concatenate([i + 1, [2 * (n - 1)]])] = np.arange(n) * ulp
    one = np.zeros(1, nat.NODE_DTYPE)
    one["left"] = one["right"] = one["feature"] = -1
    one["prediction"] = ulp
    trees = [comb] + [one] * (learners - 1)
    subs = [np.array([0], np.int32)] * learners
    X = np.arange(n, dtype=np.float64)[:, None]
    want = np.array([float(j + learners - 1) * ulp / float(learners) for j in range(n)])
    assert len(np.unique(want)) > n // learners - 2
    f = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_VARIANCE)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(n), ctx)
    try:
        got, pt = nat.predict(ctx, f, X, nat.AGG_MEAN, per_tree=True)
        np.testing.assert_array_equal(pt[0], np.arange(n) * ulp)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(nat.predict_dataset(ctx, f, ds, nat.AGG_MEAN), want)
    finally:
        ds.free()
        f.free()


# ------------------------------------------------------------------ 3. the label classes
N3, L3, DEPTH3 = 4096, 3, 6


def _label_set(name, y):
    rng = np.random.default_rng(20261020)
    n = N3
    if name in ("dyadic_shift40", "smax41"):
        out = np.ldexp(rng.integers(-2000, 2001, size=n).astype(np.float64), -40)
        out[:2] = np.ldexp([-2000.0, 2000.0], -40)
        if name == "smax41":
            out[1234] = np.ldexp(3.0, -41)
        return out
    if name in ("int_below_2p23", "int_with_2p23"):
        out = rng.integers(0, 8388608, size=n).astype(np.float64)
        out[:2] = [0.0, 8388607.0]
        if name == "int_with_2p23":
            out[1234] = 8388608.0
        return out
    if name == "negative_ints":
        out = -rng.integers(0, 8388608, size=n).astype(np.float64)
        out[:2] = [-8388607.0, 0.0]
        return out
    if name == "all_negative_nondyadic":
        return -(y[:n] + 1.0) * np.pi
    if name == "signed_zeros":
        return np.where(rng.random(n) < 0.5, 0.0, -0.0)
    if name == "zeros":
        return np.zeros(n)
    if name == "one_nonzero":
        out = np.zeros(n)
        out[1234] = 0.3
        return out
    if name == "constant":
        return np.full(n, 2.5)
    if name == "constant_nondyadic":
        return np.full(n, 0.1)
    if name == "smallest_subnormals":
        return rng.choice([0.0, 5e-324, -5e-324], size=n)
    raise KeyError(name)


LABEL_SETS = ["dyadic_shift40", "smax41", "int_below_2p23", "int_with_2p23", "negative_ints",
              "all_negative_nondyadic", "signed_zeros", "zeros", "one_nonzero", "constant",
              "constant_nondyadic", "smallest_subnormals"]
# dyadic with exact sums: the integer engine and the fp64 engine must give the same bytes
EXACT_SETS = ("dyadic_shift40", "signed_zeros", "zeros", "constant")


@pytest.fixture(scope="module")
def small(cpusmall):
    X, y = cpusmall
    return np.ascontiguousarray(X[:N3]), y


@pytest.mark.parametrize("name", LABEL_SETS)
def test_label_class_boundaries_host_analysis(ctx, small, name):
    """analyze_labels through from_numpy, and again through set_labels on a dataset that held
    ordinary labels (every statistic of the old column must be replaced): the oracle's
    forest both ways; on dyadic labels with exact sums also SBAG_F64=1's bytes."""
    X, y = small
    lab = _label_set(name, y)
    assert lab.shape == (N3,)
    orf = _oracle(X, lab, None, L3, DEPTH3)
    with _env():
        fresh = _fit(ctx, X, lab, None, L3, DEPTH3)
    _check(ctx, fresh, orf, X)
    ds = nat.DeviceDataset.from_numpy(X, y[:N3] * np.pi, ctx)
    try:
        with _env():
            nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=1,
                    max_depth=2, max_bins=BINS, impurity=nat.IMPURITY_VARIANCE).free()
            ds.set_labels(lab)
            again = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0,
                            learner_end=L3, max_depth=DEPTH3, max_bins=BINS, impurity=nat.IMPURITY_VARIANCE)
    finally:
        ds.free()
    assert _forest_bytes(again) == _forest_bytes(fresh)
    if name in EXACT_SETS:
        with _env(SBAG_F64="1"):
            forced = _fit(ctx, X, lab, None, L3, DEPTH3)
        assert _forest_bytes(forced) == _forest_bytes(fresh)


@pytest.mark.parametrize("name", LABEL_SETS)
def test_label_class_boundaries_device_analysis(ctx, small, name):
    """The same label sets as a booster's residuals: k_label_stats and k_label_image, the
    device copy of the analysis, must make the host's call at every boundary."""
    X, y = small
    lab = _label_set(name, y)
    counts, _ = _bags(X, None, 1)
    sub = np.arange(X.shape[1], dtype=np.int32)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(N3), ctx)
    try:
        with _env():
            fb = nat.fit_booster(ctx, ds, lab, counts[0], sub, max_depth=DEPTH3, max_bins=BINS)
    finally:
        ds.free()
    orf = oracle.fit(X, lab, counts[:1], [sub], max_depth=DEPTH3, max_bins=BINS)
    assert_tree_equal(fb, 0, orf, 0)
