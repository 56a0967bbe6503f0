"""Host: the oracle across the range of label magnitudes (no GPU).

The fp64 engine's GPU tests (test_gpu_f64_label_range.py) compare with the oracle where the
oracle is the only specification there is: labels y pi 2^k so small that Spark's y*y and its
sums underflow gradually.  So the oracle is first held to an independent restatement
(variance_ref.py: Python floats, one operation at a time), and the facts those GPU tests
rest on are recorded: the oracle's trees are scale-invariant over the ordinary range, and
inside the underflow window they are not -- every tree differs from the rescaled k = 0 tree,
which is what gives the window cases their teeth.

Configuration: cpusmall (8192 x 12), 6 learners, depth 9, maxBins 32, the regressor's default
seed, ratio 1.0 with replacement, one partition."""
import os

import numpy as np
import pytest

import oracle
import variance_ref
from conftest import DATA

import spark_bagging_amd as sb

SEED = oracle.DEFAULT_SEED_REGRESSOR
L, DEPTH, BINS = 6, 9, 32


@pytest.fixture(scope="module")
def base():
    X, y = sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))
    N, F = X.shape
    counts = oracle.bag(True, 1.0, 0, L, SEED, [0, N], N)
    subs = [oracle.subspace(1.0, F, SEED + i) for i in range(L)]
    cache = {}

    def forest(k):
        if k not in cache:
            cache[k] = oracle.fit(X, np.ldexp(y * np.pi, k), counts, subs, max_depth=DEPTH, max_bins=BINS)
        return cache[k]

    return X, y, counts, subs, forest


def _same_structure(fa, fb, t):
    a, b = fa.tree(t)[0], fb.tree(t)[0]
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in ("feature", "split_bin", "left", "right"))


@pytest.mark.parametrize("k", [0, -505, -520, -530, -540, -1040])
def test_oracle_root_equals_python_floats(base, k):
    """Tree 0's root from the C oracle against the Python-float restatement: feature, split
    bin, gain, impurity and prediction bit for bit -- also where y*y is subnormal (-520 ...
    -540) and where every label is subnormal (-1040: y*y is 0, the root a leaf)."""
    X, y, counts, subs, forest = base
    yk = np.ldexp(y * np.pi, k)
    want = variance_ref.root(X, yk, counts[0], subs[0], BINS)
    got = forest(k).tree(0)[0][0]
    for f in ("feature", "split_bin"):
        assert int(got[f]) == want[f], (k, f, got[f], want[f])
    for f in ("gain", "impurity", "prediction"):
        assert float(got[f]).hex() == float(want[f]).hex(), (k, f, float(got[f]), want[f])
    if k == -1040:
        assert want["feature"] == -1 and float(np.abs(yk).max()) < 2.0 ** -1022
    else:
        assert want["feature"] >= 0


@pytest.mark.parametrize("k", [-505, -100, 100, 480])
def test_oracle_forest_is_scale_invariant_in_the_ordinary_range(base, k):
    """No operation under- or overflows: the forest is the k = 0 forest, prediction 2^k."""
    *_, forest = base
    f0, fk = forest(0), forest(k)
    for t in range(L):
        assert _same_structure(f0, fk, t), f"tree {t}"
        a, b = f0.tree(t)[0], fk.tree(t)[0]
        assert np.array_equal(np.ldexp(a["prediction"], k), b["prediction"]), f"tree {t}"
        assert np.array_equal(a["threshold"], b["threshold"]), f"tree {t}"


@pytest.mark.parametrize("k,least", [(-515, 1), (-520, L), (-530, L)])
def test_oracle_trees_differ_inside_the_underflow_window(base, k, least):
    """Gradual underflow of y*y changes Spark's choice: at -520 and -530 every tree's
    structure differs from the k = 0 tree's (measured 6 of 6), at -515 at least one (measured
    2).  A screen that decides at these scales as it does at k = 0 returns other trees."""
    *_, forest = base
    f0, fk = forest(0), forest(k)
    differ = sum(not _same_structure(f0, fk, t) for t in range(L))
    print(f"k = {k}: {differ} of {L} trees differ in structure from k = 0")
    assert differ >= least
    if k != -515:
        assert all(len(fk.tree(t)[0]) > 100 for t in range(L))  # full-size trees, not stumps
