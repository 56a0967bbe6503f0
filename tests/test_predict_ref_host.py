"""CPU: the NumPy reference walk of the hand-built-forest transform tests (predict_ref.py)
against oracle.predict, bit for bit, on oracle-fitted forests of the golden fixtures --
cpusmall regression and vehicle classification -- over the NaN / +-0 / +-inf doctored
matrix of test_transform_batches_nan_and_signed_zero (no GPU)."""
import os

import numpy as np
import pytest

import oracle
import predict_ref as ref
from conftest import DATA, GOLDEN

import spark_bagging_amd as sb


def _doctored(X):
    Z = X.copy()
    rng = np.random.default_rng(3)
    Z[rng.random(Z.shape) < 0.05] = np.nan
    Z[rng.random(Z.shape) < 0.05] = -0.0
    Z[rng.random(Z.shape) < 0.01] = np.inf
    Z[rng.random(Z.shape) < 0.01] = -np.inf
    return Z


@pytest.mark.parametrize("name,data", [("cpusmall_c1", "cpusmall.svm"), ("vehicle_c2", "vehicle.svm")])
def test_reference_walk_equals_oracle_predict(name, data):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    X, y = sb.load_libsvm(os.path.join(DATA, data))
    L, repl, ratio, seed, depth, bins, cls = g["params"]
    L, depth, bins, seed, cls = int(L), int(depth), int(bins), int(seed), bool(cls)
    counts = oracle.bag(bool(repl), ratio, 0, L, seed, list(g["partitions"]), X.shape[0])
    subs = [s[s >= 0] for s in g["subspaces"]]
    f = oracle.fit(X, y, counts, subs, max_depth=depth, max_bins=bins, classification=cls)
    trees = [f.tree(t)[0] for t in range(L)]
    assert any(len(t) > 3 for t in trees)
    for Z in (X, _doctored(X)):
        want, want_pt = oracle.predict(f, Z, classification=cls, per_tree=True)
        pt = ref.per_tree(trees, subs, Z)
        np.testing.assert_array_equal(pt, want_pt)
        np.testing.assert_array_equal(ref.mode(pt) if cls else ref.mean(pt), want)
    # the doctored cells move rows: the check above is not the clean matrix's twice
    assert (ref.per_tree(trees, subs, _doctored(X)) != ref.per_tree(trees, subs, X)).any()


def test_reference_walk_special_values():
    """One stump at threshold 0.0: -0.0 and 0.0 go left, NaN and +inf right, -inf left."""
    n = np.zeros(3, oracle.NODE_DTYPE)
    n["id"] = np.arange(3)
    n["left"] = n["right"] = n["feature"] = -1
    n[0]["left"], n[0]["right"], n[0]["feature"], n[0]["threshold"] = 1, 2, 0, 0.0
    n[1]["prediction"], n[2]["prediction"] = 10.0, 20.0
    X = np.array([[-0.0], [0.0], [np.nan], [np.inf], [-np.inf], [5e-324], [-5e-324]])
    np.testing.assert_array_equal(ref.per_tree([n], [[0]], X)[0], [10, 10, 20, 20, 10, 20, 10])


def test_reference_aggregations_are_ordered():
    pt = np.array([[1e16], [1.0], [-1e16], [1.0]])
    assert ref.seq_sum(pt)[0] == 1.0 and ref.mean(pt)[0] == 0.25  # not the exact sum 2.0
    votes = np.array([[5, 2, 1], [0, 1, 2], [0, 1, 2], [5, 2, 1], [5, 2, 1], [0, 1, 2], [0, 1, 2]],
                     np.float64)
    np.testing.assert_array_equal(ref.mode(votes), [0, 1, 2])  # 4 votes beat the first to 3
    np.testing.assert_array_equal(ref.mode(votes[:4]), [0, 1, 2])  # 2 : 2, first to reach 2
    np.testing.assert_array_equal(ref.mode(votes[[0, 3, 1, 2]]), [5, 2, 1])
