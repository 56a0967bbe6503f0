"""CPU: the NumPy reference of the weighted-sum tests (weighted_ref.py) against the oracle's
restatements of the four boosted models' predictions, bit for bit, on oracle fits of the
golden fixtures; and the SBAG_EINVAL cases of sbag_predict_weighted that need no device (the
null arguments: everything else is checked behind a context, which needs one)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import boosting_ref as br
import oracle
import weighted_ref as wr
from conftest import DATA

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat


def _dense(X):
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X, np.float64)


@pytest.fixture(scope="module")
def cpusmall():
    X, y = sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))
    return _dense(X)[:1500], np.asarray(y, np.float64)[:1500]


@pytest.fixture(scope="module")
def vehicle():
    X, y = sb.load_libsvm(os.path.join(DATA, "vehicle.svm"))
    return _dense(X), np.asarray(y, np.float64)


def test_dot_one_column_is_gbm_regression_predict(cpusmall):
    X, y = cpusmall
    w, subs, trees, const = oracle.gbm_regressor_fit(X, y, num_base_learners=6, learning_rate=0.3,
                                                     replacement=True, subspace_ratio=0.7, max_depth=3)
    assert len(w) == 6 and len({tuple(s) for s in subs}) > 1
    got = wr.dot_forest([t[0] for t in trees], subs, X, w, 1)
    assert got.shape == (len(y), 1)
    np.testing.assert_array_equal(got[:, 0] + const, oracle.gbm_predict(w, subs, trees, const, X))


def test_dot_class_columns_is_gbm_classifier_raw(vehicle):
    X, y = vehicle
    K, w, subs, trees = oracle.gbm_classifier_fit(X, y, num_base_learners=3, learning_rate=0.5,
                                                  subspace_ratio=0.7, max_depth=3)
    assert K == 5 and len(trees) == 3
    flat = [ts[k][0] for ts in trees for k in range(K)]          # iteration-major: tree m * K + k
    fsub = [s for s, ts in zip(subs, trees) for _ in range(K)]
    res = wr.dot_forest(flat, fsub, X, [x for ws in w for x in ws], K)
    prob, votes = oracle.gbm_classifier_predict(K, w, subs, trees, X)
    e = np.exp(res)
    tot = np.zeros(len(y))
    for k in range(K):
        tot = tot + e[:, k]
    np.testing.assert_array_equal(e / tot[:, None], prob)
    np.testing.assert_array_equal(np.argmax(e / tot[:, None], axis=1).astype(np.float64), votes)


def test_dot_one_column_is_boosting_regression_predict(cpusmall):
    X, y = cpusmall
    weights, trees, K, _ = br.boosting_fit(X, y, classification=False, num_base_learners=3, max_depth=3)
    assert K is None and len(trees) == 3
    sub = np.arange(X.shape[1])
    acc = wr.dot_forest([t[0] for t in trees], [sub] * len(trees), X, weights, 1)[:, 0]
    wsum = 0.0
    for x in weights:
        wsum = wsum + x
    np.testing.assert_array_equal(acc / wsum, br.boosting_predict(weights, trees, X)[0])


def test_class_weights_is_boosting_classifier_raw(vehicle):
    X, y = vehicle
    weights, trees, K, _ = br.boosting_fit(X, y, classification=True, num_base_learners=4, max_depth=3)
    assert K == 5 and len(trees) == 4
    sub = np.arange(X.shape[1])
    raw = wr.cls_forest([t[0] for t in trees], [sub] * len(trees), X, weights, K)
    want, want_raw = br.boosting_predict(weights, trees, X, K)
    np.testing.assert_array_equal(raw, want_raw)
    np.testing.assert_array_equal(np.argmax(raw, axis=1).astype(np.float64), want)
    assert not raw[:, 0].any() and not np.signbit(raw[:, 0]).any()  # class 0 is empty: +0.0
    wide = wr.cls_forest([t[0] for t in trees], [sub] * len(trees), X, weights, K + 3)
    np.testing.assert_array_equal(wide[:, :K], raw)
    assert not wide[:, K:].any()


def test_rules_are_ordered_and_round_the_product():
    pt = np.array([[1.0], [1.0], [1.0], [1.0]])
    assert wr.dot(pt, [1e16, 1.0, -1e16, 1.0])[0, 0] == 1.0             # not the exact sum 2.0
    assert wr.dot(pt, [1e16, 1.0, -1e16, 1.0], 2)[0].tolist() == [0.0, 2.0]
    assert wr.cls(np.zeros((4, 1)), [1e16, 1.0, -1e16, 1.0], 2)[0].tolist() == [1.0, 0.0]
    # 0.1 * 3.0 rounds up to 0.30000000000000004 before -0.3 meets it: 2^-54, where the exact
    # product added to -0.3 gives 2^-55
    exact = float(Fraction(-0.3) + Fraction(0.1) * 3)
    assert wr.dot(np.array([[-0.3], [0.1]]), [1.0, 3.0])[0, 0] == 2.0 ** -54 != exact
    z = wr.dot(np.array([[-0.0]]), [1.0])
    assert z[0, 0] == 0.0 and not np.signbit(z[0, 0])                   # +0.0 + -0.0 = +0.0


def test_weighted_rejects_null_arguments():
    """Every pointer argument, null in turn (a null context first of all: the others cannot
    be told apart without one, so each is also tried with the rest in place)."""
    lib = nat.lib()
    assert hasattr(lib, "sbag_predict_weighted") and hasattr(lib, "sbag_predict_weighted_dataset")
    f = nat.NativeForest.from_trees([wr.stump(0.5, 1.0, 2.0)], [[0]], nat.IMPURITY_VARIANCE)
    try:
        X = np.zeros((3, 1))
        w = np.ones(1)
        out = np.full((3, 1), 7.0)
        args = [None, f.handle, nat.ptr(X), 3, 1, nat.W_DOT, nat.ptr(w), 1, 1, nat.ptr(out)]
        for null in (None, 1, 2, 6, 9):
            a = list(args)
            if null is not None:
                a[null] = None
            assert lib.sbag_predict_weighted(*a) == nat.SBAG_EINVAL
        dargs = [None, f.handle, None, nat.W_DOT, nat.ptr(w), 1, 1, nat.ptr(out)]
        for null in (None, 1, 4, 7):
            a = list(dargs)
            if null is not None:
                a[null] = None
            assert lib.sbag_predict_weighted_dataset(*a) == nat.SBAG_EINVAL
        assert (out == 7.0).all()  # nothing written
    finally:
        f.free()
    assert (nat.W_DOT, nat.W_CLASS) == (0, 1)
