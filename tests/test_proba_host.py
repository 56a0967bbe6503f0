"""CPU: the raw-prediction entry points exist (header, library, bindings) and reject null
arguments; sbag_forest_create_stats keeps and validates the stats on the host; proba_ref is
held to the oracle's per-tree predictions and leaf stats; the normalisation and log-loss
formulas on hand-made arrays."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import oracle
import proba_ref
from parity_utils import oracle_forest

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_log_loss, raw_to_probability

NAMES = ["sbag_forest_num_classes", "sbag_forest_create_stats", "sbag_predict_raw",
         "sbag_predict_raw_dataset", "sbag_predict_oob_raw"]


def test_header_library_and_bindings_name_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "sbag.h")).read()
    for name in NAMES:
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", txt, re.M), name
        assert hasattr(nat.lib(), name), name
        assert name in nat.EXPORTED, name
    assert re.search(r"#define\s+SBAG_RAW_VOTES\s+0\b", txt) and re.search(r"#define\s+SBAG_RAW_LEAF\s+1\b", txt)
    assert (nat.RAW_VOTES, nat.RAW_LEAF) == (0, 1)
    assert sb.raw_to_probability is raw_to_probability and sb.oob_log_loss is oob_log_loss


def test_null_arguments_are_einval():
    lib = nat.lib()
    n = ctypes.c_int32()
    assert lib.sbag_forest_num_classes(None, ctypes.byref(n)) == nat.SBAG_EINVAL
    assert lib.sbag_forest_create_stats(1, None, None, None, None, nat.IMPURITY_GINI, None, None, None) == nat.SBAG_EINVAL
    assert lib.sbag_predict_raw(None, None, None, 1, 1, nat.RAW_VOTES, 2, None) == nat.SBAG_EINVAL
    assert lib.sbag_predict_raw_dataset(None, None, None, nat.RAW_VOTES, 2, None) == nat.SBAG_EINVAL
    assert lib.sbag_predict_oob_raw(None, None, None, None, None, 1, nat.RAW_LEAF, 2, None, None) == nat.SBAG_EINVAL
    assert len(lib.sbag_last_error()) > 0


# ---------------------------------------------------------------- sbag_forest_create_stats
def _stump(pred_left, pred_right):
    t = np.zeros(3, nat.NODE_DTYPE)
    t["id"] = [0, 1, 2]
    t["left"] = [1, -1, -1]
    t["right"] = [2, -1, -1]
    t["feature"] = [0, -1, -1]
    t["threshold"] = [0.5, 0.0, 0.0]
    t["prediction"] = [pred_left, pred_left, pred_right]
    return t


def test_create_stats_round_trips_the_stats_and_counts_classes():
    trees = [_stump(0.0, 2.0), _stump(1.0, 0.0)]
    stats = [np.array([[3.0, 1.0, 4.0], [3.0, 0.5, 0.0], [0.0, 0.5, 4.0]]),
             np.array([[2.0, 7.0, 0.0, 0.0, 1.0], [0.0, 7.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0, 1.0]])]
    f = nat.NativeForest.from_trees(trees, [[0], [1]], nat.IMPURITY_GINI, stats=stats)
    assert len(f) == 2
    assert f.num_classes == 5  # max num_stats (5) beats the largest leaf prediction + 1 (3)
    for t in range(2):
        nodes, st = f.tree(t)
        np.testing.assert_array_equal(nodes["prediction"], trees[t]["prediction"])
        assert st.shape == stats[t].shape
        np.testing.assert_array_equal(st, stats[t])
    f.free()
    # fewer stats than the leaf predictions name: the existing rule wins
    g = nat.NativeForest.from_trees([_stump(0.0, 6.0)], [[0]], nat.IMPURITY_GINI,
                                    stats=[np.ones((3, 2))])
    assert g.num_classes == 7
    g.free()
    # sbag_forest_create keeps its behaviour: no stats, the class count of the predictions
    h = nat.NativeForest.from_trees(trees, [[0], [1]], nat.IMPURITY_GINI)
    assert h.num_classes == 3 and h.tree(0)[1].shape == (3, 0)
    h.free()
    v = nat.NativeForest.from_trees([_stump(0.25, 1.5)], [[0]], nat.IMPURITY_VARIANCE,
                                    stats=[np.ones((3, 3))])
    assert v.num_classes == 0
    np.testing.assert_array_equal(v.tree(0)[1], np.ones((3, 3)))
    v.free()


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_create_stats_rejects_negative_and_non_finite_stats(bad):
    st = np.array([[3.0, 1.0], [3.0, 0.0], [0.0, 1.0]])
    st[2, 0] = bad
    with pytest.raises(sb.IllegalArgumentException):
        nat.NativeForest.from_trees([_stump(0.0, 1.0)], [[0]], nat.IMPURITY_GINI, stats=[st])


def test_create_stats_rejects_what_create_rejects_and_a_negative_num_stats():
    lib = nat.lib()
    t = _stump(0.0, 1.0)
    nn, sl, subs = np.array([3], np.int32), np.array([1], np.int32), np.array([0], np.int32)
    st = np.ones(6)
    h = ctypes.c_void_p()

    def create(nodes, ns):
        return lib.sbag_forest_create_stats(1, nat.ptr(nn), nat.ptr(nodes), nat.ptr(sl), nat.ptr(subs),
                                            nat.IMPURITY_GINI, nat.ptr(np.array([ns], np.int32)), nat.ptr(st),
                                            ctypes.byref(h))

    assert create(t, -1) == nat.SBAG_EINVAL
    loop = t.copy()
    loop["left"][0] = 0  # a child link that does not advance
    assert create(loop, 2) == nat.SBAG_EINVAL
    noclass = t.copy()
    noclass["prediction"][2] = 0.5
    assert create(noclass, 2) == nat.SBAG_EINVAL
    assert create(t, 2) == nat.SBAG_OK
    lib.sbag_forest_free(h)


# ---------------------------------------------------------------- proba_ref against the oracle
@pytest.fixture(scope="module")
def vehicle():
    X, y = sb.load_libsvm(os.path.join(ROOT, "tests", "golden", "data", "vehicle.svm"))
    seed, L, N = oracle.DEFAULT_SEED_CLASSIFIER, 8, len(y)
    part = [0, 300, 300, N]
    counts = oracle.bag(True, 0.7, 0, L, seed, part, N)
    subs = [oracle.subspace(0.7, X.shape[1], seed + i) for i in range(L)]
    orf = oracle_forest(X, y, counts, subs, 5, 32, True, part=part)
    trees = [orf.tree(t)[0] for t in range(L)]
    stats = [orf.tree(t)[1] for t in range(L)]
    return X, y, counts, orf, trees, stats


def test_votes_equal_the_bincount_of_the_oracles_per_tree_predictions(vehicle):
    X, y, counts, orf, trees, stats = vehicle
    _, per_tree = oracle.predict(orf, X, True, per_tree=True)
    C = int(per_tree.max()) + 1
    want = np.stack([np.bincount(per_tree[:, r].astype(np.int64), minlength=C) for r in range(len(y))])
    got = proba_ref.raw(trees, stats, orf.subspaces, X, proba_ref.VOTES, C)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want.astype(np.float64))
    # masked: the out-of-bag trees only
    got_oob, n_oob = proba_ref.raw(trees, stats, orf.subspaces, X, proba_ref.VOTES, C, counts=counts)
    want_oob = np.zeros_like(got)
    for r in range(len(y)):
        for i in range(len(trees)):
            if counts[i][r] == 0:
                want_oob[r, int(per_tree[i, r])] += 1.0
    np.testing.assert_array_equal(got_oob, want_oob)
    np.testing.assert_array_equal(n_oob, (counts == 0).sum(axis=0))
    np.testing.assert_array_equal(got_oob.sum(axis=1), n_oob)


def test_leaf_of_a_single_tree_is_the_leafs_stats_over_their_sum(vehicle):
    X, y, counts, orf, trees, stats = vehicle
    import predict_ref
    C = max(s.shape[1] for s in stats)
    for t in (0, 3):
        leaf = predict_ref.walk(trees[t], orf.subspaces[t], X)
        st = stats[t][leaf]
        want = np.zeros((len(y), C))
        for r in range(len(y)):
            total = 0.0
            for v in st[r]:
                total = total + v
            want[r, :st.shape[1]] = [v / total for v in st[r]]
        got = proba_ref.raw([trees[t]], [stats[t]], [orf.subspaces[t]], X, proba_ref.LEAF, C)
        np.testing.assert_array_equal(got, want)
        assert np.abs(got.sum(axis=1) - 1.0).max() < 1e-12


def test_leaf_sums_the_trees_in_order_and_skips_empty_leaves():
    X = np.array([[0.0], [1.0]])
    trees = [_stump(0.0, 1.0)] * 3
    stats = [np.array([[2.0, 2.0], [1.0, 2.0], [0.0, 0.0]]),   # right leaf: total 0, contributes nothing
             np.array([[9.0], [7.0], [3.0]]),                   # one class of its own: column 1 unchanged
             np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 6.0], [0.1, 0.2, 0.7]])]
    got = proba_ref.raw(trees, stats, [[0]] * 3, X, proba_ref.LEAF, 4)
    row0 = [((0.0 + 1.0 / 3.0) + 7.0 / 7.0) + 1.0 / 7.0, (0.0 + 2.0 / 3.0) + 0.0 / 7.0, 0.0 + 6.0 / 7.0, 0.0]
    t3 = (0.1 + 0.2) + 0.7
    row1 = [(0.0 + 3.0 / 3.0) + 0.1 / t3, 0.0 + 0.2 / t3, 0.0 + 0.7 / t3, 0.0]
    np.testing.assert_array_equal(got, np.array([row0, row1]))


# ---------------------------------------------------------------- normalisation and log-loss
def test_probability_is_raw_over_its_left_to_right_row_sum():
    raw = np.array([[0.1, 0.2, 0.3, 0.4], [3.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1e-300, 1.0, 1e16, 1.0]])
    p = raw_to_probability(raw)
    for r in range(4):
        s = 0.0
        for v in raw[r]:
            s = s + v
        if s == 0:
            assert np.isnan(p[r]).all()
        else:
            assert p[r].tolist() == [v / s for v in raw[r]]
    with pytest.raises(sb.IllegalArgumentException):
        raw_to_probability(np.zeros(3))


def test_log_loss_over_covered_rows_with_clipping():
    proba = np.array([[0.5, 0.25, 0.25], [np.nan, np.nan, np.nan], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    n_oob = np.array([2, 0, 1, 3, 1], np.int32)
    y = np.array([1.0, 2.0, 0.0, 0.0, 2.0])
    got = oob_log_loss(proba, n_oob, y)
    want = -(math.log(0.25) + math.log(1e-15) + math.log(1 - 1e-15) + math.log(0.5)) / 4
    assert got["metric"] == "logLoss" and got["numRows"] == 5 and got["coverage"] == 4 / 5
    assert got["value"] == pytest.approx(want, rel=1e-12)
    # a label past the columns counts as probability 0
    got = oob_log_loss(proba[:1], n_oob[:1], np.array([7.0]))
    assert got["value"] == pytest.approx(-math.log(1e-15), rel=1e-12)
    none = oob_log_loss(proba, np.zeros(5, np.int32), y)
    assert math.isnan(none["value"]) and none["coverage"] == 0.0 and none["numRows"] == 5
    with pytest.raises(sb.IllegalArgumentException):
        oob_log_loss(proba, n_oob[:3], y)


def test_models_expose_the_probability_methods_and_regression_refuses():
    for name in ("predictRaw", "predictProbability", "oobProbabilities", "oobLogLoss"):
        assert callable(getattr(sb.BaggingClassificationModel, name))
        with pytest.raises(sb.IllegalArgumentException):
            getattr(sb.BaggingRegressionModel([], []), name)(np.zeros((1, 1)))
    assert isinstance(sb.BaggingClassificationModel.numClasses, property)
    with pytest.raises(sb.IllegalArgumentException):
        sb.BaggingClassificationModel([], [])._kind("weighted")
