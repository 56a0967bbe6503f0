"""CPU: the Stacking estimators' params, validators and persistence, the NumPy restatement
(stacking_ref.py) against a 3-tree, 5-row example worked out by hand, and the host arithmetic of
the device calls (sbag_stack_plan.h: ranks, rank cuts, per-tree dictionaries) swept by the
stand-alone program tests/c/stack_plan_check.cpp, plain and under ASan + UBSan."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import stacking_ref as sref
from conftest import ROOT

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat


def _blank(n):
    a = np.zeros(n, nat.NODE_DTYPE)
    a["id"] = np.arange(n)
    a["left"] = a["right"] = a["feature"] = -1
    return a


def leaf(v):
    a = _blank(1)
    a["prediction"] = v
    return a


def stump(thr, lv, rv, feature=0):
    a = _blank(3)
    a["left"][0], a["right"][0], a["feature"][0], a["threshold"][0] = 1, 2, feature, thr
    a["prediction"][1], a["prediction"][2] = lv, rv
    return a


def example():
    """Three base trees over two features, and a stack tree whose subspace permutes them:
    its feature 1 is base tree 0, its feature 2 base tree 1, its feature 0 (never tested) base
    tree 2."""
    X = np.array([[0.0, 1.0], [1.0, -1.0], [2.0, 0.0], [-0.0, 5.0], [3.0, 2.0]])
    trees = [stump(1.0, 10.0, 20.0, feature=0), stump(0.0, -1.5, 2.5, feature=1), leaf(7.0)]
    subs = [np.arange(2, dtype=np.int32)] * 3
    stack = _blank(5)
    stack["left"][0], stack["right"][0], stack["feature"][0], stack["threshold"][0] = 1, 4, 1, 10.0
    stack["left"][1], stack["right"][1], stack["feature"][1], stack["threshold"][1] = 2, 3, 2, -1.5
    stack["prediction"][2], stack["prediction"][3], stack["prediction"][4] = 100.0, 200.0, 300.0
    return X, trees, subs, stack, np.array([2, 0, 1], np.int32)


def test_restatement_against_the_hand_computed_example():
    X, trees, subs, stack, ssub = example()
    # tree 0: x0 <= 1 -> 10 else 20; tree 1: x1 <= 0 -> -1.5 else 2.5; tree 2: always 7
    want_l1 = np.array([[10.0, 2.5, 7.0], [10.0, -1.5, 7.0], [20.0, -1.5, 7.0], [10.0, 2.5, 7.0],
                        [20.0, 2.5, 7.0]])
    np.testing.assert_array_equal(sref.level1(trees, subs, X), want_l1)
    # stack: tree0 <= 10 ? (tree1 <= -1.5 ? 100 : 200) : 300
    np.testing.assert_array_equal(sref.predict(trees, subs, stack, ssub, X),
                                  [200.0, 100.0, 300.0, 200.0, 300.0])
    d, off, cb, S, codes = sref.dataset_layout(want_l1)
    np.testing.assert_array_equal(d, [10.0, 20.0, -1.5, 2.5, 7.0])
    np.testing.assert_array_equal(off, [0, 2, 4, 5])
    assert (cb, S) == (1, 16) and codes.dtype == np.uint8 and codes.shape == (5, 16)
    np.testing.assert_array_equal(codes[:, :3], [[0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    assert not codes[:, 3:].any()


def test_layout_restatement_merges_zeros_and_widens():
    P = np.array([[-0.0, 1.0], [0.0, 2.0]])
    d, off, cb, S, codes = sref.dataset_layout(P)
    np.testing.assert_array_equal(off, [0, 1, 3])
    assert not np.signbit(d[0]) and not codes[:, 0].any()
    wide = np.arange(300, dtype=np.float64)[:, None] * np.ones((1, 17))
    _, _, cb, S, codes = sref.dataset_layout(wide)
    assert (cb, S) == (2, 32) and codes.dtype == np.uint16
    assert sref.row_stride(16) == 16 and sref.row_stride(65) == 128 and sref.row_stride(1) == 16


def test_params_defaults_setters_and_validators():
    est = sb.StackingRegressor()
    assert est.getParallelism() == 1 and est.get("weightCol") is None
    assert (est.get("labelCol"), est.get("featuresCol"), est.get("predictionCol")) == \
        ("label", "features", "prediction")
    a, b = sb.DecisionTreeRegressor().setMaxDepth(2), sb.DecisionTreeRegressor().setMaxBins(8)
    assert est.setBaseLearners([a, b]).setStacker(a).setParallelism(3) is est
    assert est.getBaseLearners() == [a, b] and est.getStacker() is a and est.getParallelism() == 3
    with pytest.raises(sb.IllegalArgumentException):
        est.setParallelism(0)
    cp = est.copy({"parallelism": 2})
    assert cp.getParallelism() == 2 and est.getParallelism() == 3
    assert cp.getBaseLearners()[0] is not a and cp.getBaseLearners()[0].getMaxDepth() == 2


def test_non_tree_learners_are_refused():
    for est, good, bad in ((sb.StackingRegressor(), sb.DecisionTreeRegressor, sb.DecisionTreeClassifier),
                           (sb.StackingClassifier(), sb.DecisionTreeClassifier, sb.DecisionTreeRegressor)):
        for other in (bad(), sb.BaggingRegressor(), object()):
            with pytest.raises(sb.IllegalArgumentException, match="stacking engine fits " + good.__name__):
                est.setBaseLearners([good(), other])
            with pytest.raises(sb.IllegalArgumentException, match="stacking engine fits " + good.__name__):
                est.setStacker(other)


def test_empty_base_learners_are_refused():
    est = sb.StackingRegressor().setStacker(sb.DecisionTreeRegressor())
    with pytest.raises(sb.IllegalArgumentException):
        est.setBaseLearners([])
    with pytest.raises(sb.IllegalArgumentException):  # never set: nothing reaches the device
        est.fit((np.zeros((4, 2)), np.zeros(4)))
    with pytest.raises(sb.IllegalArgumentException):  # no stacker
        sb.StackingRegressor().setBaseLearners([sb.DecisionTreeRegressor()]).fit((np.zeros((4, 2)), np.zeros(4)))


def test_classifier_validates_labels_before_the_device():
    est = sb.StackingClassifier().setBaseLearners([sb.DecisionTreeClassifier()]) \
        .setStacker(sb.DecisionTreeClassifier())
    X = np.zeros((3, 2))
    for y in ([0.0, 1.5, 1.0], [0.0, -1.0, 1.0]):
        with pytest.raises(sb.IllegalArgumentException, match="invalid label|numClasses"):
            est.fit((X, np.array(y)))


def test_estimator_save_load_round_trip(tmp_path):
    learners = [sb.DecisionTreeRegressor().setMaxDepth(d).setMaxBins(b).setSeed(s)
                for d, b, s in ((2, 8, 1), (7, 32, 2), (4, 16, 3))]
    est = sb.StackingRegressor().setBaseLearners(learners) \
        .setStacker(sb.DecisionTreeRegressor().setMaxDepth(3).setMinInstancesPerNode(5)).setParallelism(4)
    path = str(tmp_path / "est")
    est.save(path)
    assert sorted(os.listdir(path)) == ["learner-0", "learner-1", "learner-2", "metadata", "stacker"]
    from spark_bagging_amd import persistence as sp
    meta = sp.load_metadata(path, "org.apache.spark.ml.regression.StackingRegressor")
    assert "baseLearners" not in meta["paramMap"] and "stacker" not in meta["paramMap"]
    assert meta["paramMap"]["parallelism"] == 4
    got = sb.StackingRegressor.load(path)
    assert got.uid == est.uid and got.getParallelism() == 4
    assert [(b.getMaxDepth(), b.getMaxBins(), b.getSeed()) for b in got.getBaseLearners()] == \
        [(2, 8, 1), (7, 32, 2), (4, 16, 3)]  # index order
    assert [b.uid for b in got.getBaseLearners()] == [b.uid for b in learners]
    assert got.getStacker().getMaxDepth() == 3 and got.getStacker().getMinInstancesPerNode() == 5
    with pytest.raises(sb.IllegalArgumentException, match="already exists"):
        est.save(path)
    with pytest.raises(sb.IllegalArgumentException, match="Expected class name"):
        sb.StackingClassifier.load(path)


def same_nodes(a, b):
    inner = a["left"] >= 0  # (Spark's NodeData stores gain -1 at a leaf)
    return all(np.array_equal(a[k], b[k]) for k in ("id", "left", "right", "feature", "threshold",
                                                     "prediction", "impurity")) and \
        np.array_equal(a["gain"][inner], b["gain"][inner])


@pytest.mark.parametrize("classification", [False, True])
def test_model_save_load_round_trip(tmp_path, classification):
    X, trees, subs, stack, ssub = example()
    if classification:
        Model, Learner, imp, ns = sb.StackingClassificationModel, sb.DecisionTreeClassifier, nat.IMPURITY_GINI, 2
        for t in trees + [stack]:
            t["prediction"] = (t["prediction"] > 9).astype(np.float64)
    else:
        Model, Learner, imp, ns = sb.StackingRegressionModel, sb.DecisionTreeRegressor, nat.IMPURITY_VARIANCE, 3
    rng = np.random.default_rng(3)
    models = [sb.DecisionTreeModel(t, rng.integers(0, 9, (len(t), ns)).astype(np.float64), imp) for t in trees]
    # the stack tree of a fitted model tests features in order: take the identity subspace here
    st = sb.DecisionTreeModel(stack, rng.integers(0, 9, (len(stack), ns)).astype(np.float64), imp)
    model = Model(models, st, num_features=2)
    model.setBaseLearners([Learner().setMaxDepth(i + 1) for i in range(3)]).setStacker(Learner().setMaxBins(4))
    model.setParallelism(2)
    path = str(tmp_path / "model")
    model.save(path)
    assert sorted(os.listdir(path)) == ["learner-0", "learner-1", "learner-2", "metadata", "model-0",
                                        "model-1", "model-2", "stack", "stacker"]
    got = Model.load(path)
    assert got.uid == model.uid and got.getParallelism() == 2 and got._num_features == 2
    assert [b.getMaxDepth() for b in got.getBaseLearners()] == [1, 2, 3] and got.getStacker().getMaxBins() == 4
    assert len(got.models) == 3
    for a, b in zip(got.models + [got.stack], models + [st]):
        assert same_nodes(a.nodes, b.nodes) and np.array_equal(a.stats, b.stats) and a.impurity == imp
    from spark_bagging_amd import persistence as sp
    assert sp.load_metadata(os.path.join(path, "stack"))["numFeatures"] == 3
    assert sp.load_metadata(os.path.join(path, "model-1"))["numFeatures"] == 2
    assert sp.load_metadata(os.path.join(path, "model-1"))["class"] == Learner._spark_model_class


def test_weight_col_warns_as_the_other_estimators(monkeypatch):
    est = sb.StackingRegressor().setBaseLearners([sb.DecisionTreeRegressor()]) \
        .setStacker(sb.DecisionTreeRegressor()).setWeightCol("w")

    class Stop(Exception):
        pass

    def no_device(*a, **k):
        raise Stop()

    monkeypatch.setattr(nat, "default_context", no_device)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(Stop):
            est.fit((np.zeros((4, 2)), np.zeros(4)))
    assert any("weightCol is ignored, as it is not supported by DecisionTreeRegressor now." in str(x.message)
               for x in w)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_stack_plan_sweep(tmp_path, flags):
    exe = str(tmp_path / "stack_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "spark-bagging_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "stack_plan_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"stack_plan_check: (\d+) cases, (\d+) compares, 0 failures", p.stdout)
    assert m and int(m.group(1)) == 4000 and int(m.group(2)) > 1_000_000, p.stdout[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
