"""CPU: the host side of the Boosting estimators (spark_bagging_amd/boosting.py): the scalar
recursion of ml/boosting/BoostingParams.scala on hand-computed cases, the partition-ordered
SQL sum, param validation and the Spark-format persistence of hand-built models."""
import json
import math
import os
import warnings

import numpy as np
import pytest

import boosting_ref as br

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd import boosting as bo

DOUBLE_MAX = np.finfo(np.float64).max
FIELDS = ("id", "left", "right", "feature", "threshold", "prediction", "impurity", "gain")


def same_nodes(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def test_beta_and_weight():
    assert bo.beta(0.25) == 0.25 / 0.75                      # regressor: numClasses 2
    assert bo.beta(0.25, 4) == 0.25 / (0.75 * 3)             # SAMME: (1 - avgl) * (K - 1)
    assert bo.beta(0.0, 4) == 0.0
    assert bo.weight(0.0) == 1.0                             # beta == 0: not log(1 / 0)
    assert bo.weight(0.5) == math.log(2.0)
    assert bo.weight(1.0) == 0.0
    assert bo.weight(4.0) == math.log(0.25) < 0
    assert bo.beta(1.0) == math.inf and bo.weight(math.inf) == -math.inf  # avgl == 1, as the JVM


def test_terminate():
    # avgl > (K - 1) / K: stop and drop this booster, whatever the validation says
    assert bo.terminate(0.51, False, DOUBLE_MAX, DOUBLE_MAX, 1e-3, 5, 0, 7) == (0, 0.0, 1)
    assert bo.terminate(0.76, True, 3.0, 1.0, 1e-3, 5, 2, 7, 4.0) == (0, 0.0, 1)
    assert bo.terminate(0.75, False, 0.0, DOUBLE_MAX, 1e-3, 5, 0, 7, 4.0) == (6, 0.0, 0)  # not >
    assert bo.terminate(0.6, False, 0.0, DOUBLE_MAX, 1e-3, 5, 0, 7, 4.0) == (6, 0.0, 0)
    # avgl == 0: stop and keep it
    assert bo.terminate(0.0, True, 3.0, 9.0, 1e-3, 5, 3, 7) == (0, 0.0, 0)
    # otherwise terminateVal
    assert bo.terminate(0.3, False, 5.0, DOUBLE_MAX, 1e-3, 5, 2, 7) == (6, 0.0, 0)


def test_terminate_val():
    assert bo.terminate_val(True, DOUBLE_MAX, 10.0, 1e-3, 5, 0, 7) == (6, 10.0, 0)   # improved
    assert bo.terminate_val(True, 10.0, 9.9, 1e-3, 5, 3, 7) == (6, 9.9, 0)
    assert bo.terminate_val(True, 10.0, 9.995, 1e-3, 5, 1, 7) == (6, 10.0, 2)        # within tol
    assert bo.terminate_val(True, 10.0, 11.0, 1e-3, 5, 4, 7) == (0, 0.0, 5)          # numRound - 1
    assert bo.terminate_val(True, 10.0, 11.0, 1e-3, 1, 0, 7) == (0, 0.0, 1)
    assert bo.terminate_val(False, 10.0, 1.0, 1e-3, 5, 3, 7) == (6, 0.0, 0)


def test_partition_sum_follows_the_partitions():
    e = 2.0 ** -53
    x = np.array([1.0, e, e, e])
    assert bo.partition_sum(x, [0, 4]) == 1.0                 # ((1 + e) + e) + e: every e is lost
    assert bo.partition_sum(x, [0, 1, 4]) == 1.0 + ((e + e) + e) != 1.0
    assert bo.partition_sum(x, [0, 0, 2, 2, 4]) == (1.0 + e) + (e + e) == 1.0 + 2.0 ** -52
    assert bo.partition_sum(x[::-1], [0, 4]) == ((e + e) + e) + 1.0
    assert bo.partition_sum(np.zeros(0), [0, 0]) == 0.0
    for part in ([0, 4], [0, 1, 4], [0, 0, 2, 2, 4]):
        assert bo.partition_sum(x, part) == br.partition_sum(x, part)


def test_loss_functions():
    e = np.array([0.0, 0.5, 1.0])
    assert np.array_equal(bo.loss_function("exponential")(e), 1.0 - np.exp(-e))
    assert np.array_equal(bo.loss_function("squared")(e), [0.0, 0.25, 1.0])
    assert np.array_equal(bo.loss_function("absolute")(e), e)
    with pytest.raises(RuntimeError):
        bo.loss_function("huber")


def test_defaults_and_validators():
    c, r = sb.BoostingClassifier(), sb.BoostingRegressor()
    assert c.getSeed() == sb.java_string_hash("org.apache.spark.ml.classification.BoostingClassifier")
    assert r.getSeed() == sb.java_string_hash("org.apache.spark.ml.regression.BoostingRegressor")
    assert c.getSeed() == br.DEFAULT_SEED_BOOSTING_CLASSIFIER
    assert r.getSeed() == br.DEFAULT_SEED_BOOSTING_REGRESSOR
    for est in (c, r):
        assert (est.getNumBaseLearners(), est.getTol(), est.getNumRound(), est.getLoss()) == \
            (10, 1e-3, 5, "exponential")
        for name, bad in (("numBaseLearners", 0), ("tol", -1e-9), ("numRound", 0), ("loss", "huber")):
            with pytest.raises(sb.IllegalArgumentException):
                est.set(name, bad)
    for loss in ("squared", "absolute", "Exponential"):
        assert r.copy().setLoss(loss).getLoss() == loss.lower()
        if loss != "Exponential":
            with pytest.raises(sb.IllegalArgumentException):
                c.copy().setLoss(loss)
    with pytest.raises(sb.IllegalArgumentException):
        c.setBaseLearner(sb.DecisionTreeRegressor())
    with pytest.raises(sb.IllegalArgumentException):
        r.setBaseLearner(sb.DecisionTreeClassifier())
    with pytest.raises(sb.IllegalArgumentException):
        r.setBaseLearner(sb.BaggingRegressor())
    c.setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(2))
    assert c.copy().getBaseLearner() is not c.getBaseLearner()


def test_classifier_label_validation_needs_no_device():
    X = np.zeros((3, 2))
    for y in ([0.0, 1.5, 1.0], [0.0, -1.0, 1.0]):
        with pytest.raises(sb.IllegalArgumentException):
            sb.BoostingClassifier().fit((X, np.array(y)))
    with pytest.raises(sb.IllegalArgumentException):  # the indicator column has no values
        sb.BoostingRegressor().setValidationIndicatorCol("v").fit((X, np.zeros(3)))


def _leaf(pred):
    n = np.zeros(1, nat.NODE_DTYPE)
    n["left"] = n["right"] = n["feature"] = -1
    n["prediction"], n["gain"] = pred, -1.0  # (a leaf's gain, as the tree writer stores it)
    return n


def _stump(thr, lo, hi, feature=1):
    n = np.zeros(3, nat.NODE_DTYPE)
    n["id"] = np.arange(3)
    n["left"] = n["right"] = n["feature"] = -1
    n[0]["left"], n[0]["right"], n[0]["feature"], n[0]["threshold"] = 1, 2, feature, thr
    n[1]["prediction"], n[2]["prediction"] = lo, hi
    n[1]["gain"] = n[2]["gain"] = -1.0
    return n


def test_regression_model_round_trip(tmp_path):
    trees = [_stump(0.5, -1.25, 3.0), _leaf(7.0)]
    models = [sb.DecisionTreeModel(t, np.zeros((len(t), 3)), nat.IMPURITY_VARIANCE) for t in trees]
    m = sb.BoostingRegressionModel([0.1, 1.7976931348623157e308], models, num_features=3)
    m.set("loss", "squared").set("numBaseLearners", 2).set("seed", -5)
    path = str(tmp_path / "reg")
    m.save(path)
    with pytest.raises(sb.IllegalArgumentException):
        m.save(path)
    meta = json.loads(open(os.path.join(path, "metadata", "part-00000")).read())
    assert meta["class"] == "org.apache.spark.ml.regression.BoostingRegressionModel"
    assert meta["numBaseModels"] == 2 and "numClasses" not in meta
    assert meta["paramMap"]["loss"] == "squared" and "baseLearner" not in meta["paramMap"]
    assert sorted(d for d in os.listdir(path) if not d.startswith(".")) == \
        ["data-0", "data-1", "learner", "metadata", "model-0", "model-1"]
    back = sb.BoostingRegressionModel.load(path)
    assert back.uid == m.uid and back.weights == m.weights and back.numBaseModels == 2
    assert back.get("loss") == "squared" and back.getSeed() == -5
    assert isinstance(back.getBaseLearner(), sb.DecisionTreeRegressor)
    for a, b in zip(back.models, m.models):
        assert same_nodes(a.nodes, b.nodes) and a.impurity == nat.IMPURITY_VARIANCE
    assert list(back._subspace(back.models[1])) == [0, 1, 2]


def test_classification_model_round_trip(tmp_path):
    trees = [_stump(0.5, 0.0, 2.0), _leaf(1.0)]
    stats = [np.array([[3.0, 0.0, 2.0], [3.0, 0.0, 0.0], [0.0, 0.0, 2.0]]), np.array([[1.0, 4.0]])]
    models = [sb.DecisionTreeModel(t, s, nat.IMPURITY_GINI) for t, s in zip(trees, stats)]
    m = sb.BoostingClassificationModel(3, [1.0, math.log(3.0)], models, num_features=2)
    path = str(tmp_path / "cls")
    m.save(path)
    meta = json.loads(open(os.path.join(path, "metadata", "part-00000")).read())
    assert meta["class"] == "org.apache.spark.ml.classification.BoostingClassificationModel"
    assert meta["numClasses"] == 3 and meta["numBaseModels"] == 2
    back = sb.BoostingClassificationModel.load(path)
    assert back.numClasses == 3 and back.weights == m.weights
    assert isinstance(back.getBaseLearner(), sb.DecisionTreeClassifier)
    for a, b in zip(back.models, m.models):
        assert same_nodes(a.nodes, b.nodes) and np.array_equal(a.stats, b.stats)
        assert a.impurity == nat.IMPURITY_GINI
    with pytest.raises(sb.IllegalArgumentException):  # another model class's directory
        sb.BoostingRegressionModel.load(path)


def test_estimator_round_trip_and_weight_col_warning(tmp_path):
    est = sb.BoostingRegressor().setLoss("absolute").setNumRound(3).setTol(0.01).setBaseLearner(
        sb.DecisionTreeRegressor().setMaxDepth(7))
    est.save(str(tmp_path / "e"))
    back = sb.BoostingRegressor.load(str(tmp_path / "e"))
    assert (back.getLoss(), back.getNumRound(), back.getTol()) == ("absolute", 3, 0.01)
    assert back.getBaseLearner().getMaxDepth() == 7
    with pytest.raises(sb.IllegalArgumentException):
        sb.BoostingClassifier.load(str(tmp_path / "e"))
    # weightCol warns and is ignored, as in the reference (the fit then fails on the empty
    # training set, before any device work)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(sb.SparkException):
            est.copy().setWeightCol("w").fit((np.zeros((0, 2)), np.zeros(0)))
    assert any("weightCol is ignored" in str(x.message) for x in w)


def test_reference_helpers():
    assert br.wrap64(2**63) == -2**63 and br.wrap64(-2**63 - 1) == 2**63 - 1
    m = np.array([0.0, 1e-12, 1.0, 1.0])
    assert list(br.doubles_drawn(m, [0, 1, 0, 3])) == [0, 1, 1, 4]
    bag = br.boosted_bag(np.array([0.0, 1.0, 1.0]), [0, 1, 3], 5)
    assert bag[0] == 0
    import oracle
    assert bag[1] == oracle.poisson(1.0, 5 + 1 + 0, 1)[0] and bag[2] == oracle.poisson(1.0, 5 + 1 + 1, 1)[0]
