"""GPU: BoostingClassifier / BoostingRegressor end to end against tests/boosting_ref.py (the
reference's training recursion on the CPU oracle): the booster weights, every tree node by
node, transform and predictRaw.  Host math (exp, pow, log) is numpy's on both sides; the
bag, the trees and the walks come from the device on one side and the oracle on the other.

Squared loss on cpusmall: after the first booster one row carries a Poisson mean far above
40 (119 at depth 2, 230 at depth 4), which PoissonDistribution draws with another algorithm
and the library refuses (sbag.h), so that case boosts once and pins the refusal of the
second iteration.
"""
import os

import numpy as np
import pytest

import boosting_ref as br
from conftest import DATA

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ("id", "left", "right", "feature", "threshold", "prediction", "impurity", "gain")


def _dense(X):
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X, np.float64)


@pytest.fixture(scope="module")
def vehicle():
    X, y = sb.load_libsvm(os.path.join(DATA, "vehicle.svm"))
    return _dense(X), np.asarray(y, np.float64)


@pytest.fixture(scope="module")
def cpusmall():
    X, y = sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))
    return _dense(X)[:2000], np.asarray(y, np.float64)[:2000]


def assert_model_equals_reference(model, ref, X):
    weights, trees, K, _ = ref
    assert model.weights == [float(w) for w in weights]
    assert model.numBaseModels == len(trees)
    for t, (m, (nodes, stats)) in enumerate(zip(model.models, trees)):
        assert len(m.nodes) == len(nodes), f"booster {t}: node count"
        for f in FIELDS:
            assert np.array_equal(m.nodes[f], nodes[f]), f"booster {t}: {f}"
        assert np.array_equal(m.stats, stats), f"booster {t}: stats"
    if not trees:
        return
    want, want_raw = br.boosting_predict(weights, trees, X, K)
    assert np.array_equal(model.transform(X), want)
    if K is not None:
        assert np.array_equal(model.predict_raw(X), want_raw)


def test_classifier_vehicle(vehicle):
    X, y = vehicle
    part = [0, len(y) // 2, len(y)]
    est = sb.BoostingClassifier().setNumBaseLearners(5).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(3))
    model = est.fit(sb.Frame(X, y, partition_offsets=part))
    ref = br.boosting_fit(X, y, classification=True, num_base_learners=5, max_depth=3, part=part)
    assert len(ref[0]) == 5 and model.numClasses == 5  # labels 1..4: max label + 1
    assert_model_equals_reference(model, ref, X)


def test_classifier_vehicle_validation_stops_early(vehicle):
    X, y = vehicle
    part = [0, len(y) // 2, len(y)]
    v = np.random.default_rng(1).random(len(y)) < 0.3
    est = sb.BoostingClassifier().setNumBaseLearners(8).setNumRound(2).setValidationIndicatorCol(
        "val").setBaseLearner(sb.DecisionTreeClassifier().setMaxDepth(3))
    model = est.fit(sb.Frame(X, y, partition_offsets=part), validation=v)
    ref = br.boosting_fit(X, y, classification=True, num_base_learners=8, max_depth=3, part=part,
                          validation=v, num_round=2)
    assert ref[3] < 8 and len(ref[0]) < ref[3], "the reference loop ran to the end"
    assert_model_equals_reference(model, ref, X)


@pytest.mark.parametrize("loss", ["exponential", "absolute"])
def test_regressor_cpusmall(cpusmall, loss):
    X, y = cpusmall
    part = [0, 700, 2000]
    est = sb.BoostingRegressor().setNumBaseLearners(4).setLoss(loss).setBaseLearner(
        sb.DecisionTreeRegressor().setMaxDepth(4))
    model = est.fit(sb.Frame(X, y, partition_offsets=part))
    ref = br.boosting_fit(X, y, classification=False, num_base_learners=4, max_depth=4, loss=loss,
                          part=part)
    assert len(ref[0]) == 4
    assert_model_equals_reference(model, ref, X)


def test_regressor_cpusmall_squared(cpusmall):
    X, y = cpusmall
    part = [0, 700, 2000]
    bl = sb.DecisionTreeRegressor().setMaxDepth(4)
    est = sb.BoostingRegressor().setNumBaseLearners(1).setLoss("squared").setBaseLearner(bl)
    model = est.fit(sb.Frame(X, y, partition_offsets=part))
    ref = br.boosting_fit(X, y, classification=False, num_base_learners=1, max_depth=4,
                          loss="squared", part=part)
    assert_model_equals_reference(model, ref, X)
    with pytest.raises(sb.SparkException) as e:  # the second bag has a mean of 230
        est.copy({"numBaseLearners": 2}).fit(sb.Frame(X, y, partition_offsets=part))
    assert e.value.code == nat.SBAG_EUNSUPPORTED


def test_regressor_validation_stops_early(cpusmall):
    X, y = cpusmall
    part = [0, 700, 2000]
    v = np.random.default_rng(2).random(2000) < 0.25
    est = sb.BoostingRegressor().setNumBaseLearners(8).setNumRound(2).setValidationIndicatorCol(
        "val").setBaseLearner(sb.DecisionTreeRegressor().setMaxDepth(4))
    model = est.fit(sb.Frame(X, y, partition_offsets=part), validation=v)
    ref = br.boosting_fit(X, y, classification=False, num_base_learners=8, max_depth=4, part=part,
                          validation=v, num_round=2)
    assert ref[3] < 8 and len(ref[0]) < ref[3], "the reference loop ran to the end"
    assert_model_equals_reference(model, ref, X)


def test_separable_set_stops_on_zero_loss_and_keeps_the_booster():
    X = np.arange(40, dtype=np.float64)[:, None] - 19.5
    y = (X[:, 0] > 0).astype(np.float64)
    est = sb.BoostingClassifier().setNumBaseLearners(5).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(2))
    model = est.fit((X, y))
    ref = br.boosting_fit(X, y, classification=True, num_base_learners=5, max_depth=2)
    assert ref[3] == 1 and ref[0] == [1.0], "avgl == 0: beta == 0, weight 1.0, booster kept"
    assert_model_equals_reference(model, ref, X)
    assert np.array_equal(model.transform(X), y)


def test_depth0_classifier_stops_on_large_loss_and_drops_the_booster():
    """Six rows, one of class 1, and a seed whose first bag holds that row alone: the stump
    predicts class 1, avgl = (1 - 1/e) * 5/6 > 1/2, and the booster is dropped."""
    X = np.arange(6, dtype=np.float64)[:, None]
    y = np.array([0, 0, 0, 0, 0, 1.0])
    est = sb.BoostingClassifier().setNumBaseLearners(4).setSeed(11).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(0))
    model = est.fit((X, y))
    ref = br.boosting_fit(X, y, classification=True, num_base_learners=4, max_depth=0, seed=11)
    assert ref[3] == 1 and ref[0] == []
    assert model.numBaseModels == 0 and model.weights == [] and model.numClasses == 2
    assert np.array_equal(model.predict_raw(X), np.zeros((6, 2)))
    assert np.array_equal(model.transform(X), np.zeros(6))


def test_save_load_predicts_the_same(vehicle, cpusmall, tmp_path):
    X, y = vehicle
    cm = sb.BoostingClassifier().setNumBaseLearners(3).setBaseLearner(
        sb.DecisionTreeClassifier().setMaxDepth(3)).fit((X, y))
    cm.save(str(tmp_path / "c"))
    back = sb.BoostingClassificationModel.load(str(tmp_path / "c"))
    assert back.weights == cm.weights and back.numClasses == 5 and back.numBaseModels == 3
    assert np.array_equal(back.predict_raw(X), cm.predict_raw(X))
    assert np.array_equal(back.transform(X), cm.transform(X))
    Xr, yr = cpusmall
    rm = sb.BoostingRegressor().setNumBaseLearners(3).setLoss("absolute").setBaseLearner(
        sb.DecisionTreeRegressor().setMaxDepth(3)).fit((Xr, yr))
    rm.save(str(tmp_path / "r"))
    back = sb.BoostingRegressionModel.load(str(tmp_path / "r"))
    assert back.weights == rm.weights and back.get("loss") == "absolute"
    assert np.array_equal(back.transform(Xr), rm.transform(Xr))
