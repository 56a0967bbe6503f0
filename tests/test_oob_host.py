"""CPU: the out-of-bag entry point exists (header, library, bindings) and rejects null
arguments; oob_metrics restates the documented formulas on hand-made arrays."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_metrics


def test_header_library_and_bindings_name_predict_oob():
    txt = open(os.path.join(ROOT, "include", "sbag.h")).read()
    assert re.search(r"^\s*int\s+sbag_predict_oob\s*\(", txt, re.M)
    assert hasattr(nat.lib(), "sbag_predict_oob")
    assert "sbag_predict_oob" in nat.EXPORTED
    assert sb.oob_metrics is oob_metrics


def test_predict_oob_rejects_null_arguments():
    lib = nat.lib()
    assert lib.sbag_predict_oob(None, None, None, None, None, 1, nat.AGG_MEAN, None, None) == nat.SBAG_EINVAL
    assert len(lib.sbag_last_error()) > 0


# 6 rows, rows 1 and 4 uncovered (their predictions are NaN, as the engine writes them)
Y = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
PRED = np.array([1.5, np.nan, 3.0, 8.0, np.nan, 30.0])
N_OOB = np.array([2, 0, 1, 3, 0, 1], np.int32)
COV = [0, 2, 3, 5]


def _formula(metric):
    y = [Y[i] for i in COV]
    e = [PRED[i] - Y[i] for i in COV]
    if metric == "mse":
        return sum(x * x for x in e) / 4
    if metric == "rmse":
        return math.sqrt(sum(x * x for x in e) / 4)
    if metric == "mae":
        return sum(abs(x) for x in e) / 4
    m = sum(y) / 4
    return 1 - sum(x * x for x in e) / sum((v - m) ** 2 for v in y)


@pytest.mark.parametrize("metric", ["rmse", "mse", "mae", "r2"])
def test_regression_metrics_over_covered_rows(metric):
    got = oob_metrics(PRED, N_OOB, Y, False, metric)
    assert got["metric"] == metric
    assert got["numRows"] == 6
    assert got["coverage"] == 4 / 6
    assert got["value"] == pytest.approx(_formula(metric), rel=1e-15)


def test_default_metrics():
    assert oob_metrics(PRED, N_OOB, Y, False)["metric"] == "rmse"
    assert oob_metrics(PRED, N_OOB, Y, False)["value"] == oob_metrics(PRED, N_OOB, Y, False, "rmse")["value"]
    assert oob_metrics(PRED, N_OOB, Y, True)["metric"] == "accuracy"


def test_accuracy_over_covered_rows():
    y = np.array([0.0, 1.0, 2.0, 2.0, 1.0, 0.0, 3.0])
    pred = np.array([0.0, np.nan, 1.0, 2.0, 1.0, np.nan, 3.0])
    n_oob = np.array([1, 0, 2, 1, 4, 0, 1])
    got = oob_metrics(pred, n_oob, y, True, "accuracy")
    assert got == {"metric": "accuracy", "value": 4 / 5, "coverage": 5 / 7, "numRows": 7}


@pytest.mark.parametrize("classification", [False, True])
def test_no_covered_row_gives_nan_and_zero_coverage(classification):
    got = oob_metrics(np.full(5, np.nan), np.zeros(5, np.int32), np.arange(5.0), classification)
    assert math.isnan(got["value"])
    assert got["coverage"] == 0.0
    assert got["numRows"] == 5


def test_unknown_metric_is_rejected():
    with pytest.raises(sb.IllegalArgumentException):
        oob_metrics(PRED, N_OOB, Y, False, "accuracy")
    with pytest.raises(sb.IllegalArgumentException):
        oob_metrics(PRED, N_OOB, Y, True, "rmse")


def test_models_expose_the_oob_methods():
    for cls in (sb.BaggingRegressionModel, sb.BaggingClassificationModel):
        assert callable(cls.oobPredictions) and callable(cls.oobScore)
    m = sb.BaggingRegressionModel([], [])
    assert m.learner_range is None
