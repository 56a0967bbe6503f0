"""CPU: the staged-evaluation entry point exists (header, library, bindings) and rejects null
arguments; tests/staged_ref.py (the NumPy restatement the GPU tests hold the device to) equals
a literal per-row, per-prefix loop; staged_metrics restates the documented formulas; and the
inputs of the GPU order tests make the summation order visible."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat
from spark_bagging_amd.ml import oob_metrics, staged_metrics

import oracle
from parity_utils import oracle_forest
from staged_ref import (ORDER_N, ORDER_SEEDS, STAGE_DTYPE, order_case, staged_ref, staged_terms, tile_sum)


def test_header_library_and_bindings_name_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "sbag.h")).read()
    assert re.search(r"^\s*int\s+sbag_eval_staged\s*\(", txt, re.M)
    assert "sbag_stage_stats" in txt
    assert hasattr(nat.lib(), "sbag_eval_staged")
    assert "sbag_eval_staged" in nat.EXPORTED
    assert callable(nat.eval_staged)
    assert nat.STAGE_DTYPE == STAGE_DTYPE and nat.STAGE_DTYPE.itemsize == 32
    assert sb.staged_metrics is staged_metrics
    for model in (sb.BaggingRegressionModel, sb.BaggingClassificationModel):
        assert callable(model.oobScoreCurve) and callable(model.evaluateEachIteration)


def test_all_null_call_is_rejected():
    lib = nat.lib()
    assert lib.sbag_eval_staged(None, None, None, None, None, 1, nat.AGG_MEAN, None) == nat.SBAG_EINVAL
    assert len(lib.sbag_last_error()) > 0


# ---------------------------------------------------------------- tile_sum
def test_tile_sum_follows_the_halving_order():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 511, 512, 513, 1025, 1500):
        v = rng.normal(size=n) ** 2
        pad = list(v) + [0.0] * (-n % 512)
        total = 0.0
        for k in range(len(pad) // 512):
            t = pad[512 * k:512 * k + 512]
            h = 256
            while h >= 1:
                for i in range(h):
                    t[i] = t[i] + t[i + h]
                h //= 2
            total = total + t[0]
        assert tile_sum(v) == total
    assert math.copysign(1.0, tile_sum([])) == 1.0  # no rows: +0.0


# ---------------------------------------------------------------- staged_ref vs the literal rule
def literal_prefix_terms(counts, per_tree, y, cls, l):
    """oob_by_rows' rule (tests/test_gpu_oob.py) applied to the learners [0, l], one row at a
    time: per row (covered, correct, se, ae)."""
    L, N = per_tree.shape
    out = []
    for r in range(N):
        votes = [float(per_tree[i, r]) for i in range(l + 1) if counts is None or counts[i, r] == 0]
        if not votes:
            out.append((False, False, 0.0, 0.0))
            continue
        if cls:
            final = {}
            for v in votes:
                final[v] = final.get(v, 0) + 1
            top = max(final.values())
            run = {}
            for v in votes:
                run[v] = run.get(v, 0) + 1
                if run[v] == top:
                    pred = v
                    break
            out.append((True, pred == float(y[r]), 0.0, 0.0))
        else:
            s = 0.0
            for v in votes:
                s = s + v
            e = s / float(len(votes)) - float(y[r])
            out.append((True, False, e * e, abs(e)))
    return out


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("cls", [False, True])
def test_staged_ref_equals_the_literal_rule_on_every_prefix(cls, masked):
    rng = np.random.default_rng(21)
    N, L = 300, 7
    counts = rng.poisson(1.0, size=(L, N)).astype(np.uint8) if masked else None
    if cls:
        per_tree = rng.integers(0, 4, size=(L, N)).astype(np.float64)
        y = rng.integers(0, 4, N).astype(np.float64)
    else:
        per_tree = rng.normal(size=(L, N))
        y = rng.normal(size=N)
    ref = staged_ref(counts, per_tree, y, cls)
    assert ref.dtype == STAGE_DTYPE and len(ref) == L
    for l, (covered, correct, se, ae) in enumerate(staged_terms(counts, per_tree, y, cls)):
        lit = literal_prefix_terms(counts, per_tree, y, cls, l)
        assert covered.tolist() == [t[0] for t in lit]
        assert correct.tolist() == [t[1] for t in lit]
        assert se.tobytes() == np.array([t[2] for t in lit]).tobytes()  # bit for bit
        assert ae.tobytes() == np.array([t[3] for t in lit]).tobytes()
        assert ref["covered"][l] == sum(t[0] for t in lit)
        assert ref["correct"][l] == sum(t[1] for t in lit)
        assert ref["sum_se"][l] == tile_sum([t[2] for t in lit])
        assert ref["sum_ae"][l] == tile_sum([t[3] for t in lit])
    if masked:
        assert 0 < ref["covered"][0] < N and ref["covered"][-1] > ref["covered"][0]
    else:
        assert (ref["covered"] == N).all()


# ---------------------------------------------------------------- staged_metrics
def test_staged_metrics_formulas_nan_and_refusals():
    stats = np.zeros(3, STAGE_DTYPE)
    stats["covered"] = [0, 4, 8]
    stats["correct"] = [0, 1, 6]
    stats["sum_se"] = [0.0, 9.0, 2.0]
    stats["sum_ae"] = [0.0, 5.0, 3.0]
    r = staged_metrics(stats, 8, False)
    assert r["metric"] == "rmse" and r["numRows"] == 8
    np.testing.assert_array_equal(r["coverage"], [0.0, 0.5, 1.0])
    np.testing.assert_array_equal(r["values"], [np.nan, 1.5, 0.5])
    np.testing.assert_array_equal(staged_metrics(stats, 8, False, "mse")["values"], [np.nan, 2.25, 0.25])
    np.testing.assert_array_equal(staged_metrics(stats, 8, False, "mae")["values"], [np.nan, 1.25, 0.375])
    a = staged_metrics(stats, 8, True)
    assert a["metric"] == "accuracy"
    np.testing.assert_array_equal(a["values"], [np.nan, 0.25, 0.75])
    for cls, name in ((False, "r2"), (False, "accuracy"), (True, "rmse"), (True, "r2"), (False, "nope")):
        with pytest.raises(sb.IllegalArgumentException):
            staged_metrics(stats, 8, cls, name)
    empty = staged_metrics(np.zeros(2, STAGE_DTYPE), 0, False)
    assert np.isnan(empty["values"]).all() and (empty["coverage"] == 0).all()


@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_last_stage_equals_oob_metrics_within_the_summation_bound(seed):
    """The relative gap between two summation orders of N non-negative terms is at most
    2 (N - 1) 2^-53 (each order is within (N - 1) 2^-53 of the exact sum, to first order)."""
    X, y, p, orf, counts, per_tree = order_case(seed)
    ref = staged_ref(counts, per_tree, y, False)
    n_oob = (counts == 0).sum(axis=0)
    s = np.zeros(len(y))
    for i in range(len(counts)):
        s = np.where(counts[i] == 0, s + per_tree[i], s)
    with np.errstate(invalid="ignore", divide="ignore"):
        pred = np.where(n_oob > 0, s / n_oob, np.nan)
    bound = 2 * (len(y) - 1) * 2.0 ** -53
    for m in ("mse", "mae"):
        want = oob_metrics(pred, n_oob, y, False, m)
        got = staged_metrics(ref, len(y), False, m)
        assert got["coverage"][-1] == want["coverage"]
        assert abs(got["values"][-1] - want["value"]) <= bound * want["value"]


# ---------------------------------------------------------------- the order is visible
@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_order_is_visible_on_the_gpu_tests_inputs(seed):
    """A precondition of tests/test_gpu_staged.py's order tests: on each of their inputs the
    documented tile order gives, in at least one stage, other bits than the left-to-right sum
    and than np.sum (on dyadic labels and leaves every order would agree and the GPU tests
    would show nothing about order)."""
    X, y, p, orf, counts, per_tree = order_case(seed)
    assert len(y) == ORDER_N == 1500
    vs_seq = vs_np = 0
    for covered, correct, se, ae in staged_terms(counts, per_tree, y, False):
        for v in (se, ae):
            vs_seq += tile_sum(v) != float(np.cumsum(v)[-1])
            vs_np += tile_sum(v) != float(np.sum(v))
    assert vs_seq >= 1 and vs_np >= 1
