"""CPU: contrib_ref.restated, the NumPy restatement of sbag_predict_contributions' rule, against
contrib_ref.exact, Shapley values enumerated in exact rationals, on the hand-built forests with
at most 6 distinct features: the rule is the textbook quantity where there is no GPU.  The bound is
K 2^-53 times the sum of the |leaf values|, K = 4 x the largest scaled error measured over these
forests and the fitted forest of test_gpu_contrib.py (contrib_ref.K)."""
import numpy as np
import pytest

import contrib_ref as cr


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", cr.EXACT_CASES)
def test_restated_is_the_shapley_value(case, weighted):
    trees, stats, subs, X = cr.hand_built(case)
    w = np.random.default_rng(1).normal(size=len(trees)) if weighted else None
    got = cr.restated(trees, stats, subs, X[:40], -1, w)
    err = cr.scaled_error(got, cr.exact(trees, stats, subs, X[:40], w), cr.scale(trees, stats, subs, -1, w))
    print(f"{case}, weighted={weighted}: scaled error {err}")
    assert err <= cr.K
