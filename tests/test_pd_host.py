"""CPU: pd_ref.py on a two-tree forest worked by hand.

Rows (x0, x1): (0, 0), (1, 0), (2, 1), (3, 1); feature 0 over the grid [0.5, 1.0, 2.5].
Tree A, a stump on x0 at 1.0 (ties go left): all four rows go left for 0.5 and 1.0, right for 2.5.
Tree B tests x1 at 0.5 first: the two rows with x1 = 0 stop in its first leaf whatever x0 is; the
other two reach a test of x0 at 2.0 and go left for 0.5 and 1.0, right for 2.5."""
import numpy as np

import pd_ref
import weighted_ref as wr

X = np.array([[0, 0], [1, 0], [2, 1], [3, 1]], np.float64)
GRID = [0.5, 1.0, 2.5]
SUBS = [[0, 1], [0, 1]]


def test_counts_and_mean():
    trees = [wr.stump(1.0, 10.0, 20.0), wr.comb([0.5, 2.0], [1.0, 3.0, 7.0], feature=[1, 0])]
    (va, ca), (vb, cb) = pd_ref.counts(trees, SUBS, X, 0, GRID)
    assert va.tolist() == [10.0, 20.0] and ca.tolist() == [[4, 4, 0], [0, 0, 4]]
    assert vb.tolist() == [1.0, 3.0, 7.0] and cb.tolist() == [[2, 2, 2], [2, 2, 0], [0, 0, 2]]
    pd, tree_pd = pd_ref.mean(trees, SUBS, X, 0, GRID)
    assert tree_pd.tolist() == [[10.0, 10.0, 20.0], [2.0, 2.0, 4.0]]
    assert pd.tolist() == [6.0, 6.0, 12.0]
    assert pd_ref.mean(trees, SUBS, X, 0, GRID, weights=[0.5, 2.0])[0].tolist() == [9.0, 9.0, 18.0]
    # feature 1 instead: tree A never tests it
    pd1, tree_pd1 = pd_ref.mean(trees, SUBS, X, 1, [0.0, 1.0])
    assert tree_pd1.tolist() == [[15.0, 15.0], [1.0, 4.0]] and pd1.tolist() == [8.0, 9.5]
    assert X.tolist() == [[0, 0], [1, 0], [2, 1], [3, 1]]  # the caller's rows are left alone


def test_votes():
    trees = [wr.stump(1.0, 0.0, 1.0), wr.comb([0.5, 2.0], [0.0, 1.0, 2.0], feature=[1, 0])]
    got = pd_ref.votes(trees, SUBS, X, 0, GRID, 4)
    assert got.tolist() == [[0.75, 0.25, 0, 0], [0.75, 0.25, 0, 0], [0.25, 0.5, 0.25, 0]]
