"""A plain Python restatement of the root of one variance tree, the reference that
test_label_scale_host.py holds the C oracle to where the oracle itself is the specification:
labels so small that Spark's y*y and its sums of squares underflow gradually.  It shares
neither the oracle's C code nor its compiler flags (contraction, flush-to-zero): every
operation is one Python float operation (IEEE binary64, round to nearest, subnormals kept),
no NumPy reduction, no math.fsum.

The thresholds are the oracle's (oracle.find_splits); a row goes to bin
searchsorted(thr, x, "left") (the first threshold >= x: ContinuousSplit.shouldGoLeft is
x <= threshold).  DTStatsAggregator.update adds (1, y, y*y) per exploded row in row order
(a row drawn c times is c consecutive rows; one partition), VarianceAggregator.update as
`weight * label` and `weight * label * label` with weight 1.0.  binsToBestSplit at the root:
prefix sums in bin order (mergeForFeature), right = total - left, the parent's stats
left + right of the first candidate of the first feature with splits
(calculateImpurityStats with stats == null), Variance.calculate, the first maximum over a
feature's splits and then over the features (maxBy)."""
import numpy as np

import oracle

DOUBLE_MIN_VALUE = -1.7976931348623157e308  # Double.MinValue


def variance(count, total, total_sq):
    """Variance.calculate(count, sum, sumSquares)."""
    if count == 0:
        return 0.0
    squared_loss = total_sq - (total * total) / count
    return squared_loss / count


def root(X, y, counts, sub, max_bins, min_instances_per_node=1, min_info_gain=0.0):
    """The root of DecisionTreeRegressor on the subbag `counts` (draws per row) sliced to the
    features `sub`: a dict of feature (index into sub, -1 at a leaf), split_bin, gain,
    impurity, prediction as the oracle's node 0 reports them (a leaf: gain -1.0, and
    impurity -1.0 when its stats are invalid), before pruning."""
    X = np.asarray(X, np.float64)
    labels = [float(v) for v in np.asarray(y, np.float64)]
    draws = [int(c) for c in counts]
    thr, bins = [], []
    for f in sub:
        t, _ = oracle.find_splits(X, counts, int(f), max_bins)
        thr.append(t)
        bins.append([int(b) for b in np.searchsorted(t, X[:, int(f)], "left")])
    cells = [[[0.0, 0.0, 0.0] for _ in range(len(t) + 1)] for t in thr]
    for i, c in enumerate(draws):
        lab = labels[i]
        for _ in range(c):
            for fl in range(len(thr)):
                st = cells[fl][bins[fl][i]]
                st[0] += 1.0
                st[1] += 1.0 * lab
                st[2] += 1.0 * lab * lab
    parent, parent_imp = None, 0.0
    best_f, best_s, best_gain, best_valid = -1, -1, 0.0, False
    for fl, t in enumerate(thr):
        nsp = len(t)
        if nsp == 0:
            continue
        fa = cells[fl]
        for s in range(nsp):  # mergeForFeature: prefix over the bins
            for j in range(3):
                fa[s + 1][j] += fa[s][j]
        fbest_s, fbest_gain, fbest_valid = -1, 0.0, False
        for s in range(nsp):
            left = list(fa[s])
            right = [fa[nsp][j] - left[j] for j in range(3)]
            if parent is None:
                parent = [left[j] + right[j] for j in range(3)]
                parent_imp = variance(*parent)
            lc, rc = int(left[0]), int(right[0])
            if lc < min_instances_per_node or rc < min_instances_per_node:
                gain, valid = DOUBLE_MIN_VALUE, False
            else:
                li, ri = variance(*left), variance(*right)
                lw, rw = float(lc) / float(lc + rc), float(rc) / float(lc + rc)
                gain, valid = parent_imp - lw * li - rw * ri, True
                if gain < min_info_gain:
                    gain, valid = DOUBLE_MIN_VALUE, False
            if fbest_s < 0 or gain > fbest_gain:
                fbest_s, fbest_gain, fbest_valid = s, gain, valid
        if best_f < 0 or fbest_gain > best_gain:
            best_f, best_s, best_gain, best_valid = fl, fbest_s, fbest_gain, fbest_valid
    if best_f < 0:
        raise ValueError("no feature has splits")
    count = int(parent[0])
    prediction = 0.0 if count == 0 else parent[1] / float(count)
    if best_gain <= 0:  # a leaf: LearningNode.toNode reports no split
        return dict(feature=-1, split_bin=-1, gain=-1.0,
                    impurity=parent_imp if best_valid else -1.0, prediction=prediction)
    return dict(feature=best_f, split_bin=best_s, gain=best_gain, impurity=parent_imp,
                prediction=prediction)
