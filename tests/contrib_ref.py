"""References of sbag_predict_contributions (sbag.h's rule) for test_gpu_contrib.py and
test_contrib_host.py: `restated`, the rule operation for operation in NumPy (elementwise over
the rows, so every operation is one IEEE fp64 operation) and Python loops; `exact`, the Shapley
values by subset enumeration in fractions.Fraction; and the hand-built forests with covers."""
from fractions import Fraction
from math import factorial

import numpy as np

import weighted_ref as wr

# The bound of the tests that compare with `exact`: |out - exact| <= K 2^-53 (sum of |vw_l|).  K = 4 x
# the largest scaled error of `restated` against `exact` over the forests of these tests: 0.9814
# on the hand-built ones ("negative zero"), 0.16 on test_gpu_contrib.py's depth-3 fit.
K = 4 * 0.9814


def paths(tree, st, sub, class_index=-1, w=None):
    """[(vw_l, [[global feature, z, [(threshold, went left)]]])] for the leaves in pre-order."""
    st = np.asarray(st, np.float64)
    c = st[:, 0].copy()
    for k in range(1, st.shape[1] if class_index >= 0 else 1):
        c = c + st[:, k]
    out, todo = [], [(0, [])]
    while todo:
        i, path = todo.pop()
        if tree["left"][i] >= 0:
            todo += [(int(tree[s][i]), path + [(i, int(tree[s][i]))]) for s in ("right", "left")]
            continue
        els = []
        for p, ch in path:
            g, ratio = int(sub[tree["feature"][p]]), c[ch] / c[p]
            e = next((e for e in els if e[0] == g), None)
            if e is None:
                e = [g, None, []]
                els.append(e)
            e[1] = ratio if e[1] is None else e[1] * ratio
            e[2].append((np.float64(tree["threshold"][p]), ch == tree["left"][p]))
        v = np.float64(tree["prediction"][i])
        if class_index >= 0:
            v = st[i][class_index] / c[i] if class_index < st.shape[1] else np.float64(0.0)
        out.append((v if w is None else v * np.float64(w), els))
    return out


def forest_paths(trees, stats, subspaces, class_index=-1, weights=None):
    w = [None] * len(trees) if weights is None else weights
    return [p for t in range(len(trees)) for p in paths(trees[t], stats[t], subspaces[t], class_index, w[t])]


def scale(*forest):
    """The sum over the trees and their leaves of |vw_l|: what the error bounds are scaled by."""
    return sum(abs(float(vw)) for vw, _ in forest_paths(*forest))


def restated(trees, stats, subspaces, X, class_index=-1, weights=None):
    X = np.asarray(X, np.float64)
    N, F = X.shape
    acc = np.zeros((N, F + 1))
    Q = lambda a, b: np.float64(a) / np.float64(b)
    with np.errstate(all="ignore"):  # the branch a row does not take may overflow
        for vw, els in forest_paths(trees, stats, subspaces, class_index, weights):
            m = len(els)
            o = [np.logical_and.reduce([(X[:, g] <= thr) == left for thr, left in tests]) for g, _, tests in els]
            pw = [np.ones(N)] + [np.zeros(N) for _ in range(m)]
            for u in range(1, m + 1):
                old, z = list(pw), els[u - 1][1]
                for j in range(u + 1):
                    pw[j] = (z * old[j]) * Q(u - j, u + 1)
                    if j > 0:
                        pw[j] = np.where(o[u - 1], pw[j] + old[j - 1] * Q(j, u + 1), pw[j])
            b = vw
            for k, (g, z, _) in enumerate(els):
                rz, nxt, one, zero = 1.0 / z, pw[m], np.zeros(N), np.zeros(N)
                for i in range(m - 1, -1, -1):
                    tmp = nxt * Q(m + 1, i + 1)
                    one = one + tmp
                    nxt = pw[i] - (tmp * z) * Q(m - i, m + 1)
                    zero = zero + (pw[i] * rz) * Q(m + 1, m - i)
                acc[:, g] = acc[:, g] + (np.where(o[k], one, zero) * np.where(o[k], 1.0 - z, -z)) * vw
                b = b * z
            acc[:, F] = acc[:, F] + b
    return acc / np.float64(len(trees)) if weights is None else acc


def exact(trees, stats, subspaces, X, weights=None):
    """[N][F + 1] Fractions for variance trees: phi_g = sum over S of |S|! (n - |S| - 1)! / n!
    (f(S + g) - f(S)), f(S) the tree's value with the features outside S averaged out by cover (a
    tree of n <= 6 distinct features); the bias is f({})."""
    X = np.asarray(X, np.float64)
    N, F = X.shape
    out = [[Fraction(0)] * (F + 1) for _ in range(N)]
    for t, (tree, sub) in enumerate(zip(trees, subspaces)):
        c = [Fraction(float(row[0])) for row in np.asarray(stats[t], np.float64)]
        feats = sorted({int(sub[f]) for f in tree["feature"][tree["left"] >= 0]})
        n = len(feats)
        assert n <= 6
        w = Fraction(1) if weights is None else Fraction(float(weights[t]))

        def f(i, S, x):
            l, r, g = int(tree["left"][i]), int(tree["right"][i]), int(sub[tree["feature"][i]])
            if l < 0:
                return Fraction(float(tree["prediction"][i]))
            if g in S:
                return f(l if x[g] <= tree["threshold"][i] else r, S, x)
            return (c[l] * f(l, S, x) + c[r] * f(r, S, x)) / c[i]

        for r in range(N):
            val = [f(0, {feats[k] for k in range(n) if s >> k & 1}, X[r]) for s in range(1 << n)]
            out[r][F] += w * val[0]
            for k, s in ((k, s) for k in range(n) for s in range(1 << n) if not s >> k & 1):
                size = bin(s).count("1")
                out[r][feats[k]] += w * Fraction(factorial(size) * factorial(n - size - 1), factorial(n)) * (val[s | 1 << k] - val[s])
    L = 1 if weights is not None else len(trees)
    return [[v / L for v in row] for row in out]


def scaled_error(got, want, scale_):
    """max |got - exact| / (2^-53 scale), in exact arithmetic."""
    worst = max(abs(Fraction(float(g)) - e) for gr, er in zip(got, want) for g, e in zip(gr, er))
    return float(worst / (Fraction(1, 2 ** 53) * Fraction(scale_)))


# ---------------------------------------------------------------- hand-built forests with covers
def with_cover(tree, seed=0):
    """[n, 1] variance stats: the root covers 1000 rows, a left child a seeded share of its parent."""
    rng = np.random.default_rng(seed)
    c = np.zeros((len(tree), 1))
    c[0] = 1000.0
    for i in np.nonzero(tree["left"] >= 0)[0]:
        c[tree["left"][i]] = c[i] * rng.uniform(0.2, 0.8)
        c[tree["right"][i]] = c[i] - c[tree["left"][i]]
    return c


def chain(m):
    return wr.comb(np.arange(m) % 7 + 1.5, np.arange(m + 1) * 1.25 - 3.0, feature=np.arange(m))


HAND_BUILT = {  # name: trees; "chain m" tests m distinct features on its deepest path
    "single leaf": [wr.leaf(2.5)],
    "stump": [wr.stump(4.5, 1.0, 2.0)],
    # feature 0 three times on a path: satisfiable (left-deep) and with an empty interval (right-deep)
    "merged": [wr.comb([6.5, 0.5, 4.5, 2.5], [1.0, -2.0, 0.5, 3.0, 7.0], feature=[0, 1, 0, 0], left_deep=True),
               wr.comb([2.5, 6.5, 4.5], [1.0, 2.0, 4.0, 8.0])],
    "negative zero": [wr.stump(4.5, -0.0, 3.0)],
    "cancel": [wr.stump(4.5, 1.0, 2.0), wr.stump(4.5, -1.0, -2.0)],
    "chain 7": [chain(7)], "chain 8": [chain(8)], "chain 15": [chain(15)], "chain 16": [chain(16)],
}
EXACT_CASES = ["single leaf", "stump", "merged", "negative zero", "cancel"]  # m <= 6


def hand_built(case, F=16):
    """(trees, stats, subspaces, X): 130 rows of F features with values 0 .. 9; local feature j
    of every tree is global feature F - 1 - j."""
    trees = HAND_BUILT[case]
    X = np.random.default_rng(7).integers(0, 10, size=(130, F)).astype(np.float64)
    return trees, [with_cover(t) for t in trees], [list(range(F))[::-1]] * len(trees), X
