"""NumPy restatement of sbag_eval_staged, written from the text of include/sbag.h: the
per-stage statistics of a bagged ensemble (stage l = its first l + 1 trees) from the bag
counts, the per-tree predictions and the labels, with the documented order of the two fp64
sums.  Shared by tests/test_staged_host.py (which checks it against a literal per-row,
per-prefix loop) and tests/test_gpu_staged.py (which holds the device to it)."""
import numpy as np

import oracle
from parity_utils import oracle_forest

STAGE_FIELDS = ("covered", "correct", "sum_se", "sum_ae")
STAGE_DTYPE = np.dtype([("covered", "<i8"), ("correct", "<i8"), ("sum_se", "<f8"), ("sum_ae", "<f8")])
TILE = 512

# seeds of order_case the GPU tests use; tests/test_staged_host.py asserts that on each of
# them the tile order gives other bits than the left-to-right sum and than np.sum
ORDER_SEEDS = (3, 5)
ORDER_N = 1500


def tile_sum(v):
    """The documented sum of per-row terms: tiles of 512 consecutive rows (the last one
    padded with +0.0), each summed by halving (h = 256, 128, ..., 1: v[i] = v[i] + v[i + h]
    for i < h), the tile sums added left to right from 0.0."""
    v = np.asarray(v, np.float64)
    tiles = (len(v) + TILE - 1) // TILE
    t = np.zeros(tiles * TILE)
    t[:len(v)] = v
    t = t.reshape(tiles, TILE)
    h = TILE // 2
    while h >= 1:
        t[:, :h] = t[:, :h] + t[:, h:2 * h]
        h //= 2
    s = 0.0
    for k in range(tiles):
        s = s + float(t[k, 0])
    return s


def staged_terms(counts, per_tree, y, cls):
    """Per stage, the per-row (covered, correct, se, ae): the learner loop of
    test_gpu_oob.oob_vectorised, every prefix kept.  counts None: no learner is masked."""
    per_tree = np.asarray(per_tree, np.float64)
    y = np.asarray(y, np.float64)
    L, N = per_tree.shape
    rows = np.arange(N)
    n = np.zeros(N, np.int64)
    s = np.zeros(N)
    if cls:
        C = int(per_tree.max()) + 1 if per_tree.size else 1
        cnt = np.zeros((C, N), np.int64)
        best = np.zeros(N, np.int64)
        acc = np.full(N, np.nan)
    for i in range(L):
        oob = np.ones(N, bool) if counts is None else np.asarray(counts[i]) == 0
        n = n + oob
        covered = n > 0
        zero = np.zeros(N)
        if cls:
            v = per_tree[i].astype(np.int64)
            k = cnt[v, rows] + 1
            cnt[v[oob], rows[oob]] = k[oob]
            upd = oob & (k > best)
            best = np.where(upd, k, best)
            acc = np.where(upd, per_tree[i], acc)
            yield covered, covered & (acc == y), zero, zero
        else:
            s = np.where(oob, s + per_tree[i], s)
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(covered, s / n.astype(np.float64) - y, 0.0)
            yield covered, np.zeros(N, bool), np.where(covered, e * e, 0.0), np.where(covered, np.abs(e), 0.0)


def stats_of_terms(covered, correct, se, ae):
    return int(covered.sum()), int(correct.sum()), tile_sum(se), tile_sum(ae)


def staged_ref(counts, per_tree, y, cls):
    """The four fields per stage (STAGE_DTYPE [L])."""
    out = np.zeros(len(per_tree), STAGE_DTYPE)
    for i, terms in enumerate(staged_terms(counts, per_tree, y, cls)):
        out[i] = stats_of_terms(*terms)
    return out


def stats_of_prediction(pred, n_oob, y, cls):
    """One stage's fields from a finished prediction (NaN / n_oob == 0 where not covered)."""
    covered = np.asarray(n_oob) > 0
    y = np.asarray(y, np.float64)
    if cls:
        zero = np.zeros(len(y))
        return stats_of_terms(covered, covered & (pred == y), zero, zero)
    e = np.where(covered, np.where(covered, pred, 0.0) - y, 0.0)
    return stats_of_terms(covered, np.zeros(len(y), bool), np.where(covered, e * e, 0.0),
                          np.where(covered, np.abs(e), 0.0))


def assert_stats_equal(got, want):
    """covered / correct equal, sum_se / sum_ae bit for bit."""
    assert len(got) == len(want)
    for f in STAGE_FIELDS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.tobytes() == b.tobytes(), (f, a, b)


_order_cases = {}


def order_case(seed):
    """N = 1,500 rows of u8-coded features with real-valued labels drawn from a normal
    distribution, and the oracle's 8 depth-5 regression trees on Poisson bags over two
    partitions: (X, y, params, oracle forest, counts, per-tree predictions)."""
    if seed not in _order_cases:
        rng = np.random.default_rng(seed)
        N = ORDER_N
        X = np.round(rng.normal(size=(N, 6)) * 6) / 8
        y = rng.normal(size=N) + X[:, 0] / 4
        p = dict(cls=False, replacement=True, ratio=1.0, seed=oracle.DEFAULT_SEED_REGRESSOR, lb=0, L=8,
                 depth=5, part=[0, 700, N])
        counts = oracle.bag(True, 1.0, 0, 8, p["seed"], p["part"], N)
        subs = [oracle.subspace(1.0, X.shape[1], p["seed"] + i) for i in range(8)]
        orf = oracle_forest(X, y, counts, subs, 5, 32, False, part=p["part"])
        _, per_tree = oracle.predict(orf, X, False, per_tree=True)
        _order_cases[seed] = (X, y, p, orf, counts, per_tree)
    return _order_cases[seed]
