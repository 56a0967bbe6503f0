"""GPU: in-bag-sized ("tight") entry lists on the integer engine.

Every fit keeps two entry lists per replica with a per-replica stride `cap`
(sbag_timing.entry_capacity).  The integer engine takes cap = N until the lists pass 40 % of
the device, and min(N, roundup64(largest in-bag row count + 4096)) above -- a path no
benchmark-sized test reaches on its own.  SBAG_ENT_TIGHT=1 (read per fit) takes it at small
shapes; every case here

  * asserts entry_capacity < N and = min(N, roundup64(max_r inbag_r + 4096)) recomputed from
    the oracle's bags (k_chunk_rows, the pre-count that sizes the lists, runs only on this
    path: an under-count would let k_compact write past a replica's list),
  * compares the forest to the oracle node by node, bit-exact,
  * fits the same inputs again with SBAG_ENT_TIGHT=0 (entry_capacity == N) and compares trees
    and stats byte for byte.

At L > 1 the replicas' bases r cap differ from r N, so one consumer of the stride (k_compact,
the root segments, the class-tile grouping, the global value counts, the split-sample
copy-back, k_bin_ranked, the entry ranking, the level loop's ping-pong, the MFMA root)
addressing by N reads another replica's entries and the trees differ from the oracle's.
Everything is integer statistics: no tolerances."""
import math
import os

import numpy as np
import pytest

import oracle
from conftest import DATA
from parity_utils import assert_forest_equal, oracle_forest

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


@pytest.fixture(scope="module")
def cpusmall():
    return sb.load_libsvm(os.path.join(DATA, "cpusmall.svm"))


_cache = {}  # inputs and their oracle forests: computed once, shared by the parametrised cases


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _tight_capacity(counts, N):
    """fit_range_impl's tight capacity from the oracle's bags [R][N]."""
    most = int((np.asarray(counts) > 0).sum(axis=1).max())
    return min(N, (most + 4096 + 63) // 64 * 64)


def _forest_bytes(forest):
    return [tuple(a.tobytes() for a in forest.tree(t)) for t in range(len(forest))]


def _check_tight_and_full(monkeypatch, fit, N, counts, orf):
    """fit(): one fit of the case's inputs under the environment of the moment.  Returns the
    tight fit's timing."""
    want = _tight_capacity(counts, N)
    assert want < N, f"shape too small for tight lists: capacity {want}, N {N}"
    monkeypatch.setenv("SBAG_ENT_TIGHT", "1")
    tight = fit()
    t = tight.timing()
    assert t["chain_ms"] == 0.0, t  # the integer engine
    assert t["entry_capacity"] == want and t["entry_capacity"] < N, (t["entry_capacity"], want, N)
    assert_forest_equal(tight, orf)
    monkeypatch.setenv("SBAG_ENT_TIGHT", "0")
    full = fit()
    tf = full.timing()
    assert tf["chain_ms"] == 0.0, tf
    assert tf["entry_capacity"] == N, (tf["entry_capacity"], N)
    assert _forest_bytes(tight) == _forest_bytes(full)
    return t


def _fit(ctx, ds, L, *, replacement, ratio, seed, depth, cls, part=None, compat=True):
    return nat.fit(ctx, ds, replacement=replacement, sample_ratio=ratio, seed=seed, learner_begin=0,
                   learner_end=L, subspace_ratio=1.0, subspace_bug_compat=compat,
                   partition_offsets=part, max_depth=depth, max_bins=32,
                   impurity=nat.IMPURITY_GINI if cls else nat.IMPURITY_VARIANCE)


def _oracle(X, y, L, *, replacement, ratio, seed, depth, cls, part=None, compat=True):
    N, F = X.shape
    counts = oracle.bag(replacement, ratio, 0, L, seed, part or [0, N], N)
    subs = [oracle.subspace(ratio if compat else 1.0, F, seed + i) for i in range(L)]
    return counts, oracle_forest(X, y, counts, subs, depth, 32, cls, part=part)


def _synthetic(ctx, N, F, seed_data, classes):
    ds = nat.DeviceDataset.synthetic(N, F, seed=seed_data, num_classes=classes, ctx=ctx)
    try:
        return ds.features(), ds.labels()
    finally:
        ds.free()


def _run(ctx, monkeypatch, key, make_xy, L, **kw):
    """The case's data and oracle forest (cached under key), then the tight and the full fit."""
    def make():
        X, y = make_xy()
        return (X, y) + _oracle(X, y, L, **kw)
    X, y, counts, orf = _cached(key, make)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        return _check_tight_and_full(monkeypatch, lambda: _fit(ctx, ds, L, **kw), len(y), counts, orf)
    finally:
        ds.free()


# ------------------------------------------------- variance, u8 codes
@pytest.mark.parametrize("rl", [None, "0"], ids=["row-lane", "k_hist"])
@pytest.mark.parametrize("N", [20_000, 20_001])
def test_variance_u8_codes(ctx, monkeypatch, N, rl):
    """5 Poisson(1) replicas of 100 u8 features, depth 7, with the row-lane histogram and with
    k_hist.  Odd N: the counts of replicas r >= 1 are off 16-byte alignment, so k_chunk_rows
    counts whole chunks byte by byte; even N: 16 counts per load, the last chunk the tail."""
    if rl is not None:
        monkeypatch.setenv("SBAG_HIST_RL", rl)
    _run(ctx, monkeypatch, ("u8", N), lambda: _synthetic(ctx, N, 100, 41, 0), 5, replacement=True,
         ratio=1.0, seed=SEED_REG, depth=7, cls=False)


def test_variance_partitions_bernoulli(ctx, monkeypatch):
    """Three uneven partitions, one of them empty, Bernoulli bags at 0.5 (the sampler's streams
    are per partition; the lists' stride is about half of N)."""
    N = 20_000
    _run(ctx, monkeypatch, "p3", lambda: _synthetic(ctx, N, 24, 43, 0), 4, replacement=False,
         ratio=0.5, seed=SEED_REG, depth=6, cls=False, part=[0, 7001, 7001, N], compat=False)


@pytest.mark.parametrize("L", [1, 7])
def test_low_ratio_cpusmall(ctx, cpusmall, monkeypatch, L):
    """Poisson bags at ratio 0.05 of cpusmall's 8192 rows: ~400 in-bag rows, a stride of ~4.5 k,
    so the replicas' bases r cap lie far from r N; continuous features, thresholds per replica
    from the whole subbag."""
    t = _run(ctx, monkeypatch, ("low", L), lambda: cpusmall, L, replacement=True, ratio=0.05,
             seed=SEED_REG, depth=5, cls=False, compat=False)
    assert t["entry_capacity"] < 8192 * 0.6


# ------------------------------------------------- gini, 64 classes: grouped class tiles
@pytest.mark.parametrize("case", ["known-cursors", "replacement", "resident"])
def test_gini_64_classes_class_tiles(ctx, monkeypatch, case):
    """24 000 x 100, 64 classes, depth 12: the class tiles' grouping copies (entG) follow the
    lists' stride.  Without replacement at 0.5 under SBAG_TILE_CHECK=1 (k_tile_scatter_known:
    every cursor must end at its tile's end), with replacement (k_tile_count /
    k_tile_scatter), and with the root's grouping kept for the whole fit
    (SBAG_TILE_RESIDENT=1)."""
    replacement = case == "replacement"
    if case == "known-cursors":
        monkeypatch.setenv("SBAG_TILE_CHECK", "1")
    if case == "resident":
        monkeypatch.setenv("SBAG_TILE_RESIDENT", "1")
    _run(ctx, monkeypatch, ("gini64", replacement), lambda: _synthetic(ctx, 24_000, 100, 17, 64), 2,
         replacement=replacement, ratio=1.0 if replacement else 0.5, seed=SEED_CLS, depth=12, cls=True)


# ------------------------------------------------- continuous features, sampled split finding
def _continuous(n_rows, cls, P):
    rng = np.random.default_rng(n_rows + P)
    X = np.round(rng.normal(size=(n_rows, 5)), 2)
    X[rng.random((n_rows, 5)) < 0.15] = 0.0
    y = (rng.integers(0, 5, n_rows) if cls else rng.integers(-256, 256, n_rows) / 16).astype(np.float64)
    return X, y


@pytest.mark.parametrize("n_rows,cls,P,budget_mb", [(30_000, False, 3, None), (16_000, True, 2, None),
                                                   (30_000, False, 3, "0.5")],
                         ids=["reg-p3", "cls-p2", "reg-p3-split-range"])
def test_continuous_features_sampled_splits(ctx, monkeypatch, n_rows, cls, P, budget_mb):
    """Subbags past 10^4 rows: thresholds per replica from findSplits' sample (the split sample
    and its copy-back, the global value counts, k_bin_ranked and the entry ranking all walk
    entA by the stride); with a 0.5 MB bins budget the three learners are fitted one by one
    and entry_capacity is the largest of the parts."""
    part = [int(round(i * n_rows / P)) for i in range(P + 1)]
    seed = SEED_CLS if cls else SEED_REG
    kw = dict(replacement=True, ratio=1.0, seed=seed, depth=6, cls=cls, part=part)
    key = ("cont", n_rows, cls, P)

    def make():
        X, y = _continuous(n_rows, cls, P)
        return (X, y) + _oracle(X, y, 3, **kw)
    X, y, counts, orf = _cached(key, make)
    assert oracle.split_sample_fraction(int(counts[0].sum()), 32) < 1.0
    whole_launches = None
    if budget_mb is not None:
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        try:
            whole_launches = _fit(ctx, ds, 3, **kw).timing()["hist_launches"]
        finally:
            ds.free()
        monkeypatch.setenv("SBAG_BINS_BUDGET_MB", budget_mb)
    t = _run(ctx, monkeypatch, key, None, 3, **kw)
    if whole_launches is not None:  # every part ran its own level loop
        assert t["hist_launches"] > whole_launches, (t["hist_launches"], whole_launches)


# ------------------------------------------------- MFMA root
def test_mfma_root(ctx, monkeypatch):
    """70 000 x 9 shared identity bins, 40 replicas, dyadic labels: the root histogram as an
    int8 MFMA contraction (root_ms > 0), the levels below it from the tight lists."""
    N, F, L = 70_000, 9, 40

    def data():
        rng = np.random.default_rng(N + F)
        levels = rng.choice([2, 5, 17, 32], size=F)
        X = np.stack([rng.integers(0, levels[f], size=N) for f in range(F)], axis=1).astype(np.float64)
        return X, (X[:, 0] * 3.0 - X[:, 1] + rng.integers(-8, 9, size=N)) / 4.0
    monkeypatch.setenv("SBAG_ROOT_MFMA", "1")
    t = _run(ctx, monkeypatch, "mfma", data, L, replacement=True, ratio=1.0, seed=SEED_REG, depth=6,
             cls=False)
    assert t["root_ms"] > 0.0 and t["root_mfma_ops"] > 0.0, t


# ------------------------------------------------- caller-supplied counts (sbag_fit_booster)
def _booster_data():
    N, F = 20_000, 6
    rng = np.random.default_rng(31)
    X = rng.integers(0, 32, size=(N, F)).astype(np.float64)
    counts = rng.integers(1, 256, size=N).astype(np.uint8)
    counts[rng.random(N) < 0.5] = 0
    counts[[3, 4, 5, N - 1]] = [128, 129, 255, 255]
    counts[[6, 7]] = [127, 1]
    kin = math.isqrt((2**53 - 1) // (N * 255))  # dyadic labels inside the integer engine's 2^53 rule
    k = rng.integers(-kin, kin + 1, size=N) // 2 + (X[:, 1] * (kin // 64)).astype(np.int64)
    assert N * 255 * int(np.abs(k).max()) ** 2 < 2**53
    y = k.astype(np.float64)
    sub = np.arange(F, dtype=np.int32)
    orf = oracle.fit(X, y, counts[None, :], [sub], max_depth=6, max_bins=32)
    return X, y, counts, sub, orf


def test_booster_counts_with_high_bytes(ctx, monkeypatch):
    """A booster's counts are the caller's bytes: about half of them 0, the rest over 1..255
    with 128, 129 and 255 among them.  k_chunk_rows counts the nonzero bytes of a 32-bit word
    with a carry into bit 7, which must also hold for bytes >= 0x80 -- Poisson bags never
    get there."""
    X, y, counts, sub, orf = _cached("booster", _booster_data)
    N = len(y)
    nz = counts[counts > 0]
    assert 0.4 < (counts == 0).mean() < 0.6 and {1, 127, 128, 129, 255} <= set(nz.tolist())
    assert (nz >= 128).mean() > 0.4
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(N), ctx)
    try:
        _check_tight_and_full(monkeypatch, lambda: nat.fit_booster(ctx, ds, y, counts, sub, max_depth=6,
                                                                   max_bins=32),
                              N, counts[None, :], orf)
    finally:
        ds.free()
