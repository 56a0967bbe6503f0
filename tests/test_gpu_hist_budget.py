"""GPU: the packed LDS histogram words at the edges of their bit budget.

A variance word is (c << cshift) + c (k + K0), flushed from LDS after at most flush_limit
entries of one node; the exact fallback's plane holds c k^2; a gini word is a 32-bit count
(hist_word_budget, csrc/sbag_budget.h; tests/test_hist_budget_host.py sweeps the arithmetic).
Here the kernels run at those edges, at small shapes: SBAG_HIST_FLUSH_LIMIT=256 makes one
workgroup hold more than flush_limit entries of a node, so the flush that the limit alone
causes happens (sbag_timing.hist_midrun_flushes counts them) -- the second flush of a run adds
where the first stored; labels over the whole |k| < 2^23; the hand-over to the fp64 engine at
N cmax kabs^2 = 2^53 from both sides; draw counts up to 255; the MFMA root at its int32 bound.

Every comparison is bit for bit against the oracle (node stats included); every label set is
dyadic with all sums below 2^53 but the one just past the hand-over, where the oracle follows
Spark's summation order.  chain_ms tells the engines apart: only the fp64 engine records it
(T_CHAIN, whenever a node has a candidate split), the integer engine leaves it 0."""
import math

import numpy as np
import pytest

import oracle
from parity_utils import assert_forest_equal, assert_tree_equal, fuzz_case_labels, oracle_forest

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER
KMAX = 2**23 - 1  # the largest |k| of the labels' fixed-point image


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


_cache = {}  # datasets and their oracle forests: computed once, shared by the parametrised cases


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _setenv(monkeypatch, rl=None, limit=None, **more):
    for name, v in dict(SBAG_HIST_RL=rl, SBAG_HIST_FLUSH_LIMIT=limit, **more).items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _fit(ctx, X, y, L, *, replacement, ratio, depth, part=None, cls=False):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        return nat.fit(ctx, ds, replacement=replacement, sample_ratio=ratio,
                       seed=SEED_CLS if cls else SEED_REG, learner_begin=0, learner_end=L,
                       partition_offsets=part, max_depth=depth, max_bins=32,
                       impurity=nat.IMPURITY_GINI if cls else nat.IMPURITY_VARIANCE)
    finally:
        ds.free()


def _oracle(X, y, L, *, replacement, ratio, depth, part=None, cls=False):
    N, F = X.shape
    seed = SEED_CLS if cls else SEED_REG
    counts = oracle.bag(replacement, ratio, 0, L, seed, part or [0, N], N)
    subs = [oracle.subspace(ratio, F, seed + i) for i in range(L)]
    return oracle_forest(X, y, counts, subs, depth, 32, cls, part=part), counts


def _forest_bytes(forest, L):
    return [tuple(a.tobytes() for a in forest.tree(t)) for t in range(L)]


# ------------------------------------------------- G1: limit-caused flush, variance
def _g1_data(name):
    rng = np.random.default_rng({"plain": 101, "dup": 102, "wide": 103}[name])
    N, F = (60_000, 100) if name == "wide" else (200_000, 8)
    X = rng.integers(0, 32, size=(N, F)).astype(np.float64)
    if name == "dup":  # exact ties between columns: the kHistSq plane's flush and re-zero
        X[:, 3] = X[:, 0]
        X[:, 6] = X[:, 0]
    y = (rng.integers(-2**14, 2**14, size=N) + 64 * X[:, 0]) / 4.0
    part = [0, 70_001, N] if N > 70_001 else [0, 7_001, N]
    orf, _ = _oracle(X, y, 4, replacement=True, ratio=1.0, depth=5, part=part)
    return X, y, part, orf


@pytest.mark.parametrize("limit", [None, "256"])
@pytest.mark.parametrize("rl", ["0", None])
@pytest.mark.parametrize("data", ["plain", "dup", "wide"])
def test_limit_flush_variance(ctx, monkeypatch, data, rl, limit):
    """200 000 rows x 4 learners on 512 workgroups: with the limit at 256 every workgroup
    flushes its node many times (store, then adds); cshift lands on the raised 32 instead of
    39.  k_hist (SBAG_HIST_RL=0) and k_hist_rl, duplicated columns (exact fallbacks: the
    squares plane), and 100 features (two lane groups / the row-lane tail tile).  Trees equal
    to the oracle and byte-identical across the four settings."""
    L, depth = 4, 5
    X, y, part, orf = _cached(("g1", data), lambda: _g1_data(data))
    _setenv(monkeypatch, rl=rl, limit=limit)
    forest = _fit(ctx, X, y, L, replacement=True, ratio=1.0, depth=depth, part=part)
    t = forest.timing()
    assert t["chain_ms"] == 0.0, t
    if data == "dup":
        assert t["exact_fallbacks"] > 0, t
    mid = t["hist_midrun_flushes"]
    if limit is None:
        assert mid == 0, t
    else:
        # Between two flushes of a run (one workgroup's consecutive pieces of one node) lie at
        # most 256 entries, so a run of n entries has at least n / 256 - 1 flushes that only the
        # limit explains.  A run starts with a workgroup (<= 512 per launch: two 512-thread
        # workgroups on each of 256 CUs) or with a node (<= L (2^(depth + 1) - 1) in all).
        bound = t["hist_entries"] / 256.0 - 512 * t["hist_launches"] - L * (2 ** (depth + 1) - 1)
        print(f"G1 {data} rl={rl}: hist_midrun_flushes {mid}, lower bound {bound:.0f}, "
              f"entries {t['hist_entries']:.0f}, launches {t['hist_launches']}")
        assert mid > 0 and mid >= bound, t
        if data == "plain":
            assert bound > 0, t  # (the shape makes the bound bite)
    assert_forest_equal(forest, orf)
    first = _cached(("g1 bytes", data), lambda: _forest_bytes(forest, L))
    assert _forest_bytes(forest, L) == first


def test_limit_knob_only_lowers(ctx, monkeypatch):
    """SBAG_HIST_FLUSH_LIMIT at or above the host's own choice changes nothing: 2^22 (and a
    value past it) give no limit-caused flush; a value below 256 is clamped to 256."""
    X, y, part, orf = _cached(("g1", "plain"), lambda: _g1_data("plain"))
    got = {}
    for limit in ["4194304", "1000000000000", "256", "1", "511"]:
        _setenv(monkeypatch, limit=limit)
        forest = _fit(ctx, X, y, 4, replacement=True, ratio=1.0, depth=5, part=part)
        got[limit] = forest.timing()["hist_midrun_flushes"]
        assert_forest_equal(forest, orf)
    assert got["4194304"] == 0 and got["1000000000000"] == 0, got
    assert got["256"] > 0 and got["1"] == got["256"] == got["511"], got


# ------------------------------------------------- G2: limit-caused flush, gini
def _g2_data(classes, L, replacement, ratio):
    N, F = 100_000, 20
    ds = nat.DeviceDataset.synthetic(N, F, seed=41 + classes, num_classes=classes)
    try:
        X, y = ds.features(), ds.labels()
    finally:
        ds.free()
    orf, _ = _oracle(X, y, L, replacement=replacement, ratio=ratio, depth=8, cls=True)
    return X, y, orf


@pytest.mark.parametrize("classes,L,replacement,ratio", [(7, 6, True, 1.0), (12, 48, True, 1.0),
                                                         (12, 48, False, 0.6)])
def test_limit_flush_gini(ctx, monkeypatch, classes, L, replacement, ratio):
    """Gini words are 32-bit counts; the limit at 256.  7 classes ungrouped; 12 classes in
    grouped tiles of 3 (class-tile-major layout and the zero plan, which leaves a tile that
    one workgroup stores unzeroed -- its second flush must add), with replacement and without
    (all-ones counts, k_tile_scatter_known under SBAG_TILE_CHECK=1).  At 20 features twelve
    class planes fit the default LDS budget and the row-lane kernel takes every feature, so
    neither tiles nor groups by itself (tests/test_gpu_parity.py::test_gini_tile_layouts gets
    its tiles of 3 from 60 features): SBAG_HIST_LDS_KB=29 makes the planes need tiles,
    SBAG_HIST_RL=0 leaves them to the grouped k_hist, and SBAG_HIST_GROUPED_LDS_KB=16 holds
    three 4352-byte planes (32 bins x 32 padded features + 64 dump words).
    The case that matters is a (node, tile) sub-segment that one workgroup owns and that is
    longer than 256 entries: its first flush stores, its second adds, and the host did not
    zero the tile.  A grouped launch spreads its pieces over 2048 workgroups and the levels
    below the root hold about a fifth of the root's entries, so it takes 48 learners (0.6 M
    entries per level, ~300 per workgroup) for a workgroup to hold such a sub-segment down to
    the deepest level: SBAG_LEVEL_TRACE then reports 20 to 100 limit flushes after a store on
    each of the levels 1 to 6, all under the zero plan; 18 learners gave none."""
    X, y, orf = _cached(("g2", classes, L, replacement),
                        lambda: _g2_data(classes, L, replacement, ratio))
    tiles = dict(SBAG_HIST_LDS_KB="29", SBAG_HIST_GROUPED_LDS_KB="16") if classes == 12 else {}
    _setenv(monkeypatch, rl="0" if classes == 12 else None, limit="256",
            SBAG_TILE_CHECK="1" if not replacement else None, **tiles)
    forest = _fit(ctx, X, y, L, replacement=replacement, ratio=ratio, depth=8, cls=True)
    t = forest.timing()
    print(f"G2 {classes} classes: hist_midrun_flushes {t['hist_midrun_flushes']}, launches "
          f"{t['hist_launches']}, entries {t['hist_entries']:.0f}, group_ms {t['group_ms']:.2f}")
    assert t["hist_midrun_flushes"] > 0, t
    if classes == 12:
        assert t["group_ms"] > 0.0, t  # the grouped class tiles ran
    assert_forest_equal(forest, orf)
    _setenv(monkeypatch, rl="0" if classes == 12 else None, limit=None, **tiles)
    plain = _fit(ctx, X, y, L, replacement=replacement, ratio=ratio, depth=8, cls=True)
    assert plain.timing()["hist_midrun_flushes"] == 0
    assert _forest_bytes(plain, L) == _forest_bytes(forest, L)


# ------------------------------------------------- G3: the whole label range, integer engine
def _g3_labels(name, rng, N):
    if name in ("full", "full_shift40"):
        k = rng.integers(-KMAX, KMAX + 1, size=N)
        k[3], k[N - 2] = -KMAX, KMAX
    elif name in ("high", "low"):
        k = rng.integers(KMAX - 1000, KMAX + 1, size=N)
        k[3], k[N - 2] = KMAX - 1000, KMAX
        if name == "low":
            k = -k
    else:  # "ends"
        k = np.where(rng.random(N) < 0.5, -KMAX, KMAX)
        k[3], k[N - 2] = -KMAX, KMAX
    return np.ldexp(k.astype(np.float64), -40 if name == "full_shift40" else 0)


@pytest.mark.parametrize("limit", [None, "256"])
@pytest.mark.parametrize("labels", ["full", "full_shift40", "high", "low", "ends"])
def test_whole_label_range_integer_engine(ctx, monkeypatch, labels, limit):
    """100 rows, every count 1 (without replacement at ratio 1), so N cmax kabs^2 < 2^53 for
    any |k| < 2^23: the integer engine takes k over the full +-(2^23 - 1) (kspan = 2^24 - 1,
    both at shift 0 and as k 2^-40), one-sided ranges at either end (K0 far from zero, tiny
    kspan) and the two ends alone."""
    N, F, L = 100, 3, 2
    rng = np.random.default_rng(7)
    X = rng.integers(0, 6, size=(N, F)).astype(np.float64)
    y = _g3_labels(labels, rng, N)
    assert N * KMAX**2 < 2**53 and np.abs(y).max() * (2.0**40 if labels == "full_shift40" else 1) == KMAX
    _setenv(monkeypatch, limit=limit)
    forest = _fit(ctx, X, y, L, replacement=False, ratio=1.0, depth=4)
    orf, counts = _oracle(X, y, L, replacement=False, ratio=1.0, depth=4)
    assert counts.max() == 1
    t = forest.timing()
    assert t["chain_ms"] == 0.0 and t["hist_midrun_flushes"] == 0, t
    assert len(forest.tree(0)[0]) > 1
    assert_forest_equal(forest, orf)


# ------------------------------------------------- G4: the hand-over at 2^53, from both sides
@pytest.mark.parametrize("side", ["inside", "outside"])
@pytest.mark.parametrize("P", [1, 2])
def test_handover_at_2_53(ctx, P, side):
    """N cmax kin^2 < 2^53 <= N cmax (kin + 1)^2: labels in [-kin, kin] stay on the integer
    engine, one label of kin + 1 hands the fit to the fp64 engine; both equal the oracle."""
    N, F, L = 5000, 4, 3
    part = [0, N] if P == 1 else [0, 1801, N]
    rng = np.random.default_rng(19)
    X = rng.integers(0, 32, size=(N, F)).astype(np.float64)
    cmax = int(oracle.bag(True, 1.0, 0, L, SEED_REG, part, N).max())
    kin = math.isqrt((2**53 - 1) // (N * cmax))
    assert N * cmax * kin**2 < 2**53 <= N * cmax * (kin + 1) ** 2
    k = rng.integers(-kin, kin + 1, size=N)
    k[5], k[N - 7] = -kin, kin
    if side == "outside":
        k[N // 2] = kin + 1
    y = k.astype(np.float64)
    forest = _fit(ctx, X, y, L, replacement=True, ratio=1.0, depth=5, part=part)
    orf, counts = _oracle(X, y, L, replacement=True, ratio=1.0, depth=5, part=part)
    assert counts.max() == cmax
    t = forest.timing()
    assert len(forest.tree(0)[0]) > 1
    if side == "inside":
        assert t["chain_ms"] == 0.0, t
    else:
        assert t["chain_ms"] > 0.0, t
    assert_forest_equal(forest, orf)


# ------------------------------------------------- G5: draw counts up to 255
def _g5_data(kind):
    N, F = 20_000, 6
    rng = np.random.default_rng(23)
    X = rng.integers(0, 32, size=(N, F)).astype(np.float64)
    if kind == "all255":
        counts = np.full(N, 255, np.uint8)
    else:
        counts = rng.integers(0, 256, size=N).astype(np.uint8)
        counts[:50], counts[50] = 0, 255
    kin = math.isqrt((2**53 - 1) // (N * 255))
    assert N * 255 * kin**2 < 2**53 <= N * 255 * (kin + 1) ** 2
    k = rng.integers(-kin, kin + 1, size=N) // 2 + (X[:, 1] * (kin // 64)).astype(np.int64)
    k[60], k[N - 9] = -kin, kin
    assert np.abs(k).max() == kin and counts[60] > 0 and counts[N - 9] > 0
    y = k.astype(np.float64)
    sub = np.arange(F, dtype=np.int32)
    orf = oracle.fit(X, y, counts[None, :], [sub], max_depth=6, max_bins=32)
    return X, y, counts, sub, orf


@pytest.mark.parametrize("limit", [None, "256"])
@pytest.mark.parametrize("rl", ["0", None])
@pytest.mark.parametrize("kind", ["all255", "mixed"])
def test_counts_up_to_255(ctx, monkeypatch, kind, rl, limit):
    """A booster's counts are the caller's bytes: all 255, and 0..255 with zeros.  The labels
    sit at the 2^53 rule for cmax = 255, so count x label fills the word's low field and the
    squares plane as far as the integer engine lets them."""
    X, y, counts, sub, orf = _cached(("g5", kind), lambda: _g5_data(kind))
    _setenv(monkeypatch, rl=rl, limit=limit)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx)
    try:
        f = nat.fit_booster(ctx, ds, y, counts, sub, max_depth=6, max_bins=32)
    finally:
        ds.free()
    t = f.timing()
    assert t["chain_ms"] == 0.0, t
    if limit is None:
        assert t["hist_midrun_flushes"] == 0, t
    assert len(f.tree(0)[0]) > 1
    assert_tree_equal(f, 0, orf, 0)


# ------------------------------------------------- G6: k_hist_mfma at its int32 bound
MF_N = 2 * 65536 + 32  # two whole 65536-row slices and a short third; divisible by 16


def _g6_data(digits):
    rng = np.random.default_rng(29)
    N = MF_N
    X = np.stack([np.zeros(N, np.int64), rng.integers(0, 32, size=N), rng.integers(0, 17, size=N)],
                 axis=1).astype(np.float64)  # column 0 constant: one bin sums a whole slice
    k = (3 * X[:, 1] - 2 * X[:, 2] + rng.integers(-4, 5, size=N)).astype(np.int64)
    k[N - 1], k[N - 2] = -300, 300  # the range: kmid = 0, K0 = 300, two digit planes either way
    kmin, kmax = -300, 300
    s0, s1 = np.arange(65536), np.arange(65536, 131072)
    if digits == "8":
        # balanced base-256 digits of k - kmid (k_label_digits): the low digit is -128 at
        # k = -128 and 127 at k = 127.  (A lone balanced digit never is -128: the host centres
        # the range on kmid = kmin + (kmax - kmin) / 2, so one digit spans at most [-127, 127]
        # or [-127, 128] -> two digits; the low one of two reaches -128.)
        k[rng.choice(s0, size=int(0.5 * 65536), replace=False)] = -128
        k[rng.choice(s1, size=int(0.5 * 65536), replace=False)] = 127
        v = k - (kmin + (kmax - kmin) // 2)
        d0 = (v + 128) % 256 - 128
        assert (d0[s0] == -128).mean() >= 0.4 and (d0[s1] == 127).mean() >= 0.4
    else:
        # unsigned 7-bit digits of k + K0: the low digit is 127 at k = -45 (255 = 127 + 128)
        k[rng.choice(s0, size=int(0.5 * 65536), replace=False)] = -45
        k[rng.choice(s1, size=int(0.5 * 65536), replace=False)] = -45
        d0 = (k - kmin) & 127
        assert (d0[s0] == 127).mean() >= 0.4 and (d0[s1] == 127).mean() >= 0.4
    assert k.min() == kmin and k.max() == kmax
    y = k.astype(np.float64)
    sub = np.arange(3, dtype=np.int32)
    orfs = {c: oracle.fit(X, y, np.full((1, N), c, np.uint8), [sub], max_depth=4, max_bins=32)
            for c in (127, 128)}
    return X, y, sub, orfs


@pytest.mark.parametrize("digits", ["8", "7"])
def test_mfma_root_at_int32_bound(ctx, monkeypatch, digits):
    """Counts of 127 times a digit of -128 / +127 / 127 on half the rows of a 65536-row slice,
    all in one bin (a constant column): |sum| ~ 127 x 128 x 32768 in the slice's int32
    accumulator, the most a fit can put there.  Byte-identical to the LDS-atomic root and
    equal to the oracle; counts of 128 decline the MFMA root (cmax <= 127)."""
    X, y, sub, orfs = _cached(("g6", digits), lambda: _g6_data(digits))
    monkeypatch.setenv("SBAG_MFMA_DIGITS", digits)

    def fit(count, mfma):
        monkeypatch.setenv("SBAG_ROOT_MFMA", mfma)
        ds = nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx)
        try:
            return nat.fit_booster(ctx, ds, y, np.full(len(X), count, np.uint8), sub, max_depth=4,
                                   max_bins=32)
        finally:
            ds.free()

    a, b, c = fit(127, "1"), fit(127, "0"), fit(128, "1")
    ta, tb, tc = a.timing(), b.timing(), c.timing()
    assert ta["root_ms"] > 0.0 and ta["root_mfma_ops"] > 0.0, ta
    assert tb["root_ms"] == 0.0 and tc["root_ms"] == 0.0, (tb, tc)
    assert ta["chain_ms"] == 0.0 and tc["chain_ms"] == 0.0
    assert len(a.tree(0)[0]) > 1
    assert _forest_bytes(a, 1) == _forest_bytes(b, 1)
    assert_tree_equal(a, 0, orfs[127], 0)
    assert_tree_equal(c, 0, orfs[128], 0)


# ------------------------------------------------- G7: label magnitudes in the fuzz
# Seeds of scripts/fuzz_parity.py --labels (found on an MI355X among 70000..70229), each with
# at most 40 000 rows: (seed, fp64 engine, partitions); cshift is what hist_word_budget gives
# for the seed's label image and largest count
LABEL_SEEDS = [
    (70048, False, 2),  # cshift 32: k [-399, 517] at shift 21, counts of 1
    (70035, False, 6),  # cshift 32: k [462513, 463436] at shift 34: K0 far from zero, depth 14
    (70019, False, 5),  # cshift 41: k [-98816, 136192], counts to 7: the limit search halves twice
    (70066, False, 6),  # cshift 36: k near 152 000, counts to 7: N cmax kabs^2 = 2^51.2, 140 features
    (70163, True, 2),  # cshift 36: k near -3.6 M: past 2^53 at 3243 rows, depth 10
    (70219, True, 5),  # cshift 35: k near -1.8 M at shift 4, 8 learners
]


@pytest.mark.parametrize("seed,fp64,P", LABEL_SEEDS)
def test_label_magnitude_fuzz_seeds(ctx, seed, fp64, P):
    """fuzz_case_labels: fuzz_case's regression draws with the labels moved by up to 2^22 grid
    units and scaled by 2^-30 .. 2^12 (fuzz_case itself keeps |k| near 2^11).  Both engines,
    several partitions, cshift at 32 and above it."""
    X, y, cls, _, part, p, kind = fuzz_case_labels(seed)
    N, F = X.shape
    assert not cls and N <= 40_000 and len(part) - 1 == P
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        forest = nat.fit(ctx, ds, replacement=p["replacement"], sample_ratio=p["ratio"],
                         seed=SEED_REG, learner_begin=0, learner_end=p["L"],
                         partition_offsets=part, max_depth=p["depth"], max_bins=p["bins"],
                         min_instances_per_node=p["min_inst"], min_info_gain=p["min_gain"],
                         impurity=nat.IMPURITY_VARIANCE)
    finally:
        ds.free()
    counts = oracle.bag(p["replacement"], p["ratio"], 0, p["L"], SEED_REG, part, N)
    subs = [oracle.subspace(p["ratio"], F, SEED_REG + i) for i in range(p["L"])]
    orf = oracle_forest(X, y, counts, subs, p["depth"], p["bins"], False, p["min_inst"],
                        p["min_gain"], part=part)
    t = forest.timing()
    assert (t["chain_ms"] > 0.0) == fp64, t
    assert t["hist_midrun_flushes"] == 0, t
    assert_forest_equal(forest, orf)
