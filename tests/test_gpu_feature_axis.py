"""GPU: fits along the feature axis -- row-lane widths, feature tiles, wide rows.

The feature count selects code in the fit: k_hist_rl<MODE, K> is instantiated per K =
ceil(FT / 16) and runs when roundup(FT, 16) < roundup(FT, 64); more than 256 features (or a
histogram plane past the LDS target) are cut into feature tiles (blockIdx.y, ft0 > 0, a short
last tile); the split searches stride their features by 256 threads, so from 257 features on
one thread sees two; and the per-replica binning picks k_bin_ranked<., ., 4 | 8 | 16>,
k_bin_cuts or k_bin_cuts_rows (+ k_transpose) by the width of a code row.  The rest of the
suite stops at 256 features on the fit side, and parity_utils.fuzz_case draws F from a list
that ends at 140 (left as it is: the committed seeds depend on its stream), so the fuzz does
not reach these shapes either.

A fit-level comparison sees only the histogram of the feature that wins, so sections A and B
aim the label at a chosen target feature j (first / last byte of a lane, both sides of a tile
boundary, the last feature), one cheap fit per target, and require the ORACLE's root to split
on j and a deeper node on another feature.  Every comparison is bit for bit against the CPU
oracle, node stats included; every fitted forest's predictions (host rows and device dataset)
equal the oracle's tree walk.

Each case asserts where it went: sbag_timing's hist_lds_atomics / hist_entries is
ntf roundup(FT, 16) / 64 for the row lanes and ntf ceil(FT / 64) for k_hist (the host's own
bookkeeping), compared with a Python restatement of hist_geometry (_geometry, cross-checked
below against figures worked out by hand); SBAG_DEBUG_BINS names the binning kernel and the
origin of the column copy; root_mfma_ops, chain_ms, group_ms, exact_fallbacks and
hist_midrun_flushes tell the MFMA root, the fp64 engine, the grouped class tiles, the exact
fallback and the limit-caused flushes."""
import re

import numpy as np
import pytest

import oracle
from parity_utils import assert_forest_equal, assert_tree_equal

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED_REG = oracle.DEFAULT_SEED_REGRESSOR
SEED_CLS = oracle.DEFAULT_SEED_CLASSIFIER
RL_K = (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15)  # the K of k_hist_rl that the planner can choose
KNOBS = ("SBAG_HIST_RL", "SBAG_HIST_FLUSH_LIMIT", "SBAG_ROOT_MFMA", "SBAG_TILE_CHECK",
         "SBAG_F64_SCREEN", "SBAG_DEBUG_BINS", "SBAG_HIST_LDS_KB", "SBAG_HIST_GROUPED_LDS_KB",
         "SBAG_OVERLAP")


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


_cache = {}  # datasets and their oracle forests: computed once, shared by the parametrised cases


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _setenv(monkeypatch, **knobs):
    for name in KNOBS:
        if knobs.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, knobs[name])


# ------------------------------------------------- hist_geometry, restated
def _roundup(x, a):
    return (x + a - 1) // a * a


def _plane(NB, FPH, gini):  # hist_plane_bytes
    return (NB * FPH + 64) * (4 if gini else 8)


_STAGE = 8 * 64 * 8  # hist_stage_bytes: 8 waves x 64 entries x 8 bytes
_HARD = 160 * 1024 - 256


def _geometry_one(Fmax, NB, NS, gini, rl_ok, grouped):
    align = 32 if gini else 16
    soft = (38 if grouped else 80) * 1024
    stage = 0 if grouped else _STAGE

    def lds_for(ft, ct):
        b = _plane(NB, _roundup(ft, align), gini) * (ct if gini else 1)
        return b + (stage if gini and ct < NS else 0)

    ft, ct = min(256, _roundup(Fmax, align)), NS if gini else 1
    while True:
        if not gini:
            if lds_for(ft, 1) <= soft or ft <= align:
                break
            ft -= align
            continue
        P = _plane(NB, _roundup(ft, align), True)
        if NS * P <= soft:
            ct = NS
            break
        c = (soft - stage) // P if soft > stage else 0
        if c >= 1:
            nct = -(-NS // c)
            ct = -(-NS // nct)
            break
        if ft <= align:
            ct = 1
            break
        ft -= align
    assert lds_for(ft, ct) <= _HARD
    FT = min(ft, Fmax)
    FPH = _roundup(FT, align)
    rl = (rl_ok and _roundup(FT, 16) < _roundup(FT, 64)
          and _plane(NB, FPH, gini) * (ct if gini else 1) + _STAGE <= _HARD)
    return dict(FT=FT, FPH=FPH, CT=ct, ntf=-(-Fmax // FT), rl=rl, grouped=False)


def _geometry(Fmax, NB, NS=1, gini=False, rl_ok=True):
    """hist_geometry + maybe_grouped (sbag_host.cpp) for Fmax features of NB bins and, for
    gini, NS classes; rl_ok: the rows are in subspace order (rl_mode_for).  per_entry is the
    launch's LDS atomic wave-instructions per entry as the host books them."""
    g = _geometry_one(Fmax, NB, NS, gini, rl_ok, False)
    if gini and g["CT"] < NS and not g["rl"]:
        gg = _geometry_one(Fmax, NB, NS, True, False, True)
        if gg["CT"] < NS:
            gg["grouped"] = True
            g = gg
    g["K"] = -(-g["FT"] // 16)
    g["tail"] = Fmax - (g["ntf"] - 1) * g["FT"]
    g["per_entry"] = g["ntf"] * (_roundup(g["FT"], 16) / 64.0 if g["rl"] else -(-g["FT"] // 64))
    return g


def test_geometry_restatement():
    """_geometry against figures worked out by hand from hist_geometry's rules."""
    g = _geometry(257, 32)
    assert (g["rl"], g["FT"], g["ntf"], g["tail"], g["per_entry"]) == (False, 256, 2, 1, 8)
    g = _geometry(300, 32)
    assert (g["rl"], g["FT"], g["ntf"], g["tail"], g["per_entry"]) == (False, 256, 2, 44, 8)
    g = _geometry(520, 32)
    assert (g["rl"], g["FT"], g["ntf"], g["tail"], g["per_entry"]) == (False, 256, 3, 8, 12)
    # 64 bins: (64 FT + 64) 8 <= 80 KB gives FT <= 159, in steps of 16: 144 = 9 x 16
    g = _geometry(200, 64)
    assert (g["rl"], g["K"], g["FT"], g["ntf"], g["tail"], g["per_entry"]) == (True, 9, 144, 2, 56, 4.5)
    g = _geometry(520, 64)
    assert (g["rl"], g["K"], g["FT"], g["ntf"], g["tail"], g["per_entry"]) == (True, 9, 144, 4, 88, 9.0)
    for K in range(1, 17):
        for F in (16 * K - 15, 16 * K):
            g = _geometry(F, 32)
            assert (g["FT"], g["ntf"], g["K"]) == (F, 1, K)
            assert g["rl"] == (K in RL_K)
            assert g["per_entry"] == (_roundup(F, 16) / 64.0 if K in RL_K else -(-F // 64))
    # gini, 32 bins: five planes of (32 x 96 + 64) 4 bytes fit 80 KB, of 128 features not
    assert _geometry(96, 32, 5, True)["CT"] == 5 and _geometry(97, 32, 5, True)["CT"] == 3
    assert _geometry(97, 32, 5, True)["rl"] and not _geometry(97, 32, 5, True)["grouped"]
    g = _geometry(128, 32, 5, True)
    assert (g["rl"], g["grouped"], g["CT"]) == (False, True, 2)
    g = _geometry(300, 32, 2, True)
    assert (g["rl"], g["grouped"], g["CT"], g["FT"], g["ntf"], g["per_entry"]) == (False, False, 2, 256, 2, 8)
    g = _geometry(300, 32, 5, True)
    assert (g["rl"], g["grouped"], g["CT"], g["FT"], g["ntf"], g["per_entry"]) == (False, True, 1, 256, 2, 8)
    # the value-count histogram (one u32 plane over the codes): 150 codes -> tiles of 128
    g = _geometry(300, 150, 1, True, rl_ok=False)
    assert (g["FT"], g["ntf"]) == (128, 3)


# ------------------------------------------------- shared pieces
def _per_entry(t):
    return t["hist_lds_atomics"] / t["hist_entries"]


def _forest_bytes(forest):
    return [tuple(a.tobytes() for a in forest.tree(t)) for t in range(len(forest))]


def _split_features(orf, t=None):
    """The features the oracle's internal nodes split on (of tree t, or of every tree)."""
    out = []
    for l in range(orf.nodes.shape[0]) if t is None else [t]:
        f = orf.tree(l)[0]["feature"]
        out.append(f[f >= 0])
    return np.concatenate(out)


def _root_features(orf):
    return [int(orf.tree(l)[0]["feature"][0]) for l in range(orf.nodes.shape[0])]


def _check_predict(ctx, forest, orf, X, ds, cls=False):
    agg = nat.AGG_MODE if cls else nat.AGG_MEAN
    want = oracle.predict(orf, X, classification=cls)
    np.testing.assert_array_equal(nat.predict(ctx, forest, X, agg), want)
    np.testing.assert_array_equal(nat.predict_dataset(ctx, forest, ds, agg), want)


def _full(F):
    return np.arange(F, dtype=np.int32)


def _levels(N, F, nlev, rng):
    """nlev-level integer columns (identity u8 codes), every level present in every column."""
    X = rng.integers(0, nlev, size=(N, F))
    X[:nlev, :] = np.arange(nlev)[:, None]
    return X.astype(np.float64)


def _aim(X, noise, j, j2=None):
    """A label whose best root split is on feature j and whose next-best is on j2: the root
    takes 3/4 of 16 var(x) against 3/4 of 9 var(x), its children 3/4 of 16 var(x) / 4 against
    3/4 of 9 var(x).  Dyadic (multiples of 1/8)."""
    y = 4.0 * X[:, j] + noise
    return y if j2 is None else y + 3.0 * X[:, j2]


def _booster_case(X, y, counts, depth, bins, j, other=True, **kw):
    """The oracle's tree for one aimed target, with the preconditions asserted on it."""
    orf = oracle.fit(X, y, counts[None, :], [_full(X.shape[1])], max_depth=depth, max_bins=bins, **kw)
    feats = _split_features(orf)
    assert _root_features(orf) == [j], (j, feats)
    if other:
        assert (feats != j).any(), (j, feats)
    return orf


def _fit_booster(ctx, ds, y, counts, F, depth, bins, **kw):
    return nat.fit_booster(ctx, ds, y, counts, _full(F), max_depth=depth, max_bins=bins, **kw)


def _zeros_ds(ctx, X):
    return nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx)


# ------------------------------------------------- A: every row-lane width
A_N = 3001
A_F = [f for K in range(1, 17) for f in (16 * K - 15, 16 * K)]


def _a_targets(F):
    K = -(-F // 16)
    return sorted({j for j in (0, K - 1, K, (F - 1) // K * K, F - 1, 63, 64) if 0 <= j < F})


def _a_other(F, j):
    return (j + F // 2) % F if F > 1 else None


def _a_data(F):
    rng = np.random.default_rng(1000 + F)
    X = _levels(A_N, F, 32, rng)
    noise = rng.integers(-8, 9, size=A_N) / 8.0
    counts = oracle.bag(True, 1.0, 0, 1, SEED_REG, [0, A_N], A_N)[0]
    cases = {}
    for j in _a_targets(F):
        y = _aim(X, noise, j, _a_other(F, j))
        cases[j] = (y, _booster_case(X, y, counts, 3, 32, j, other=F > 1))
    dup = None
    if F > 1:  # the last feature copied into a middle one: an exact tie at every node
        a = (F - 1) // 2
        Xd = X.copy()
        Xd[:, a] = Xd[:, F - 1]
        yd = _aim(Xd, noise, F - 1)
        od = _booster_case(Xd, yd, counts, 3, 32, a, other=False)
        assert (_split_features(od) != F - 1).all()  # the lower index wins everywhere
        dup = (Xd, yd, od)
    return X, counts, cases, dup


@pytest.mark.parametrize("F", A_F)
def test_row_lane_widths_variance(ctx, monkeypatch, F):
    """32-level features, one tile of F features, K = ceil(F / 16): F = 16 K - 15 leaves one
    feature in the last lane that holds any, F = 16 K fills every lane.  K in RL_K runs
    k_hist_rl<K>, K = 4, 8, 12, 16 hand over to k_hist's lane groups of 64.  Targets: the
    first lane's first and last byte, the second lane's first, the last lane's first and
    last, and both sides of k_hist's first lane-group boundary.  A duplicated column makes
    the screen flag a tie, so the exact fallback's kHistSq runs through the same K; for
    K = 6, 11, 15 the 64-bit row addresses (SBAG_HIST_RL=1) give the same bytes."""
    X, counts, cases, dup = _cached(("A", F), lambda: _a_data(F))
    K = -(-F // 16)
    g = _geometry(F, 32)
    assert g["rl"] == (K in RL_K) and g["ntf"] == 1
    _setenv(monkeypatch)
    ds = _zeros_ds(ctx, X)
    try:
        for j, (y, orf) in cases.items():
            f = _fit_booster(ctx, ds, y, counts, F, 3, 32)
            t = f.timing()
            assert _per_entry(t) == g["per_entry"], (j, t)
            assert t["chain_ms"] == 0.0, t
            assert_tree_equal(f, 0, orf, 0)
            _check_predict(ctx, f, orf, X, ds)
        if K in (6, 11, 15):
            j = F - 1
            y, orf = cases[j]
            auto = _fit_booster(ctx, ds, y, counts, F, 3, 32)
            _setenv(monkeypatch, SBAG_HIST_RL="1")
            wide = _fit_booster(ctx, ds, y, counts, F, 3, 32)
            _setenv(monkeypatch)
            assert _per_entry(wide.timing()) == g["per_entry"]
            assert _forest_bytes(wide) == _forest_bytes(auto)
            assert_tree_equal(wide, 0, orf, 0)
    finally:
        ds.free()
    if dup is not None:
        Xd, yd, od = dup
        ds = _zeros_ds(ctx, Xd)
        try:
            f = _fit_booster(ctx, ds, yd, counts, F, 3, 32)
            t = f.timing()
            assert t["exact_fallbacks"] > 0 and t["chain_ms"] == 0.0, t
            assert _per_entry(t) == g["per_entry"], t
            assert_tree_equal(f, 0, od, 0)
            _check_predict(ctx, f, od, Xd, ds)
        finally:
            ds.free()


def _gini_aim(X, rng, j, j2, C, half):
    """Classes 2 [x_j >= half] + [x_j2 >= half / 2], a tenth of the rows moved on by one class:
    the balanced cut on j is the best root split, the 1 : 3 cut on j2 the best below it."""
    y = 2 * (X[:, j] >= half) if j2 is None else 2 * (X[:, j] >= half) + (X[:, j2] >= half // 2)
    return ((y + (rng.random(len(X)) < 0.1)) % C).astype(np.float64)


def _gini_fit_case(X, y, L, depth, bins, *, replacement=True, ratio=1.0, roots=None):
    """(Every learner on every feature: the callers fit with subspace ratio 1.)"""
    N, F = X.shape
    counts = oracle.bag(replacement, ratio, 0, L, SEED_CLS, [0, N], N)
    subs = [_full(F)] * L
    orf = oracle.fit(X, y, counts, subs, max_depth=depth, max_bins=bins, classification=True)
    if roots is not None:
        assert _root_features(orf) == [roots] * L, _root_features(orf)
        assert F == 1 or (_split_features(orf) != roots).any()
    return orf


def _a_gini_data(F):
    rng = np.random.default_rng(2000 + F)
    X = _levels(A_N, F, 32, rng)
    K = -(-F // 16)
    cases = {}
    for j in sorted({j for j in (0, K, F - 1) if j < F}):
        y = _gini_aim(X, rng, j, _a_other(F, j), 5, 16)
        cases[j] = (y, _gini_fit_case(X, y, 2, 3, 32, roots=j))
    return X, cases


@pytest.mark.parametrize("F", A_F)
def test_row_lane_widths_gini(ctx, monkeypatch, F):
    """Five classes through the same widths, two learners: up to 96 features the five class
    planes are resident, from 97 on the row lanes stage class tiles per wave and k_hist groups
    its entries by class tile (group_ms)."""
    X, cases = _cached(("A gini", F), lambda: _a_gini_data(F))
    K = -(-F // 16)
    g = _geometry(F, 32, 5, True)
    assert g["rl"] == (K in RL_K) and g["ntf"] == 1 and (g["CT"] < 5) == (F >= 97)
    _setenv(monkeypatch)
    for j, (y, orf) in cases.items():
        ds = nat.DeviceDataset.from_numpy(X, y, ctx)
        try:
            f = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED_CLS, learner_begin=0,
                        learner_end=2, max_depth=3, max_bins=32, impurity=nat.IMPURITY_GINI)
            t = f.timing()
            assert _per_entry(t) == g["per_entry"], (j, t)
            assert (t["group_ms"] > 0.0) == g["grouped"], (j, t)
            assert_forest_equal(f, orf)
            _check_predict(ctx, f, orf, X, ds, cls=True)
        finally:
            ds.free()


# ------------------------------------------------- B: feature tiles
B_N = 4096 + 37


def _b_data(F, nlev, N=B_N):
    rng = np.random.default_rng(3000 + F + nlev)
    X = _levels(N, F, nlev, rng)
    noise = rng.integers(-8, 9, size=N) / 8.0
    g = _geometry(F, nlev)
    # both sides of every tile boundary and the last feature
    edges = sorted({t * g["FT"] + d for t in range(1, g["ntf"]) for d in (-1, 0)} | {F - 1})
    return X, noise, g, edges


def _b_forest_label(X, noise, edges):
    """Every edge feature carries signal, the later tiles the most."""
    y = noise.copy()
    for w, j in enumerate([0] + edges):
        y += (w + 1.0) * X[:, j]
    return y


def _b_var_case(F, nlev, ratio=1.0, L=3, depth=5, N=B_N):
    X, noise, g, edges = _b_data(F, nlev, N)
    y = _b_forest_label(X, noise, edges)
    counts = oracle.bag(True, ratio, 0, L, SEED_REG, [0, N], N)
    subs = [oracle.subspace(ratio, F, SEED_REG + i) for i in range(L)]
    orf = oracle.fit(X, y, counts, subs, max_depth=depth, max_bins=nlev)
    assert (_split_features(orf) >= g["FT"]).any()  # a later tile decides some split
    return X, y, noise, g, edges, orf, subs


def _fit_var(ctx, ds, L, depth, bins, ratio=1.0):
    return nat.fit(ctx, ds, replacement=True, sample_ratio=ratio, seed=SEED_REG, learner_begin=0,
                   learner_end=L, max_depth=depth, max_bins=bins)


@pytest.mark.parametrize("F,nlev,rl,ntf,tail,per_entry", [
    (257, 32, False, 2, 1, 8), (300, 32, False, 2, 44, 8), (520, 32, False, 3, 8, 12),
    (200, 64, True, 2, 56, 4.5), (520, 64, True, 4, 88, 9.0)])
def test_feature_tiles_variance(ctx, monkeypatch, F, nlev, rl, ntf, tail, per_entry):
    """More than one feature tile on the variance side: k_hist in tiles of 256 features with
    tails of 1, 44 and 8; 64-bin planes cut to 144 features, which the row lanes take at
    K = 9 in two and four tiles.  A three-learner forest whose label leans on every tile
    edge, then one aimed single-tree fit per edge feature."""
    X, y, noise, g, edges, orf, _ = _cached(("B", F, nlev), lambda: _b_var_case(F, nlev))
    assert (g["rl"], g["ntf"], g["tail"], g["per_entry"]) == (rl, ntf, tail, per_entry)
    assert (not rl and g["FT"] == 256) or (rl and g["FT"] == 144 and g["K"] == 9)
    _setenv(monkeypatch)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = _fit_var(ctx, ds, 3, 5, nlev)
        t = f.timing()
        assert _per_entry(t) == per_entry and t["chain_ms"] == 0.0, t
        assert_forest_equal(f, orf)
        _check_predict(ctx, f, orf, X, ds)
        counts = oracle.bag(True, 1.0, 0, 1, SEED_REG, [0, B_N], B_N)[0]
        for j in edges:
            ya = _aim(X, noise, j, (j + F // 2) % F)
            oa = _cached(("B aim", F, nlev, j), lambda: _booster_case(X, ya, counts, 4, nlev, j))
            fa = _fit_booster(ctx, ds, ya, counts, F, 4, nlev)
            assert _per_entry(fa.timing()) == per_entry, (j, fa.timing())
            assert_tree_equal(fa, 0, oa, 0)
            _check_predict(ctx, fa, oa, X, ds)
    finally:
        ds.free()


def test_feature_tiles_subspaces(ctx, monkeypatch):
    """520 features at sample ratio 0.7: under subspace_bug_compat each learner takes about
    364 of them, so the rows are read through A.pos across two tiles of k_hist (a gather is
    no row-lane layout)."""
    F, L = 520, 3
    X, y, _, _, _, orf, subs = _cached(("B sub",), lambda: _b_var_case(F, 32, ratio=0.7))
    Fmax = max(len(s) for s in subs)
    assert 300 < Fmax < 420 and all(len(s) < F for s in subs)
    g = _geometry(Fmax, 32, rl_ok=False)
    assert (g["FT"], g["ntf"], g["per_entry"]) == (256, 2, 8)
    # a split on a feature that sits in the second tile of its learner's subspace
    assert any(int(np.searchsorted(subs[l], j)) >= 256 for l in range(L) for j in _split_features(orf, l))
    _setenv(monkeypatch)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = _fit_var(ctx, ds, L, 5, 32, ratio=0.7)
        assert _per_entry(f.timing()) == 8, f.timing()
        assert_forest_equal(f, orf)
        _check_predict(ctx, f, orf, X, ds)
    finally:
        ds.free()


def _b_gini_case(C, replacement):
    F = 300
    rng = np.random.default_rng(3500 + C)
    X = _levels(B_N, F, 32, rng)
    # classes from the features on both sides of the tile boundary and the last one
    s = 4 * X[:, 255] + 3 * X[:, 256] + 2 * X[:, 299] + X[:, 0] + rng.integers(0, 24, size=B_N)
    y = np.minimum((s * C) // (s.max() + 1), C - 1).astype(np.float64)
    assert len(np.unique(y)) == C
    ratio = 1.0 if replacement else 0.7
    orf = _gini_fit_case(X, y, 3, 5, 32, replacement=replacement, ratio=ratio)
    return X, y, ratio, orf


@pytest.mark.parametrize("C,replacement", [(2, True), (5, True), (5, False)])
def test_feature_tiles_gini(ctx, monkeypatch, C, replacement):
    """300 features in two feature tiles of k_hist: two classes with both planes resident
    (ungrouped), five classes in grouped class tiles x feature tiles (blockIdx.y = class
    tile x ntf + feature tile); without replacement the tile scatter's known cursors are
    checked (SBAG_TILE_CHECK=1)."""
    X, y, ratio, orf = _cached(("B gini", C, replacement), lambda: _b_gini_case(C, replacement))
    g = _geometry(300, 32, C, True)
    assert (g["rl"], g["grouped"], g["FT"], g["ntf"]) == (False, C == 5, 256, 2)
    assert (_split_features(orf) >= 256).any()
    _setenv(monkeypatch, SBAG_TILE_CHECK=None if replacement else "1")
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = nat.fit(ctx, ds, replacement=replacement, sample_ratio=ratio, seed=SEED_CLS, learner_begin=0,
                    learner_end=3, subspace_ratio=1.0, subspace_bug_compat=False, max_depth=5, max_bins=32,
                    impurity=nat.IMPURITY_GINI)
        t = f.timing()
        assert _per_entry(t) == g["per_entry"], t
        assert (t["group_ms"] > 0.0) == (C == 5), t
        assert_forest_equal(f, orf)
        _check_predict(ctx, f, orf, X, ds, cls=True)
    finally:
        ds.free()


def test_feature_tiles_mfma_root(ctx, monkeypatch):
    """The int8 MFMA root over 300 features: 38 groups of 8 features, the last of 4.  It
    wants a row count divisible by 16 (4096 + 48 here).  Forest bytes equal to the LDS-atomic
    root's, both equal to the oracle; the levels below run k_hist in two tiles either way."""
    N = 4096 + 48
    X, y, _, g, _, orf, _ = _cached(("B mfma",), lambda: _b_var_case(300, 32, N=N))
    assert g["per_entry"] == 8
    got = {}
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        for mfma in ("1", "0"):
            _setenv(monkeypatch, SBAG_ROOT_MFMA=mfma)
            f = _fit_var(ctx, ds, 3, 5, 32)
            t = f.timing()
            assert (t["root_mfma_ops"] > 0.0) == (mfma == "1") and (t["root_ms"] > 0.0) == (mfma == "1"), t
            assert _per_entry(t) == 8 and t["chain_ms"] == 0.0, t
            assert_forest_equal(f, orf)
            _check_predict(ctx, f, orf, X, ds)
            got[mfma] = (_forest_bytes(f), t["hist_entries"])
    finally:
        ds.free()
    assert got["1"][0] == got["0"][0]
    assert got["1"][1] < got["0"][1]  # the root's entries went through the MFMA kernel


def test_feature_tiles_limit_flush(ctx, monkeypatch):
    """SBAG_HIST_FLUSH_LIMIT=256 at 300 features: a workgroup that holds more than 256
    entries of a node flushes in mid-run -- a store, then adds -- in both feature tiles.
    A workgroup gets a second piece of a node only when the launch has more than 512 pieces
    of up to 256 entries, so this case takes 64 learners (about 167 000 in-bag entries in
    pieces of 192)."""
    L, F = 64, 300
    X, y, _, g, _, _, _ = _cached(("B", F, 32), lambda: _b_var_case(F, 32))
    counts = oracle.bag(True, 1.0, 0, L, SEED_REG, [0, B_N], B_N)
    orf = _cached(("B limit",), lambda: oracle.fit(X, y, counts, [_full(F)] * L, max_depth=4, max_bins=32))
    assert (counts > 0).sum() > 512 * 256
    got = {}
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        for limit in ("256", None):
            _setenv(monkeypatch, SBAG_HIST_FLUSH_LIMIT=limit, SBAG_OVERLAP="0")
            f = _fit_var(ctx, ds, L, 4, 32)
            t = f.timing()
            print(f"B limit {limit}: hist_midrun_flushes {t['hist_midrun_flushes']}, launches {t['hist_launches']}")
            assert (t["hist_midrun_flushes"] > 0) == (limit is not None), t
            assert _per_entry(t) == 8, t
            assert_forest_equal(f, orf)
            got[limit] = _forest_bytes(f)
    finally:
        ds.free()
    assert got["256"] == got[None]


# ------------------------------------------------- C: the split search past 256 features
C_N, C_F = 4096, 300
# (lower, higher) copies: 7 / 263 meet in one thread of the 256-thread search (fl and fl + 256),
# 34 / 291 in two threads of which one is on its second feature, 270 / 299 both past 256
C_PAIRS = [(7, 263), (34, 291), (270, 299)]


def _c_data():
    rng = np.random.default_rng(4000)
    X = _levels(C_N, C_F, 32, rng)
    for lo, hi in C_PAIRS:
        X[:, hi] = X[:, lo]
    noise = rng.integers(-8, 9, size=C_N) / 8.0
    s = 4.0 * X[:, 7] + 3.0 * X[:, 34] + 2.0 * X[:, 270]
    return X, s, noise, rng


def _c_check_ties(orf):
    feats = _split_features(orf)
    assert set(_root_features(orf)) == {7}
    assert {7, 34, 270} <= set(feats.tolist())  # each kind of tie decides some node
    assert not {263, 291, 299} & set(feats.tolist())  # and the lower index wins it
    assert (feats >= 256).any()


def _c_var_case(real):
    X, s, noise, _ = _cached(("C data",), _c_data)
    y = s + noise
    if real:
        y = y * 1.1 + 0.3
    counts = oracle.bag(True, 1.0, 0, 3, SEED_REG, [0, C_N], C_N)
    orf = oracle.fit(X, y, counts, [_full(C_F)] * 3, max_depth=4, max_bins=32)
    _c_check_ties(orf)
    return X, y, counts, orf


@pytest.mark.parametrize("labels,screen", [("dyadic", None), ("real", None), ("real", "0")])
def test_split_search_past_256_variance(ctx, monkeypatch, labels, screen):
    """300 features with three exactly tied pairs, the best splits at the root and below:
    k_split_screen and the exact k_split fallback on dyadic labels, k_f64_screen on labels
    x 1.1 + 0.3, and with SBAG_F64_SCREEN=0 every feature of every node summed in fp64."""
    X, y, _, orf = _cached(("C var", labels), lambda: _c_var_case(labels == "real"))
    _setenv(monkeypatch, SBAG_F64_SCREEN=screen)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = _fit_var(ctx, ds, 3, 4, 32)
        t = f.timing()
        assert _per_entry(t) == 8, t
        if labels == "dyadic":
            assert t["exact_fallbacks"] > 0 and t["chain_ms"] == 0.0, t
        else:
            assert t["chain_ms"] > 0.0, t
        assert_forest_equal(f, orf)
        _check_predict(ctx, f, orf, X, ds)
    finally:
        ds.free()


def _c_gini_case(C):
    X, s, _, _ = _cached(("C data",), _c_data)
    rng = np.random.default_rng(4100 + C)
    v = s + rng.integers(0, 24, size=C_N)
    y = np.minimum((v * C) // (v.max() + 1), C - 1).astype(np.float64)
    assert len(np.unique(y)) == C
    orf = _gini_fit_case(X, y, 3, 4, 32)
    _c_check_ties(orf)
    return X, y, orf


@pytest.mark.parametrize("C", [2, 5])
def test_split_search_past_256_gini(ctx, monkeypatch, C):
    """The same ties through k_split_gini's feature groups and its running threshold."""
    X, y, orf = _cached(("C gini", C), lambda: _c_gini_case(C))
    _setenv(monkeypatch)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        f = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED_CLS, learner_begin=0,
                    learner_end=3, max_depth=4, max_bins=32, impurity=nat.IMPURITY_GINI)
        assert _per_entry(f.timing()) == 8, f.timing()
        assert_forest_equal(f, orf)
        _check_predict(ctx, f, orf, X, ds, cls=True)
    finally:
        ds.free()


@pytest.mark.parametrize("kind", ["dyadic", "real", "gini"])
def test_min_info_gain_at_the_tied_gain(ctx, monkeypatch, kind):
    """min_info_gain at the tied root gain keeps the split (Spark rejects gain < minInfoGain),
    one ulp above it leaves a single leaf: the engine decides as the oracle does."""
    cls = kind == "gini"
    if cls:
        X, y, _ = _cached(("C gini", 5), lambda: _c_gini_case(5))
        counts = oracle.bag(True, 1.0, 0, 1, SEED_CLS, [0, C_N], C_N)[0]
    else:
        X, y, counts3, _ = _cached(("C var", kind), lambda: _c_var_case(kind == "real"))
        counts = counts3[0]
    kw = dict(max_depth=4, max_bins=32, classification=cls)
    free = oracle.fit(X, y, counts[None, :], [_full(C_F)], **kw)
    gain = float(free.tree(0)[0]["gain"][0])
    assert _root_features(free) == [7] and gain > 0.0
    _setenv(monkeypatch)
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        for mg, split in ((gain, True), (np.nextafter(gain, np.inf), False), (np.nextafter(gain, 0.0), True)):
            orf = oracle.fit(X, y, counts[None, :], [_full(C_F)], min_info_gain=mg, **kw)
            assert (len(orf.tree(0)[0]) > 1) == split
            if cls:
                f = nat.fit_bag(ctx, ds, counts, _full(C_F), impurity=nat.IMPURITY_GINI, max_depth=4,
                                max_bins=32, min_info_gain=mg)
            else:
                f = nat.fit_booster(ctx, ds, y, counts, _full(C_F), max_depth=4, max_bins=32, min_info_gain=mg)
            if split:  # (a fit that ends at its root records no chain time on either engine)
                assert (f.timing()["chain_ms"] > 0.0) == (kind == "real")
            assert_tree_equal(f, 0, orf, 0)
    finally:
        ds.free()


# ------------------------------------------------- D: per-replica bins by row width
D_N = 6000  # below max(maxBins^2, 10 000): thresholds from the whole subbag's value counts


def _d_data(F, nval, real=False, C=0):
    """Continuous columns of about nval distinct values each (multiples of 1/8): more than
    maxBins, so every replica's bag has thresholds of its own; u8 codes up to 256 values per
    column, u16 above."""
    rng = np.random.default_rng(5000 + F + nval)
    X = rng.integers(0, nval, size=(D_N, F)) / 8.0
    distinct = [len(np.unique(X[:, f])) for f in range(F)]
    assert 32 < min(distinct) and (max(distinct) <= 256 if nval <= 256 else min(distinct) > 256)
    feats = sorted({0, min(255, F - 2), min(256, F - 2) if F > 257 else F // 2, F - 1})
    s = sum((w + 1.0) * X[:, j] for w, j in enumerate(feats))
    if C:
        v = s + rng.integers(0, max(1, nval // 16), size=D_N) / 8.0
        y = np.minimum(np.floor(v * C / (v.max() + 1)), C - 1)
        assert len(np.unique(y)) == C
    else:
        y = s + rng.integers(-8, 9, size=D_N) / 8.0
        if real:
            y = y * 1.1 + 0.3
    return X, y.astype(np.float64), feats


def _d_case(F, nval, real, C, replacement):
    X, y, feats = _d_data(F, nval, real, C)
    L, seed = 2, SEED_CLS if C else SEED_REG
    counts = oracle.bag(replacement, 1.0, 0, L, seed, [0, D_N], D_N)
    orf = oracle.fit(X, y, counts, [_full(F)] * L, max_depth=4, max_bins=32, classification=C > 0)
    used = set(_split_features(orf).tolist())
    assert set(feats[1:]) <= used, used  # both sides of index 256 (or the middle) and the last feature
    return X, y, orf


D_CASES = [
    # F, values per column, code bytes, real labels, classes, replacement, path, cols, per_entry
    (100, 150, 1, False, 0, True, "ranked<4>", "binning", 1.75),
    (300, 150, 1, False, 0, True, "ranked<8>", "binning", 8),
    (520, 150, 1, False, 0, True, "ranked<16>", "binning", 12),
    (120, 2000, 2, False, 0, True, "ranked<4>", "binning", 2),
    (200, 2000, 2, False, 0, True, "ranked<8>", "binning", 3.25),
    (300, 2000, 2, False, 0, True, "ranked<16>", "binning", 8),
    (520, 2000, 2, False, 0, True, "rows", "transpose", 12),
    (120, 2000, 2, True, 0, True, "cuts", "binning", 2),
    (300, 2000, 2, True, 0, True, "rows", "transpose", 8),
    (300, 2000, 2, False, 0, False, "shared rows", "transpose", 8),
    (300, 2000, 2, False, 5, True, "ranked<16>", "binning", 8),
]


@pytest.mark.parametrize("F,nval,cb,real,C,replacement,path,cols,per_entry", D_CASES)
def test_per_replica_bins_by_row_width(ctx, monkeypatch, capfd, F, nval, cb, real, C, replacement, path, cols,
                                       per_entry):
    """The binning kernel goes by the bytes of a code row: k_bin_ranked with 4, 8 or 16
    16-byte pieces per thread up to 256 / 512 / 1024 bytes (integer labels: only in-bag rows,
    by rank); past 1024 bytes every row is binned, and since k_bin_cuts stages rows of up to
    256 bytes only, by k_bin_cuts_rows with the column copy from a per-replica k_transpose;
    the fp64 engine bins every row (k_bin_cuts, then the rows fallback); without replacement
    at ratio 1 the replicas share one bins matrix.  Two learners, depth 4."""
    X, y, orf = _cached(("D", F, nval, real, C, replacement), lambda: _d_case(F, nval, real, C, replacement))
    S = _roundup(F, 16) if F <= 64 else _roundup(F, 128)
    m = re.fullmatch(r"ranked<(\d+)>", path)
    if m:  # the instance follows from the row bytes
        assert int(m.group(1)) == (4 if S * cb <= 256 else 8 if S * cb <= 512 else 16) and S * cb <= 1024
    else:
        assert real or not replacement or S * cb > 1024
        assert (path == "cuts") == (S * cb <= 256)
    _setenv(monkeypatch, SBAG_DEBUG_BINS="1")
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    try:
        lay = ds.layout()
        assert lay[:4] == (D_N, F, S, cb), lay
        capfd.readouterr()
        f = nat.fit(ctx, ds, replacement=replacement, sample_ratio=1.0, seed=SEED_CLS if C else SEED_REG,
                    learner_begin=0, learner_end=2, max_depth=4, max_bins=32,
                    impurity=nat.IMPURITY_GINI if C else nat.IMPURITY_VARIANCE)
        err = capfd.readouterr().err
        t = f.timing()
        print(f"D F={F} cb={cb}: {[l for l in err.splitlines() if 'bins' in l or 'cut table' in l]} "
              f"per entry {_per_entry(t)} valuecount_ms {t['valuecount_ms']:.3f}")
        assert f"[sbag] bins: path {path} cols {cols} replicas {2 if replacement else 1}\n" in err, err
        assert ("shared 1" in err) == (not replacement), err
        assert (t["chain_ms"] > 0.0) == real, t
        assert t["valuecount_ms"] > 0.0, t
        if (F, cb) == (300, 1):  # the value counts of u8 codes: an LDS histogram over the codes
            ncmax = max(len(np.unique(X[:, j])) for j in range(F))
            assert _geometry(F, ncmax, 1, True, rl_ok=False)["ntf"] == 3
        assert _per_entry(t) == per_entry, t
        if C:
            assert t["group_ms"] > 0.0, t  # class tiles x feature tiles
        assert_forest_equal(f, orf)
        _setenv(monkeypatch)
        _check_predict(ctx, f, orf, X, ds, cls=C > 0)
    finally:
        ds.free()
