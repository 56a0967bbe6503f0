"""GPU: the transform kernels on hand-built forests (NativeForest.from_trees), at the limits
the host planner between them branches on -- no fit, a few thousand rows.

Every output here is defined bit for bit, so every assertion is assert_array_equal against
the NumPy walk of predict_ref.py (held to oracle.predict by test_predict_ref_host.py).
Each case goes through every entry point that applies:
  * nat.predict on host rows: k_quantize -> k_predict_tiled<u16>, or k_predict where
    plan_tiled refuses;
  * nat.predict(per_tree=True): always k_predict;
  * nat.predict_dataset on a DeviceDataset of the same rows (NaN rows left out: a dataset
    refuses NaN), u8 / u16 / u32 codes (u32: k_predict);
  * nat.predict_dataset_device: per-tree fp64 (vote_bytes 8), the in-order sum, and u8 / u16
    votes with the device mode over them.

The planner's limits are restated from its formulas, not as bare numbers:
  * predict_tiled_lds (sbag_kernels.hip:3706-3711): kPredRows * (S * code_bytes + 4)
    + chunk_bytes [+ nclasses * kPredRows * 2 in mode aggregation], rounded up to 16;
  * plan_tiled (sbag_host.cpp, its first lines): fixed = that with chunk_bytes = 0, lds_cap =
    160 KB - 512; refuse if fixed + 4096 > lds_cap; budget = min(64 KB, lds_cap - fixed) & ~15;
  * plan_tiled (its loop over the trees): a tree takes one 8-byte PNode per node and one
    8-byte leaf value per leaf, so a tree of n internal nodes (n + 1 leaves) takes
    (2n + 1) * 8 + (n + 1) * 8 = (3n + 2) * 8 bytes, and is refused above the budget;
  * plan_tiled (the same loop): a chunk is closed when the next tree would pass
    the budget.
So the largest comb the tiled kernel holds has (65536 / 8 - 2) / 3 = 2730 internal nodes,
not 4095: the 4095- and 4096-node combs the issue names both take the global walk, and the
cases below run them and the combs of 2730 / 2731 nodes that bracket the real edge."""
import numpy as np
import pytest
import torch

import predict_ref as ref

from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

K_PRED_ROWS = 512                  # sbag_kernels.hip:3703 kPredRows
LDS_CAP = 160 * 1024 - 512         # plan_tiled's lds_cap
K_LDS_MODE_CLASSES = 320           # sbag_internal.h:210 kLdsModeClasses


def tiled_budget(S, code_bytes, mode_classes=0):
    """plan_tiled's chunk budget for rows of S codes (None: it refuses, k_predict runs)."""
    fixed = K_PRED_ROWS * (S * code_bytes + 4) + mode_classes * K_PRED_ROWS * 2
    fixed = (fixed + 15) & ~15
    if fixed + 4096 > LDS_CAP:
        return None
    return min(64 * 1024, LDS_CAP - fixed) & ~15


def tree_bytes(n_internal):
    return (2 * n_internal + 1) * 8 + (n_internal + 1) * 8


def host_stride(F):
    return (F + 15) // 16 * 16     # sbag_predict's Sq (u16 codes of host rows)


def plan_chunks(sizes, budget):
    """plan_tiled's greedy chunking of trees of `sizes` bytes: [(t0, t1)]."""
    chunks, used = [], 0
    for t, b in enumerate(sizes):
        assert b <= budget
        if not chunks or used + b > budget:
            chunks.append([t, t])
            used = 0
        chunks[-1][1] = t + 1
        used += b
    return [tuple(c) for c in chunks]


BUDGET_1F = tiled_budget(host_stride(1), 2)            # one feature, host rows (u16 codes)
N_TILED = (BUDGET_1F // 8 - 2) // 3                    # largest comb the tiled kernel holds
assert tree_bytes(N_TILED) <= BUDGET_1F < tree_bytes(N_TILED + 1)
assert tiled_budget(16, 1) == BUDGET_1F                # a u8 dataset of <= 16 features: the same


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- forests
def _blank(n):
    a = np.zeros(n, nat.NODE_DTYPE)
    a["id"] = np.arange(n)
    a["left"] = a["right"] = a["feature"] = -1
    return a


def leaf(v):
    a = _blank(1)
    a["prediction"] = v
    return a


def stump(thr, lv, rv, feature=0):
    a = _blank(3)
    a["left"][0], a["right"][0], a["feature"][0], a["threshold"][0] = 1, 2, feature, thr
    a["prediction"][1], a["prediction"][2] = lv, rv
    return a


def comb(thr, leaves, feature=0, left_deep=False):
    """n = len(thr) internal nodes in one chain, pre-order ids.  Right-deep: node 2i has
    leaf 2i + 1 on the left and node 2i + 2 on the right; left-deep: node i has node i + 1
    on the left and leaf 2n - i on the right.  leaves[k] is the leaf internal node k hangs
    off the chain, leaves[n] the leaf at its end."""
    thr = np.asarray(thr, np.float64)
    n = len(thr)
    a = _blank(2 * n + 1)
    if left_deep:
        i = np.arange(n)
        a["left"][i], a["right"][i] = i + 1, 2 * n - i
        ids = np.concatenate([2 * n - i, [n]])
    else:
        i = 2 * np.arange(n)
        a["left"][i], a["right"][i] = i + 1, i + 2
        ids = np.concatenate([i + 1, [2 * n]])
    a["feature"][i] = feature
    a["threshold"][i] = thr
    a["prediction"][ids] = leaves
    return a


def n_internal(tree):
    return int((tree["left"] >= 0).sum())


# ---------------------------------------------------------------- the entry points
def _check_host(ctx, f, X, pt, gini):
    agg, want = (nat.AGG_MODE, ref.mode(pt)) if gini else (nat.AGG_MEAN, ref.mean(pt))
    np.testing.assert_array_equal(nat.predict(ctx, f, X, agg), want)
    out, got = nat.predict(ctx, f, X, agg, per_tree=True)
    np.testing.assert_array_equal(got, pt)
    np.testing.assert_array_equal(out, want)


def _check_dataset(ctx, f, X, pt, gini, code_bytes, votes=()):
    L, N = pt.shape
    agg, want = (nat.AGG_MODE, ref.mode(pt)) if gini else (nat.AGG_MEAN, ref.mean(pt))
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(N), ctx)
    try:
        assert ds.layout()[3] == code_bytes
        np.testing.assert_array_equal(nat.predict_dataset(ctx, f, ds, agg), want)
        d = torch.zeros((L, N), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        nat.predict_dataset_device(ctx, f, ds, nat.OUT_VOTES, 8, d.data_ptr())
        np.testing.assert_array_equal(d.cpu().numpy(), pt)
        if not gini:
            s = torch.zeros(N, dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            nat.predict_dataset_device(ctx, f, ds, nat.OUT_SUM, 0, s.data_ptr())
            np.testing.assert_array_equal(s.cpu().numpy(), ref.seq_sum(pt))
        for vb in votes:
            v = torch.zeros((L, N), dtype=torch.uint8 if vb == 1 else torch.int16, device=DEV)
            out = torch.zeros(N, dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            nat.predict_dataset_device(ctx, f, ds, nat.OUT_VOTES, vb, v.data_ptr())
            np.testing.assert_array_equal(v.cpu().numpy().astype(np.float64), pt)
            nat.aggregate_device(ctx, v.data_ptr(), vb, L, N, nat.AGG_MODE, L, int(pt.max()) + 1,
                                 out.data_ptr())
            np.testing.assert_array_equal(out.cpu().numpy(), want)
    finally:
        ds.free()


def code_width(X):
    d = max(len(np.unique(X[:, g])) for g in range(X.shape[1]))
    return 1 if d <= 256 else 2 if d <= 65536 else 4


def with_filler(X, distinct):
    """X with one more column of `distinct` values that no tree reads: it sets the code
    width of the dataset (build_dataset: the widest dictionary decides)."""
    assert X.shape[0] >= distinct
    return np.ascontiguousarray(np.column_stack([X, np.arange(X.shape[0]) % distinct]).astype(np.float64))


def check_all(ctx, trees, subs, X, *, gini=False, pt=None, widths=(), votes=()):
    """Host rows, and the device dataset of the rows without NaN at each code width in
    `widths` (1: X as it is, at most 256 distinct values a column; 2 / 4: X, or X with a
    filler column where X's own dictionaries are narrower)."""
    X = np.ascontiguousarray(X, np.float64)
    if pt is None:
        pt = ref.per_tree(trees, subs, X)
    f = nat.NativeForest.from_trees(trees, subs, nat.IMPURITY_GINI if gini else nat.IMPURITY_VARIANCE)
    try:
        _check_host(ctx, f, X, pt, gini)
        keep = ~np.isnan(X).any(axis=1)
        Xd, ptd = np.ascontiguousarray(X[keep]), np.ascontiguousarray(pt[:, keep])
        for w in widths:
            own = code_width(Xd)
            assert own <= w
            Xw = Xd if own == w else with_filler(Xd, 257 if w == 2 else 65537)
            _check_dataset(ctx, f, Xw, ptd, gini, w, votes)
    finally:
        f.free()


# ---------------------------------------------------------------- a. thresholds per feature
def _threshold_case(T, n_comb):
    """Combs of n_comb internal nodes on feature 0 whose thresholds are a shuffled partition
    of arange(T) (the last comb shorter); the rows are every threshold, every midpoint, both
    ends, +-inf and NaN.  Expected per tree by searchsorted: leaf k = #{thresholds < x}, the
    last leaf for NaN; leaf values are the leaf index plus a per-tree base."""
    perm = np.random.default_rng(T).permutation(T).astype(np.float64)
    X = np.concatenate([np.arange(T), np.arange(T - 1) + 0.5,
                        [-0.5, T + 1.0, np.inf, -np.inf, np.nan]])[:, None]
    trees, pt = [], []
    for t, a in enumerate(range(0, T, n_comb)):
        thr = np.sort(perm[a:a + n_comb])
        base = t * float(1 << 17)
        trees.append(comb(thr, base + np.arange(len(thr) + 1)))
        k = np.searchsorted(thr, X[:, 0], "left")
        k[np.isnan(X[:, 0])] = len(thr)
        pt.append(base + k)
    return trees, X, np.stack(pt)


@pytest.mark.parametrize("n_comb", [4095, N_TILED], ids=["comb4095_global", "comb_tiled"])
@pytest.mark.parametrize("T", [65535, 65536, 69615])
def test_threshold_count_across_u16(ctx, T, n_comb):
    """k_quantize's code of a host row is #{thresholds of the feature < x}, 0..T inclusive, in
    a u16: with T >= 65536 thresholds on one feature the codes of the rows above the 65535th
    threshold, and of NaN, wrapped modulo 65536 and those rows walked left.  sbag_predict
    now sends such a forest to the node walk.  Combs of 4095 nodes never reached the tiled
    kernel (98 296 bytes a tree); the combs of N_TILED nodes do, and showed the wrap: before
    the fix nat.predict differed from the reference on 3 rows at T = 65 536 (T + 1, +inf and
    NaN, whose code 65 536 became 0) and on 8 161 rows at T = 69 615 (every row above
    threshold 65 535), and on none in the other four cases."""
    trees, X, pt = _threshold_case(T, n_comb)
    assert len(trees) == -(-T // n_comb) and sum(n_internal(t) for t in trees) == T
    rows = np.r_[np.random.default_rng(1).integers(0, len(X), 300), np.arange(len(X) - 5, len(X))]
    np.testing.assert_array_equal(ref.per_tree(trees[-2:], [[0]] * 2, X[rows]), pt[-2:, rows])
    check_all(ctx, trees, [[0]] * len(trees), X, pt=pt)


# ---------------------------------------------------------------- b. chunk budget edges
def _edge_rows(n, N, distinct=None, seed=0):
    """One feature over a comb's thresholds arange(n): integers (equal to a threshold),
    halves, both ends."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(-4, 2 * n + 8, size=distinct or N) / 2.0
    vals[:4] = [-2.0, n + 1.0, 0.0, n - 1.0]
    return (vals if distinct is None else vals[rng.integers(0, distinct, N)])[:, None]


@pytest.mark.parametrize("n", [N_TILED, N_TILED + 1, 4095, 4096])
def test_single_comb_at_the_chunk_budget(ctx, n):
    """One comb: N_TILED nodes fill the chunk to the byte, one more goes to the global walk
    (as do the 4095 and 4096 nodes the issue names)."""
    if n == N_TILED:
        assert tree_bytes(n) == BUDGET_1F
    t = comb(np.arange(n), np.arange(n + 1))
    check_all(ctx, [t], [[0]], _edge_rows(n, 1500), widths=(2,))
    check_all(ctx, [t], [[0]], _edge_rows(n, 1500, distinct=256), widths=(1,))


@pytest.mark.parametrize("delta", [0, -8, 8], ids=["exact", "under8", "over8"])
def test_chunks_filled_to_the_budget(ctx, delta):
    """Consecutive trees that sum to the budget, to 8 bytes under and to 8 bytes over it,
    three such groups in a row; every group begins with a single-leaf tree and ends with
    one.  Every leaf of the forest holds its own index, so a tree read at a wrong chunk
    offset cannot give the right number."""
    B = BUDGET_1F
    small = {0: ["leaf", "comb", "stump", "leaf"], -8: ["leaf", "comb", "stump", "leaf", "leaf"],
             8: ["leaf", "comb", "leaf"]}[delta]
    rest = sum(tree_bytes({"leaf": 0, "stump": 1}[k]) for k in small if k != "comb")
    n = (B + delta - rest - 16) // 24  # tree_bytes(n) = 24 n + 16
    assert rest + tree_bytes(n) == B + delta
    trees, nxt = [], 0
    for _ in range(3):
        for k in small:
            m = {"leaf": 0, "stump": 1, "comb": n}[k]
            thr = np.arange(m) if k == "comb" else np.array([n / 2 + 0.25] * m)
            trees.append(comb(thr, nxt + np.arange(m + 1)))
            nxt += m + 1
    chunks = plan_chunks([tree_bytes(n_internal(t)) for t in trees], B)
    if delta <= 0:  # a group is a chunk: it begins and ends with a single-leaf tree
        assert chunks == [(i * len(small), (i + 1) * len(small)) for i in range(3)]
        assert all(len(trees[a]) == 1 and len(trees[b - 1]) == 1 for a, b in chunks)
    else:           # the group's last leaf opens the next chunk; one chunk is two lone leaves
        assert chunks == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)]
        assert [len(trees[i]) for i in (2, 3)] == [1, 1] and len(trees[8]) == 1
    subs = [[0]] * len(trees)
    check_all(ctx, trees, subs, _edge_rows(n, 1500, seed=1), widths=(2,))
    check_all(ctx, trees, subs, _edge_rows(n, 1500, distinct=256, seed=1), widths=(1,))


# ---------------------------------------------------------------- c. two walks per thread
_UNEVEN = {}


def _uneven_forest(depth):
    if depth not in _UNEVEN:
        trees, nxt = [], 0
        for n in (30, depth):
            for left_deep in (False, True):
                thr = np.arange(n)[::-1] if left_deep else np.arange(n)
                trees.append(comb(thr, nxt + np.arange(n + 1), left_deep=left_deep))
                nxt += n + 1
        _UNEVEN[depth] = trees
    return _UNEVEN[depth]


@pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 512, 513, 1025])
@pytest.mark.parametrize("depth", [N_TILED, 4095], ids=["tiled", "depth4095_global"])
def test_two_walks_of_uneven_depth(ctx, depth, N):
    """A right-deep and a left-deep comb of depth 30 and of `depth`.  Thread t of a 512-row
    tile walks rows t and t + 256 in one loop: of each pair one row leaves a comb at depth 1
    and the other at its end, in both orders (even and odd t), and every seventh row stops
    somewhere between.  N: a lone row, a missing second row, ragged last tiles and a tile
    whose upper half lies past N."""
    trees = _uneven_forest(depth)
    r = np.arange(N)
    deep = ((r % 512) // 256 + r % 256) % 2 == 0
    x = np.where(deep, depth + 1.0, -1.0)
    mid = r % 7 == 3
    x[mid] = np.random.default_rng(N).integers(0, depth, mid.sum())
    pt = ref.per_tree(trees, [[0]] * 4, x[:, None])
    if N > 257:  # both orders within a thread's pair: deep / shallow and shallow / deep
        assert pt[2, 0] != pt[2, 256] and pt[2, 1] != pt[2, 257] and pt[2, 0] != pt[2, 1]
    check_all(ctx, trees, [[0]] * 4, x[:, None], pt=pt, widths=(1, 2) if N > 256 else (1,))


# ---------------------------------------------------------------- d. row width, LDS flip
F_TILED_MAX = max(F for F in range(1, 4096) if tiled_budget(host_stride(F), 2) is not None)
F_GLOBAL = (F_TILED_MAX // 16 + 1) * 16
assert tiled_budget(host_stride(F_TILED_MAX + 1), 2) is None


def _wide_forest(F):
    """Trees that split on features F - 1, 0 and F // 2 through the subspace
    [F - 1, 0, F // 2]; thresholds on the rows' value grid, 0.0 and -0.0 among them."""
    sub = [F - 1, 0, F // 2]
    trees = [stump(0.0, 1.0, 2.0, 0), stump(-0.0, 3.0, 5.0, 1), stump(1.5, 7.0, 11.0, 2),
             comb(np.arange(40) / 4.0 - 5.0, 100.0 + np.arange(41), feature=np.arange(40) % 3),
             comb((np.arange(25) / 2.0 - 6.0)[::-1], 200.0 + np.arange(26), feature=(np.arange(25) + 1) % 3,
                  left_deep=True),
             leaf(0.125)]
    return trees, [sub] * len(trees)


def _wide_rows(N, F, doctored, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-24, 25, size=(N, F)) / 4.0
    if doctored:
        X[rng.random(X.shape) < 0.05] = np.nan
        X[rng.random(X.shape) < 0.05] = -0.0
        X[rng.random(X.shape) < 0.02] = np.inf
        X[rng.random(X.shape) < 0.02] = -np.inf
        X[:8, F - 1] = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1.5, -5.0, 4.75]
    return X


@pytest.mark.parametrize("F", [1, 15, 16, 17, F_TILED_MAX, F_TILED_MAX + 1, F_GLOBAL])
def test_host_row_widths(ctx, F):
    """Host rows: F around the 16-code padding of Sq, the widest row plan_tiled accepts
    (the staged tile leaves a chunk of 13.5 KB) and the first rows past it -- F_TILED_MAX + 1
    and the next multiple of 16 -- which take the global walk; NaN, +-0 and +-inf cells."""
    trees, subs = _wide_forest(F)
    assert all(tree_bytes(n_internal(t)) <= tiled_budget(host_stride(F_TILED_MAX), 2) for t in trees)
    check_all(ctx, trees, subs, _wide_rows(700, F, True, F))


@pytest.mark.parametrize("F", [1, 2, 3, 5, 7, 64, 65, 256, 257])
def test_dataset_row_widths_u8(ctx, F):
    """Device dataset, u8 codes: the staging loop copies whole 32-bit words of a padded row
    (F = 1, 2, 3, 5, 7); 64 / 65 switch the row stride from 16s to 128s; at 257 features the
    stride of 384 bytes no longer leaves plan_tiled its chunk (256 does)."""
    trees, subs = _wide_forest(F)
    check_all(ctx, trees, subs, _wide_rows(700, F, False, F), widths=(1,))


# ---------------------------------------------------------------- e. dictionary sizes
@pytest.mark.parametrize("D,cb", [(256, 1), (257, 2), (65536, 2), (65537, 4)])
def test_dictionary_sizes(ctx, D, cb):
    """A column of D distinct values: the codes go from u8 to u16 past 256 and to u32 (the
    global walk) past 65 536.  Thresholds below the least value, at a value, one ulp to
    either side of one, between two, at the greatest value and above it; a second column
    of three values with thresholds 0.0 and -0.0."""
    N = 65537
    rng = np.random.default_rng(D)
    vals = np.unique(rng.normal(size=2 * D) * 1000.0)[:D]
    rng.shuffle(vals)
    assert len(vals) == D
    X = np.column_stack([vals[np.arange(N) % D], np.array([-1.0, 0.0, 2.5])[rng.integers(0, 3, N)]])
    s = np.sort(vals)
    at = sorted({0, 5, 255, 256 % D, D // 2, D - 2, D - 1})
    thr = [s[0] - 1.0, s[-1] + 1.0, (s[5] + s[6]) / 2, (s[D - 2] + s[D - 1]) / 2]
    for k in at:
        thr += [s[k], np.nextafter(s[k], np.inf), np.nextafter(s[k], -np.inf)]
    trees = [stump(t, 2.0 * i, 2.0 * i + 1, 0) for i, t in enumerate(thr)]
    trees += [comb(np.sort(thr), 1000.0 + np.arange(len(thr) + 1), 0),
              stump(0.0, 0.25, 0.5, 1), stump(-0.0, 0.75, 1.5, 1), stump(-1.0, 3.5, 4.5, 1)]
    check_all(ctx, trees, [[0, 1]] * len(trees), X, widths=(cb,))


# ---------------------------------------------------------------- f. order-sensitive sums
def test_order_sensitive_mean_and_sum(ctx):
    """200 single-leaf and stump trees whose fp64 sum depends on the order (1e16, 1, -1e16,
    1, ... and values an ulp apart), with four large combs between them so that the forest
    spans several chunks: the mean and the device sum are the in-order sums."""
    big = [1e16, 1.0, -1e16, 1.0]
    trees = []
    for k in range(200):
        if k % 50 == 40:
            trees.append(comb(np.arange(2000) / 400.0, 3.0 + np.arange(2001) * 2.0 ** -50))
        elif k % 2:
            trees.append(stump(k % 5 + 0.5, big[(k // 2) % 4], 0.1 * (1.0 + k * 2.0 ** -52)))
        else:
            trees.append(leaf(big[(k // 2 + 1) % 4] if k % 3 else 1.0 / 3.0))
    assert len(plan_chunks([tree_bytes(n_internal(t)) for t in trees], BUDGET_1F)) >= 3
    X = (np.random.default_rng(5).integers(0, 24, size=(700, 1)) / 4.0)
    pt = ref.per_tree(trees, [[0]] * 200, X)
    assert (ref.seq_sum(pt) != ref.seq_sum(pt[::-1])).any()  # the order does matter here
    check_all(ctx, trees, [[0]] * 200, X, pt=pt, widths=(1, 2))


# ---------------------------------------------------------------- g. mode counters
def _mode_limit(S, code_bytes):
    return max(C for C in range(1, 4097) if tiled_budget(S, code_bytes, C) is not None)


C_HOST = _mode_limit(host_stride(1), 2)  # host rows, and a u16 dataset of two features
C_U8 = _mode_limit(16, 1)                # a u8 dataset of one feature
MODE_CLASSES = sorted({C_HOST, C_HOST + 1, C_U8, C_U8 + 1, 256, 257, K_LDS_MODE_CLASSES,
                       K_LDS_MODE_CLASSES + 1, 4096})


@pytest.mark.parametrize("N", [300, 700])
@pytest.mark.parametrize("C", MODE_CLASSES)
def test_mode_at_counter_boundaries(ctx, C, N):
    """24 stumps over C classes: the last class count whose [C][512] u16 counters still fit
    the tiled kernel's LDS beside the row tile and the first that does not (host rows / u16
    codes, and u8 codes), 256 / 257 (votes of one byte, then two), kLdsModeClasses and one
    over (k_predict's counters move to global memory) and 4 096 (class id 4 095).  The rows
    that go left everywhere see 0, m, a, m, a, 0 four times over: three classes tie at 8 and
    m = C // 2 reaches it first, neither the smallest nor the last vote; the rows that go
    right everywhere see 1, a, 0, a, 0, 1 and a = C - 1 win the same way."""
    m, a = C // 2, C - 1
    lv = [0, m, a, m, a, 0] * 4
    rv = [1, a, 0, a, 0, 1] * 4
    trees = [stump(t % 4 + 0.5, lv[t], rv[t]) for t in range(24)]
    X = (np.arange(N) * 7 % 5).astype(np.float64)[:, None]
    pt = ref.per_tree(trees, [[0]] * 24, X)
    want = ref.mode(pt)
    assert (want[X[:, 0] == 0] == m).all() and (want[X[:, 0] == 4] == a).all()
    assert set(np.unique(want)) == {0.0, m, a}  # the rows between mix the two sequences
    check_all(ctx, trees, [[0]] * 24, X, gini=True, pt=pt, widths=(1, 2),
              votes=(1, 2) if C <= 256 else (2,))
