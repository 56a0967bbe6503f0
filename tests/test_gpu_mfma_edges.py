"""GPU: the MFMA root histogram (k_hist_mfma, sbag_mfma.hip) at the edges of its arithmetic.

tests/test_gpu_mfma_root.py compares MFMA-rooted forests with LDS-atomic-rooted ones at three
large shapes with the Poisson(1) sampler's bags.  Here the bag comes from the caller wherever
the sampler cannot produce it (sbag_fit_bag / sbag_fit_booster with SBAG_ROOT_MFMA=1, which
lifts the R >= 16 requirement), and every case

  (a) fits the same input with SBAG_ROOT_MFMA=1 and =0: trees and stats byte-identical,
  (b) compares both with the CPU oracle, every field bit for bit,
  (c) asserts root_ms > 0 where the MFMA root must run and == 0 where the host must divert,

and, where the case fixes the label digit planes, derives their count from root_mfma_ops =
2 32^3 ceil(N/32) F ceil(R/32) (1 + ND) and asserts it.

A. the int32 accumulators at their bound: count 127 on every row of a 65536-row slice, all in
   one bin, every digit plane at its extreme; counts of 128 and 255 divert.
B. the digit planes at the boundaries of their count and at the balanced digits' carry points.
C. one to four replica tiles per launch and replicas split over launches, 1 to 4 planes.
D. row counts around one 256-row chunk and one 65536-row slice, 1 / 8 / 9 / 17 features,
   5 and 32 bins, a constant column, no replacement, an empty partition.
E. the host's gate: N % 16 != 0, 33 values, a proper subspace, gini.

Labels are integers or quarters, features small integers of <= 32 values, so the labels'
fixed-point image is known here: k = y (k = 4 y for quarters).  Its range gives the expected
plane count (planes()), which the library's own count must equal.

Reachable instances: <1..4, 1> (C: 16-129 learners), <1..3, 2> (C: 96 / 97; D),
<1..2, 3> and <1..2, 4> (C: 64 / 65); <1, ND> at R = 1 (A, B)."""
import functools
import math

import numpy as np
import pytest

import oracle
from parity_utils import assert_forest_equal

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED = oracle.DEFAULT_SEED_REGRESSOR
SLICE = 65536  # rows of one workgroup of k_hist_mfma: its int32 accumulators must stay exact


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


# ---------------------------------------------------------------- expectations
def planes(kmin, kmax, mode):
    """Digit planes of an image range: unsigned 7-bit digits of k - kmin, or balanced base-256
    digits (each in [-128, 127]) of k - midpoint, n of which hold [-128 m, 127 m] with
    m = (256^n - 1) / 255; mode "7" / "8" forces one, "auto" takes the fewer."""
    span = kmax - kmin
    u = max(1, math.ceil(span.bit_length() / 7))
    lo, hi = -(span // 2), span - span // 2
    s = next(n for n in range(1, 9) if -128 * ((256**n - 1) // 255) <= lo and hi <= 127 * ((256**n - 1) // 255))
    return {"7": u, "8": s, "auto": min(u, s)}[mode]


def test_expected_plane_counts():
    """planes() at the boundaries sections A-C use, worked by hand: (auto, 7, 8)."""
    for span, want in [(127, (1, 1, 1)), (128, (1, 2, 1)), (16383, (2, 2, 2)), (16384, (2, 3, 2)),
                       (254, (1, 2, 1)), (255, (2, 2, 2)), (256, (2, 2, 2)), (254 * 257, (2, 3, 2)),
                       (255 * 257, (3, 3, 3)), (255 * 257 + 1, (3, 3, 3)), (2**21 - 1, (3, 3, 3)),
                       (2**21, (3, 4, 3)), (254 * 65793, (3, 4, 3)), (254 * 65793 + 1, (4, 4, 4))]:
        for kmin in (0, -span // 2, -span - 5):
            assert tuple(planes(kmin, kmin + span, m) for m in ("auto", "7", "8")) == want, (span, kmin)


def derived_planes(t, N, F, R):
    """ND from the library's root_mfma_ops (0 operations: the MFMA root did not run)."""
    unit = 2 * 32**3 * ((N + 31) // 32) * F * ((R + 31) // 32)
    ops = int(t["root_mfma_ops"])
    assert ops == t["root_mfma_ops"] and ops % unit == 0, (t["root_mfma_ops"], unit)
    return ops // unit - 1


def codes_are_bins(X, counts, part=None):
    """Does every replica's split-finding sample (its whole bag up to 10^4 draws) meet every
    value of every feature?  Then each value is a bin of its own for every replica, and the
    root histogram over the value codes is the level-0 histogram the trees are grown from;
    otherwise the fit bins the rows per replica and histograms the root again."""
    N, F = X.shape
    part = [0, N] if part is None else list(part)
    Xi = X.astype(np.int64)
    nval = [len(np.unique(Xi[:, f])) for f in range(F)]
    for row in counts:
        frac = oracle.split_sample_fraction(int(row.astype(np.int64).sum()), 32)
        m = oracle.split_sample(row, part, oracle.DT_SEED_REGRESSOR, frac) if frac < 1.0 else row
        for f in range(F):
            if np.count_nonzero(np.bincount(Xi[m > 0, f], minlength=64)) != nval[f]:
                return False
    return True


def forest_bytes(f):
    return [(f.tree(t)[0].tobytes(), f.tree(t)[1].tobytes()) for t in range(len(f))]


def check_pair(monkeypatch, fit, orf, N, F, R, *, mfma, nd=None, forced=True, min_nodes=3, digits="auto"):
    """fit() with the MFMA root asked for (SBAG_ROOT_MFMA=1 when forced, unset otherwise) and
    with SBAG_ROOT_MFMA=0: (a) byte-identical, (b) both the oracle's forest, (c) root_ms > 0
    exactly when `mfma`, and then nd digit planes."""
    if digits == "auto":
        monkeypatch.delenv("SBAG_MFMA_DIGITS", raising=False)
    else:
        monkeypatch.setenv("SBAG_MFMA_DIGITS", digits)
    if forced:
        monkeypatch.setenv("SBAG_ROOT_MFMA", "1")
    else:
        monkeypatch.delenv("SBAG_ROOT_MFMA", raising=False)
    a = fit()
    monkeypatch.setenv("SBAG_ROOT_MFMA", "0")
    b = fit()
    ta, tb = a.timing(), b.timing()
    print(f"root_ms {ta['root_ms']:.3f} / {tb['root_ms']:.3f}, mfma ops {ta['root_mfma_ops']:.0f}, "
          f"chain_ms {ta['chain_ms']:.3f}, nodes {[len(a.tree(t)[0]) for t in range(min(len(a), 4))]}")
    assert tb["root_ms"] == 0.0 and tb["root_mfma_ops"] == 0.0, tb
    if mfma:
        assert ta["root_ms"] > 0.0, ta
        if nd is not None:
            assert derived_planes(ta, N, F, R) == nd, (ta["root_mfma_ops"], nd)
        else:
            assert derived_planes(ta, N, F, R) in (1, 2, 3, 4)
    else:
        assert ta["root_ms"] == 0.0 and ta["root_mfma_ops"] == 0.0, ta
    assert len(a) == len(b) == R
    assert forest_bytes(a) == forest_bytes(b)
    assert_forest_equal(a, orf)
    assert_forest_equal(b, orf)
    assert all(len(a.tree(t)[0]) >= min_nodes for t in range(R)), [len(a.tree(t)[0]) for t in range(R)]
    return a, ta


def bag_fitter(ctx, X, y, bag, depth):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    sub = np.arange(X.shape[1], dtype=np.int32)

    def fit():
        return nat.fit_bag(ctx, ds, bag, sub, impurity=nat.IMPURITY_VARIANCE, max_depth=depth, max_bins=32)

    return ds, fit


def oracle_bag(X, y, bag, depth):
    return oracle.fit(X, y, bag[None, :], [np.arange(X.shape[1], dtype=np.int32)], max_depth=depth, max_bins=32)


def integer_engine(N, cmax, kmin, kmax):
    """The integer engine keeps a fit while N cmax kabs^2 < 2^53 (sbag_budget.h)."""
    return N * cmax * max(abs(kmin), abs(kmax)) ** 2 < 2**53


# ---------------------------------------------------------------- A: accumulators at their bound
# variant: (SBAG_MFMA_DIGITS, kmin, kmax, the label of every row of the loaded slices, its digits)
A_VARIANTS = {
    # unsigned: k - kmin = 127, and 127 + 127 * 128
    "u1": ("7", 0, 127, 127, (127,)),
    "u2": ("7", -8191, 8192, 8192, (127, 127)),
    # balanced about the midpoint 0 (the range's two sides differ by at most one, so one digit
    # spans [-127, 127] and -128 needs a second): 127; 127 + 127 * 256; -128 + 127 * 256
    "b1": ("8", -127, 127, 127, (127,)),
    "b2hi": ("8", -32639, 32639, 32639, (127, 127)),
    "b2lo": ("8", -32639, 32639, 32384, (-128, 127)),
}
A_DEPTH = 3


@functools.lru_cache(maxsize=None)
def a_data(variant, nslices=1):
    mode, kmin, kmax, kload, digs = A_VARIANTS[variant]
    NL = nslices * SLICE
    N = NL + 4096
    rng = np.random.default_rng(17)
    x0 = np.zeros(N, np.int64)
    x0[NL:] = 1 + np.arange(4096) % 15  # the loaded slices: bin 0 alone; the rest: bins 1..15
    x1 = np.arange(N) % 32
    rng.shuffle(x1)
    X = np.stack([x0, x1], axis=1).astype(np.float64)
    k = np.full(N, kload, np.int64)
    # ordinary labels on the rest: across the whole range, both ends present
    k[NL:] = kmin + ((x0[NL:] - 1) * (kmax - kmin)) // 14
    k[NL + 30:] = np.clip(k[NL + 30:] + rng.integers(-3, 4, N - NL - 30), kmin, kmax)
    assert k.min() == kmin and k.max() == kmax and len(np.unique(x1)) == 32 and len(np.unique(x0)) == 16
    # the image's digits on the loaded rows are the extremes the variant names
    base, off = (128, kmin) if mode == "7" else (256, kmin + (kmax - kmin) // 2)
    assert sum(d * base**j for j, d in enumerate(digs)) == kload - off
    assert len(digs) == planes(kmin, kmax, mode)
    # (the rest is drawn often too: the split-finding sample, 10^4 of the bag's 9 10^6 draws,
    # must meet every value of feature 0 for the codes to be the bins)
    bag = rng.integers(90, 128, N).astype(np.uint8)
    bag[:NL] = 127
    return X, k.astype(np.float64), bag, N


@functools.lru_cache(maxsize=None)
def a_oracle(variant, nslices, top):
    X, y, bag, N = a_data(variant, nslices)
    bag = bag.copy()
    if top != 127:
        bag[N // 3] = top
    return bag, oracle_bag(X, y, bag, A_DEPTH)


def run_a(ctx, monkeypatch, variant, nslices=1, top=127):
    mode, kmin, kmax, kload, digs = A_VARIANTS[variant]
    X, y, _, N = a_data(variant, nslices)
    bag, orf = a_oracle(variant, nslices, top)
    assert codes_are_bins(X, bag[None, :])
    NL = nslices * SLICE
    assert int(bag.max()) == top and (bag[:NL] >= 127).all()
    # the largest |sum| one slice's int32 accumulator holds, below 2^31
    assert 127 * max(abs(d) for d in digs) * SLICE in (127 * 127 * SLICE, 127 * 128 * SLICE)
    assert 127 * 128 * SLICE < 2**31
    ds, fit = bag_fitter(ctx, X, y, bag, A_DEPTH)
    try:
        f, t = check_pair(monkeypatch, fit, orf, N, 2, 1, mfma=top <= 127, nd=len(digs), digits=mode)
    finally:
        ds.free()
    # the engine the inputs imply is the one that ran
    assert (t["chain_ms"] == 0.0) == integer_engine(N, top, kmin, kmax), t
    # the root splits feature 0 between the loaded bin and the rest; the left child is those sums
    nodes, stats = f.tree(0)
    assert nodes["feature"][0] == 0 and nodes["threshold"][0] == 0.5
    left = int(nodes["left"][0])
    cnt = int(bag[:NL].astype(np.int64).sum())
    assert stats[left][0] == cnt and nodes["prediction"][left] == float(kload) and nodes["impurity"][left] == 0.0
    return t


@pytest.mark.parametrize("variant", ["u1", "u2", "b1"])
def test_accumulators_at_bound_integer_engine(ctx, monkeypatch, variant):
    """127 x 127 x 65536 in every digit plane of one slice (unsigned one and two planes,
    balanced one plane), on the integer engine."""
    _, kmin, kmax, _, _ = A_VARIANTS[variant]
    assert integer_engine(SLICE + 4096, 127, kmin, kmax)
    run_a(ctx, monkeypatch, variant)


@pytest.mark.parametrize("variant", ["b2hi", "b2lo"])
def test_accumulators_at_bound_fp64_engine(ctx, monkeypatch, variant):
    """Two balanced planes at (127, 127) and at (-128, 127): -127 x 128 x 65536 in the low
    plane.  The range [-32639, 32639] two balanced digits hold passes N cmax kabs^2 = 2^53 at
    this bag, so the fp64 engine takes the fit -- with the MFMA root, on the exact image."""
    _, kmin, kmax, _, _ = A_VARIANTS[variant]
    assert not integer_engine(SLICE + 4096, 127, kmin, kmax)
    t = run_a(ctx, monkeypatch, variant)
    assert t["chain_ms"] > 0.0


def test_accumulators_at_bound_three_slices(ctx, monkeypatch):
    """Three loaded slices: 127 x 127 x 196608 > 2^31 if their rows shared an accumulator.
    (127 x 128 x 131072 < 2^31: two slices in one accumulator would still be exact.)"""
    assert 127 * 128 * 2 * SLICE < 2**31 < 127 * 127 * 3 * SLICE
    run_a(ctx, monkeypatch, "u1", nslices=3)


@pytest.mark.parametrize("top", [128, 255])
def test_count_past_int8_takes_the_lds_root(ctx, monkeypatch, top):
    """The same bag with one row at 128 (the first count the host must divert) and at 255."""
    run_a(ctx, monkeypatch, "u1", top=top)


# ---------------------------------------------------------------- B: digit boundaries
NB_ = 4112  # rows of sections B and C: 16 full 256-row chunks and 16 rows
B_DEPTH = 4
# name: (kmin, kmax, offsets from the range's midpoint that must occur)
B_RANGES = {
    "u127": (-37, -37 + 127, ()),
    "u128": (-37, -37 + 128, ()),
    "u16383": (-5000, -5000 + 16383, ()),
    "u16384": (-5000, -5000 + 16384, ()),
    # balanced digits about the midpoint hold a span of 254 m; 255 m is [-128 m, 127 m] itself
    "s254": (1000, 1000 + 254, (-127, 127)),
    "s255": (1000 - 128, 1000 + 127, (-127, 128)),
    "s256": (1000 - 128, 1000 + 128, (-128, 128)),
    "s254m": (-300 - 127 * 257, -300 + 127 * 257, (-127 * 257, 127 * 257)),
    # (32640 = 127 * 257 + 1 is the first offset with a third digit: -128, -128, 1)
    "s255m": (-300 - 128 * 257, -300 + 127 * 257, (-32767, 32768, 32639, 32640, -32640, -32641)),
    "s255m1": (-300 - 128 * 257, -300 + 127 * 257 + 1, (-32768, 32768, 32639, 32640, -32640, -32641)),
    # low bytes 0x7F / 0x80 / 0xFF of the offset, and -129, at one and two bytes
    "carry": (-3000 + 11, 3000 + 11, (0x7F, 0x80, 0xFF, 0x100, -0x7F, -0x80, -129, -0xFF, -0x100, 0x17F, 0x180,
                                       0x7FF, 0x87F, 0x880, -0x180, -0x181, -0x880, -0x881)),
}


def features(N, F, kind, seed):
    """Small-integer columns: "mixed" 32 / 5 / 17 / 2 values, "small" 8 / 5 / 3 / 2, "nb5" at
    most 5, "v32" exactly 32 each; "const" / "smallconst": column 0 constant."""
    rng = np.random.default_rng(seed)
    lv = {"mixed": [32, 5, 17, 2], "const": [32, 5, 17, 2], "small": [8, 5, 3, 2], "smallconst": [8, 5, 3, 2],
          "nb5": [5, 3, 2, 4], "v32": [32]}[kind]
    X = np.stack([rng.integers(0, lv[f % len(lv)], size=N) for f in range(F)], axis=1)
    if N >= 64:
        for f in range(F):  # every value occurs
            X[: lv[f % len(lv)], f] = np.arange(lv[f % len(lv)])
    if kind in ("const", "smallconst"):
        X[:, 0] = 3
    return X.astype(np.float64)


@functools.lru_cache(maxsize=None)
def b_data(name):
    kmin, kmax, offs = B_RANGES[name]
    rng = np.random.default_rng(len(name) * 131 + kmax)
    X = features(NB_, 3, "mixed", 5)
    span = kmax - kmin
    k = kmin + (X[:, 0].astype(np.int64) * span) // 31  # follows feature 0 across the whole range
    k = np.clip(k + rng.integers(-(span // 16) - 1, span // 16 + 2, NB_), kmin, kmax)
    mid = kmin + span // 2
    rows = rng.permutation(NB_)
    k[rows[:60]], k[rows[60:120]] = kmin, kmax
    for j, o in enumerate((-1, 0, 1) + tuple(offs)):
        assert kmin <= mid + o <= kmax
        k[rows[120 + 60 * j: 180 + 60 * j]] = mid + o
    assert k.min() == kmin and k.max() == kmax
    bag = rng.poisson(1.0, NB_).astype(np.uint8)
    bag[rows[:3 * 60:7]] = 9
    y = k.astype(np.float64)
    assert codes_are_bins(X, bag[None, :])
    return X, y, bag, oracle_bag(X, y, bag, B_DEPTH)


@pytest.mark.parametrize("mode", ["auto", "7", "8"])
@pytest.mark.parametrize("name", list(B_RANGES))
def test_digit_plane_boundaries(ctx, monkeypatch, name, mode):
    """Unsigned ranges of 127 | 128 and 16383 | 16384; balanced spans of 254 m | 255 m |
    255 m + 1 for m = 1 and 257; offsets from the midpoint whose low bytes are 0x7F, 0x80,
    0xFF and -129: with the host's choice and with either encoding forced."""
    kmin, kmax, _ = B_RANGES[name]
    X, y, bag, orf = b_data(name)
    assert integer_engine(NB_, int(bag.max()), kmin, kmax)
    ds, fit = bag_fitter(ctx, X, y, bag, B_DEPTH)
    try:
        _, t = check_pair(monkeypatch, fit, orf, NB_, 3, 1, mfma=True, nd=planes(kmin, kmax, mode), digits=mode)
    finally:
        ds.free()
    assert t["chain_ms"] == 0.0


def nondyadic(N, seed):
    X = features(N, 3, "mixed", 5)
    rng = np.random.default_rng(seed)
    y = (X[:, 0] * 3.0 - X[:, 1] + rng.integers(-8, 9, size=N)) * 1.1 + 0.3
    return X, y, rng.poisson(1.0, N).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def b_f64_data(api):
    X, y, bag = nondyadic(NB_, 23)
    if api == "booster":  # residual-like: what is left of y after a first constant model
        y = -(-(y - (y.mean() + 0.0)))
    assert codes_are_bins(X, bag[None, :])
    return X, y, bag, oracle_bag(X, y, bag, B_DEPTH)


@pytest.mark.parametrize("mode,nd", [("auto", 3), ("7", 4), ("8", 3)])
@pytest.mark.parametrize("api", ["bag", "booster"])
def test_fp64_image_planes(ctx, monkeypatch, api, mode, nd):
    """Non-dyadic labels: the fp64 engine's screening image k = round(y 2^s), 2^21 <= max|k| <
    2^22 with 0 in its range, takes 3 balanced planes and 4 unsigned ones -- through
    sbag_fit_bag (the dataset's labels) and sbag_fit_booster (the caller's residuals)."""
    X, y, bag, orf = b_f64_data(api)
    sub = np.arange(3, dtype=np.int32)
    ds = nat.DeviceDataset.from_numpy(X, y if api == "bag" else np.zeros(NB_), ctx)

    def fit():
        if api == "bag":
            return nat.fit_bag(ctx, ds, bag, sub, impurity=nat.IMPURITY_VARIANCE, max_depth=B_DEPTH, max_bins=32)
        return nat.fit_booster(ctx, ds, y, bag, sub, max_depth=B_DEPTH, max_bins=32)

    try:
        _, t = check_pair(monkeypatch, fit, orf, NB_, 3, 1, mfma=True, nd=nd, digits=mode)
    finally:
        ds.free()
    assert t["chain_ms"] > 0.0


# ---------------------------------------------------------------- C: replica tiles, launch splits
C_F, C_DEPTH = 9, 5


@functools.lru_cache(maxsize=None)
def c_data(label):
    X = features(NB_, C_F, "mixed", 41)
    rng = np.random.default_rng(43)
    x0, x1 = X[:, 0].astype(np.int64), X[:, 1].astype(np.int64)
    if label == "p1":  # span 60: one plane either way
        k = x0 + 5 * x1 + rng.integers(0, 10, NB_) - 20
    elif label == "p2":  # span 3498: two planes either way
        k = 100 * x0 - 50 * x1 + rng.integers(0, 200, NB_)
    else:  # non-dyadic: three balanced planes, four unsigned
        return X, (x0 * 3.0 - x1 + rng.integers(-8, 9, NB_)) * 1.1 + 0.3, None
    assert len(np.unique(x0)) == 32 and len(np.unique(x1)) == 5
    return X, k.astype(np.float64), (int(k.min()), int(k.max()))


@functools.lru_cache(maxsize=None)
def c_oracle(label, L):
    X, y, _ = c_data(label)
    counts = oracle.bag(True, 1.0, 0, L, SEED, [0, NB_], NB_)
    assert counts.max() <= 127 and codes_are_bins(X, counts)
    subs = [oracle.subspace(1.0, C_F, SEED + i) for i in range(L)]
    return oracle.fit(X, y, counts, subs, max_depth=C_DEPTH, max_bins=32)


def sampler_fitter(ctx, X, y, L, depth, **kw):
    ds = nat.DeviceDataset.from_numpy(X, y, ctx)
    args = dict(replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L,
                max_depth=depth, max_bins=32, impurity=nat.IMPURITY_VARIANCE)
    args.update(kw)

    def fit():
        return nat.fit(ctx, ds, **args)

    return ds, fit


# launches of at most 4, 3, 2, 2 tiles of 32 replicas for 1, 2, 3, 4 planes
C_CASES = ([("p1", "auto", 1, L) for L in (16, 31, 32, 33, 96, 97, 128, 129)] +
           [("p2", "auto", 2, L) for L in (96, 97)] +
           [("nd", "auto", 3, L) for L in (64, 65)] +
           [("nd", "7", 4, L) for L in (64, 65)])


@pytest.mark.parametrize("label,mode,nd,L", C_CASES)
def test_replica_tiles_and_launch_splits(ctx, monkeypatch, label, mode, nd, L):
    """Exact tile multiples and one replica past them: k_hist_mfma<1..4, 1>, <3, 2>, <2, 3>,
    <2, 4>, and the remainder launch's <1, ND> with its counts / histogram offsets."""
    X, y, krange = c_data(label)
    if krange:
        assert planes(*krange, "7") == planes(*krange, "8") == nd
    ds, fit = sampler_fitter(ctx, X, y, L, C_DEPTH)
    try:
        check_pair(monkeypatch, fit, c_oracle(label, L), NB_, C_F, L, mfma=True, nd=nd, forced=False, digits=mode)
    finally:
        ds.free()


@pytest.mark.parametrize("forced", [True, False])
def test_fifteen_replicas_need_the_override(ctx, monkeypatch, forced):
    """Below 16 replicas the host keeps the LDS atomics unless SBAG_ROOT_MFMA=1."""
    X, y, _ = c_data("p1")
    ds, fit = sampler_fitter(ctx, X, y, 15, C_DEPTH)
    try:
        check_pair(monkeypatch, fit, c_oracle("p1", 15), NB_, C_F, 15, mfma=forced, nd=1, forced=forced)
    finally:
        ds.free()


# ---------------------------------------------------------------- D: row and feature edges
D_L, D_DEPTH = 33, 5
D_CASES = [
    # N: below one 256-row chunk, a chunk and 16 rows either side, a slice and 16 rows either side
    # (up to 272 rows a value of 32 would miss some learner's bag: at most 8 values there)
    (16, 9, "nb5"), (240, 1, "nb5"), (256, 8, "small"), (272, 9, "small"), (272, 17, "smallconst"),
    (65520, 17, "mixed"), (65536, 9, "const"), (65536, 8, "nb5"), (65552, 9, "v32"), (65552, 1, "v32"),
]


def d_labels(X, seed):
    """Quarters: k = 4 y, span a few hundred (two planes either way)."""
    rng = np.random.default_rng(seed)
    F = X.shape[1]
    k = 12 * X[:, 0].astype(np.int64) - 7 * X[:, min(1, F - 1)].astype(np.int64) + rng.integers(-40, 41, len(X))
    k[0] |= 1  # (the image's shift is 2)
    return k / 4.0


@functools.lru_cache(maxsize=None)
def d_data(N, F, kind, replacement=True, ratio=1.0, part=None):
    X = features(N, F, kind, N + F)
    y = d_labels(X, N)
    part_ = list(part) if part else [0, N]
    counts = oracle.bag(replacement, ratio, 0, D_L, SEED, part_, N)
    subs = [oracle.subspace(1.0, F, SEED + i) for i in range(D_L)]
    return X, y, oracle.fit(X, y, counts, subs, max_depth=D_DEPTH, max_bins=32, part=part_), \
        codes_are_bins(X, counts, part_)


@pytest.mark.parametrize("N,F,kind", D_CASES)
def test_row_and_feature_edges(ctx, monkeypatch, N, F, kind):
    """The min(row, n1 - 16) clamps and the double buffer's `more` flag at N = 16 ... 65552;
    F = 1 (seven idle waves), 8, 9 and 17; NB = 5 (lanes past the bins), exactly 32 values,
    a constant column."""
    X, y, orf, shared = d_data(N, F, kind)
    nb = max(len(np.unique(X[:, f])) for f in range(F))
    if N >= 64:
        assert nb == {"mixed": 32, "const": 32, "small": 8, "smallconst": 8, "nb5": 5, "v32": 32}[kind]
        assert shared  # (N = 16: some learner's bag misses a value; the root is histogrammed again)
    ds, fit = sampler_fitter(ctx, X, y, D_L, D_DEPTH)
    try:
        check_pair(monkeypatch, fit, orf, N, F, D_L, mfma=True, forced=False,
                   min_nodes=1 if N == 16 else 3)
    finally:
        ds.free()


def test_without_replacement(ctx, monkeypatch):
    """Counts of 0 / 1 at ratio 0.5, every feature to every learner."""
    N, F = NB_, 9
    X, y, orf, shared = d_data(N, F, "mixed", False, 0.5)
    assert shared
    ds, fit = sampler_fitter(ctx, X, y, D_L, D_DEPTH, replacement=False, sample_ratio=0.5,
                             subspace_bug_compat=False, subspace_ratio=1.0)
    try:
        check_pair(monkeypatch, fit, orf, N, F, D_L, mfma=True, forced=False)
    finally:
        ds.free()


def test_three_partitions_one_empty(ctx, monkeypatch):
    N, F, part = NB_, 9, (0, 1500, 1500, NB_)
    X, y, orf, shared = d_data(N, F, "mixed", part=part)
    assert shared
    ds, fit = sampler_fitter(ctx, X, y, D_L, D_DEPTH, partition_offsets=list(part))
    try:
        check_pair(monkeypatch, fit, orf, N, F, D_L, mfma=True, forced=False)
    finally:
        ds.free()


# ---------------------------------------------------------------- E: the gate
E_L = 16


@pytest.mark.parametrize("case", ["n4113", "v33", "subspace", "gini"])
def test_gate_diverts(ctx, monkeypatch, case):
    """What k_hist_mfma cannot take stays with the LDS atomics even under SBAG_ROOT_MFMA=1: a
    row count off the 16-row pieces, a feature of 33 values, a proper feature subspace, gini."""
    N, F = (4113 if case == "n4113" else NB_), 9
    X = features(N, F, "mixed", 77)
    if case == "v33":
        X[:33, 2] = np.arange(33)
        assert len(np.unique(X[:, 2])) == 33
    gini = case == "gini"
    y = d_labels(X, 3)
    if gini:
        y = ((X[:, 0] + X[:, 1]) % 4).astype(np.float64)
    sratio = 0.7 if case == "subspace" else 1.0
    counts = oracle.bag(True, 1.0, 0, E_L, SEED, [0, N], N)
    subs = [oracle.subspace(sratio, F, SEED + i) for i in range(E_L)]
    if case == "subspace":
        assert any(len(s) < F for s in subs)
    orf = oracle.fit(X, y, counts, subs, max_depth=D_DEPTH, max_bins=32, classification=gini)
    ds, fit = sampler_fitter(ctx, X, y, E_L, D_DEPTH, subspace_bug_compat=False, subspace_ratio=sratio,
                             impurity=nat.IMPURITY_GINI if gini else nat.IMPURITY_VARIANCE)
    try:
        check_pair(monkeypatch, fit, orf, N, F, E_L, mfma=False)
    finally:
        ds.free()
