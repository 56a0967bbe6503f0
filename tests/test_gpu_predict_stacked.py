"""GPU: sbag_predict_stacked / sbag_predict_stacked_dataset on hand-built forests against the
composed result (sbag_predict's per-tree matrix, then sbag_predict of the stack tree on it) and
the NumPy restatement (stacking_ref.predict), bit for bit -- on the fused pass, and with
SBAG_STACK_FORCE_FALLBACK=1 (ranks chunk by chunk, then the stack tree) and =2 (ranks by the
node walk from global memory).  The knob is set in the environment of a fresh child process
(this file run as a script), which writes every case's outputs to an .npz the test reads.

Run as a script: python test_gpu_predict_stacked.py OUT.npz"""
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest  # noqa: F401  (as a script too: registers spark_bagging_amd)
import stacking_ref as sref

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

VAR = nat.IMPURITY_VARIANCE
F = 3


# ---------------------------------------------------------------- hand-built trees
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


def comb(thr, leaves, feature=0):
    """len(thr) internal nodes in one right-deep chain, pre-order ids."""
    thr = np.asarray(thr, np.float64)
    n = len(thr)
    a = _blank(2 * n + 1)
    i = 2 * np.arange(n)
    a["left"][i], a["right"][i] = i + 1, i + 2
    a["feature"][i] = feature
    a["threshold"][i] = thr
    a["prediction"][np.concatenate([i + 1, [2 * n]])] = leaves
    return a


def tree3(f0, t0, f1, t1, leaves):
    """(f0 <= t0 ? (f1 <= t1 ? l0 : l1) : l2)"""
    a = _blank(5)
    a["left"][0], a["right"][0], a["feature"][0], a["threshold"][0] = 1, 4, f0, t0
    a["left"][1], a["right"][1], a["feature"][1], a["threshold"][1] = 2, 3, f1, t1
    a["prediction"][[2, 3, 4]] = leaves
    return a


def rows(n, seed=1):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, F)) * 8) / 4
    X[rng.random((n, F)) < 0.1] = 0.0
    X[:, 2] = rng.integers(-30, 1030, n)
    return X


BASE = [stump(1.0, 10.0, 20.0, feature=0),                       # 0
        tree3(1, 0.0, 0, -1.0, [-1.5, 2.5, -0.0]),               # 1
        leaf(7.0),                                               # 2: a single leaf
        comb([-1.0, 0.0, 1.0], [0.0, -3.0, 10.0, 4.0], feature=1)]  # 3
SUBS = [np.arange(F, dtype=np.int32)] * 4


def cases():
    """name -> (base trees, their subspaces, stack tree, stack subspace, host rows)."""
    c = {}
    # thresholds exactly equal to base leaf values (the <= side), between, below and above all
    # (tree 1 <= -1.5 ? 1 : tree 3 <= -100 ? 2 : tree 1 <= -0.0 ? 3 : tree 0 <= 10 ? 4 : tree 3 <= 1e9 ? 5 : 6)
    stack = comb([-1.5, -100.0, -0.0, 10.0, 1e9], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], feature=0)
    stack["feature"][[0, 2, 4, 6, 8]] = [1, 3, 1, 0, 3]
    for n in (1, 257, 4099):
        c[f"edges_n{n}"] = (BASE, SUBS, stack, np.arange(4, dtype=np.int32), rows(n, seed=n))
    # the stack subspace permutes the base trees: its feature j is base tree perm[j]
    perm = np.array([1, 3, 2, 0], np.int32)
    c["permuted"] = (BASE, SUBS, stack, perm, rows(257, seed=2))
    # a single-leaf stack tree
    c["stack_leaf"] = (BASE, SUBS, leaf(-8.5), np.arange(4, dtype=np.int32), rows(257, seed=3))
    # one feature twice (a window 0 < tree 3 <= 4), another never; tests the single-leaf tree 2 too
    twice = tree3(3, 4.0, 3, 0.0, [11.0, 12.0, 13.0])
    c["twice"] = (BASE, SUBS, twice, np.arange(4, dtype=np.int32), rows(257, seed=4))
    c["tests_leaf_tree"] = (BASE, SUBS, stump(7.0, 1.0, 2.0, feature=2), np.arange(4, dtype=np.int32),
                            rows(63, seed=5))
    # host rows outside every threshold: huge, infinite, NaN (a dataset refuses NaN: host rows only)
    X = rows(64, seed=6)
    X[0::4] = 1e300
    X[1::4] = -np.inf
    X[2::8] = np.nan
    X[3, 1] = np.inf
    c["outside"] = (BASE, SUBS, stack, np.arange(4, dtype=np.int32), X)
    # a NaN base leaf compares false with every threshold
    nan_base = BASE[:3] + [comb([0.0, 1.0], [np.nan, 1.0, 2.0], feature=1)]
    c["nan_leaf"] = (nan_base, SUBS, stack, np.arange(4, dtype=np.int32), rows(257, seed=7))
    # three combs of 1000 internal nodes: two LDS chunks of the base forest
    combs = [comb(np.arange(1000.0), np.arange(1001.0) * 0.5 - 3.0, feature=2),
             comb(np.arange(1000.0) + 0.5, np.arange(1001.0) % 7, feature=2),
             comb(np.arange(1000.0) - 0.5, -np.arange(1001.0), feature=2)]
    st = tree3(0, 250.0, 2, -400.0, [1.0, 2.0, 3.0])
    c["chunks"] = (combs, SUBS[:3], st, np.arange(3, dtype=np.int32), rows(4099, seed=8))
    # seven of them, all tested: past the fused pass's LDS, the general path on its own
    big = [comb(np.arange(1000.0) + k / 8.0, np.arange(1001.0) * (k + 1), feature=2) for k in range(7)]
    stb = comb([100.0 * (k + 1) ** 2 for k in range(7)], np.arange(8.0), feature=0)  # tree k's leaf index <= 100 (k + 1)
    stb["feature"][2 * np.arange(7)] = np.arange(7)
    c["past_fused"] = (big, [SUBS[0]] * 7, stb, np.arange(7, dtype=np.int32), rows(257, seed=9))
    # a comb past the 64 KB chunk: the node walk on its own
    deep = [comb(np.arange(3000.0) / 2.0, np.arange(3001.0), feature=2), BASE[0]]
    c["past_chunk"] = (deep, SUBS[:2], tree3(0, 700.0, 1, 10.0, [1.0, 2.0, 3.0]),
                       np.arange(2, dtype=np.int32), rows(257, seed=10))
    return c


def forests(case):
    trees, subs, stack, ssub, _ = case
    return (nat.NativeForest.from_trees(trees, subs, VAR), nat.NativeForest.from_trees([stack], [ssub], VAR))


def run_cases(ctx):
    """name -> (host rows' output, the dataset's output over the finite rows)."""
    out = {}
    for name, case in cases().items():
        base, stack = forests(case)
        X = case[4]
        fin = X[np.isfinite(X).all(axis=1)]
        ds = nat.DeviceDataset.from_numpy(fin, np.zeros(len(fin)), ctx)
        out[name + ":host"] = nat.predict_stacked(ctx, base, stack, X)
        out[name + ":dataset"] = nat.predict_stacked(ctx, base, stack, ds)
        if name == "edges_n257":  # the level-1 dataset too (the knob sends it through the host ingest)
            out.update(exported_level1(ds.stacked(base)))
        ds.free()
        base.free()
        stack.free()
    return out


def exported_level1(l1):
    n, f, s, cb, dv = l1.layout()
    codes = np.zeros(n * s * cb, np.uint8)
    d, off, _ = l1.export(codes.ctypes.data)
    l1.free()
    return {"level1:layout": np.array([n, f, s, cb, dv]), "level1:codes": codes, "level1:dict": d,
            "level1:off": off}


if __name__ == "__main__":
    c = nat.Context(0)
    np.savez(sys.argv[1], **run_cases(c))
    c.close()
    sys.exit(0)


# ---------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def expected(ctx):
    """The composed result of every case, checked against the restatement once."""
    want = {}
    for name, case in cases().items():
        trees, subs, stack, ssub, X = case
        base, sf = forests(case)
        _, pt = nat.predict(ctx, base, X, nat.AGG_MEAN, per_tree=True)
        composed = nat.predict(ctx, sf, np.ascontiguousarray(pt.T), nat.AGG_MEAN)
        assert np.array_equal(bits(composed), bits(sref.predict(trees, subs, stack, ssub, X))), name
        fin = np.isfinite(X).all(axis=1)
        want[name + ":host"] = composed
        want[name + ":dataset"] = composed[fin]
        if name == "edges_n257":
            want.update(exported_level1(nat.DeviceDataset.from_numpy(np.ascontiguousarray(pt.T), np.zeros(len(X)), ctx)))
        base.free()
        sf.free()
    return want


def assert_all_equal(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k


def test_cases_reach_their_edges(expected):
    c = cases()
    trees, subs, stack, ssub, X = c["edges_n4099"]
    P = sref.level1(trees, subs, X)
    # the thresholds -1.5 and -0.0 equal leaves of tree 1, 10.0 one of tree 0: rows on the <= side
    assert (P[:, 1] == -1.5).any() and (P[:, 1] == 0.0).any()
    assert ((P[:, 1] == 2.5) & (P[:, 0] == 10.0)).any() and ((P[:, 1] == 2.5) & (P[:, 0] == 20.0)).any()
    assert set(np.unique(expected["edges_n4099:host"])) == {1.0, 3.0, 4.0, 5.0}
    assert 6.0 in expected["nan_leaf:host"]  # NaN <= 1e9 is false
    assert len(np.unique(expected["twice:host"])) == 3 and len(np.unique(expected["chunks:host"])) == 3
    assert len(np.unique(expected["permuted:host"])) >= 3
    assert not np.array_equal(expected["permuted:host"], expected["edges_n257:host"][:257])
    assert np.isnan(c["outside"][4]).any() and len(np.unique(expected["outside:host"])) >= 2
    assert len(np.unique(expected["past_fused:host"])) >= 4 and len(np.unique(expected["past_chunk:host"])) == 3
    assert np.isnan(sref.level1(*c["nan_leaf"][:2], c["nan_leaf"][4])).any()


def test_fused_pass_equals_the_composed_result(ctx, expected):
    assert "SBAG_STACK_FORCE_FALLBACK" not in os.environ
    assert_all_equal(run_cases(ctx), expected)


@pytest.mark.parametrize("knob", ["1", "2"])
def test_forced_fallbacks_equal_the_composed_result(expected, tmp_path, knob):
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, SBAG_STACK_FORCE_FALLBACK=knob)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(out) as z:
        assert_all_equal({k: z[k] for k in z.files}, expected)


def test_batched_host_rows(ctx, expected, monkeypatch):
    """Host rows in batches of 100 (sbag_predict's knob): 4099 rows, tails included."""
    monkeypatch.setenv("SBAG_PREDICT_BATCH_ROWS", "100")
    case = cases()["edges_n4099"]
    base, stack = forests(case)
    got = nat.predict_stacked(ctx, base, stack, case[4])
    assert np.array_equal(bits(got), bits(expected["edges_n4099:host"]))
    base.free()
    stack.free()


def test_refusals(ctx, expected):
    case = cases()["edges_n257"]
    trees, subs, stack, ssub, X = case
    base, good = forests(case)
    two = nat.NativeForest.from_trees([stack, stack], [ssub, ssub], VAR)
    short = nat.NativeForest.from_trees([leaf(1.0)], [np.arange(3, dtype=np.int32)], VAR)
    long_ = nat.NativeForest.from_trees([leaf(1.0)], [np.arange(5, dtype=np.int32)], VAR)
    past = nat.NativeForest.from_trees([leaf(1.0)], [np.array([0, 1, 2, 4], np.int32)], VAR)
    ds = nat.DeviceDataset.from_numpy(X, np.zeros(len(X)), ctx)
    for bad in (two, short, long_, past):
        for arg in (X, ds):
            with pytest.raises(sb.IllegalArgumentException) as e:
                nat.predict_stacked(ctx, base, bad, arg)
            assert e.value.code == nat.SBAG_EINVAL
    with pytest.raises(sb.IllegalArgumentException):  # rows shorter than a base subspace
        nat.predict_stacked(ctx, base, good, X[:, :2])
    narrow = nat.DeviceDataset.from_numpy(X[:, :2], np.zeros(len(X)), ctx)
    with pytest.raises(sb.IllegalArgumentException):
        nat.predict_stacked(ctx, base, good, narrow)
    L = nat.lib()
    out = np.zeros(len(X))
    assert L.sbag_predict_stacked(ctx.handle, None, good.handle, nat.ptr(X), len(X), F, nat.ptr(out)) == nat.SBAG_EINVAL
    assert L.sbag_predict_stacked_dataset(ctx.handle, base.handle, good.handle, None, nat.ptr(out)) == nat.SBAG_EINVAL
    # zero rows are fine, and the context still works
    assert L.sbag_predict_stacked(ctx.handle, base.handle, good.handle, nat.ptr(X), 0, F, nat.ptr(out)) == nat.SBAG_OK
    assert not out.any()
    assert np.array_equal(bits(nat.predict_stacked(ctx, base, good, X)), bits(expected["edges_n257:host"]))
    for o in (two, short, long_, past, ds, narrow, base, good):
        o.free()
