"""GPU: the ingest on the device (sbag_dataset_create_device / _create_columns_device,
sbag_ingest.hip) builds the dataset the host ingest builds, byte for byte.  The reference is
NumPy: per column np.unique(col + 0.0) and np.searchsorted; every code byte (padding columns
included), the dictionaries as uint64, the labels and features() are compared exactly, and
every case asserts the path taken so that a silent fallback cannot pass."""
import os

import numpy as np
import pytest

from conftest import DATA

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def _check(ds, X, y, path="device"):
    X = np.asarray(X, np.float64)
    assert ds.ingest_path == path
    n, f, s, cb, _ = ds.layout()
    d = [np.unique(X[:, j] + 0.0) for j in range(f)]
    widest = max(len(v) for v in d)
    assert (n, f, cb) == (*X.shape, 1 if widest <= 256 else 2 if widest <= 65536 else 4)
    want = np.zeros((n, s), {1: np.uint8, 2: np.uint16, 4: np.uint32}[cb])
    for j in range(f):
        want[:, j] = np.searchsorted(d[j], X[:, j] + 0.0)
    got = np.full_like(want, 0xAB)
    dv, off, yy = ds.export(got.ctypes.data)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(dv.view(np.uint64), np.concatenate(d).view(np.uint64))
    assert off.tolist() == np.cumsum([0] + [len(v) for v in d]).tolist()
    assert np.array_equal(yy, y) and np.array_equal(ds.features(), X)
    return got.tobytes()


def _data(n, f, seed=0):
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(size=(n, f)), 1), rng.integers(0, 3, n).astype(np.float64)


@pytest.mark.parametrize("n,f", [(1, 1), (257, 17), (1000, 64), (1000, 65), (513, 130)])
def test_dense_rows_at_the_tile_and_stride_edges(ctx, n, f):
    X, y = _data(n, f)
    _check(nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device"), X, y)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
def test_columns_of_every_type(ctx, dtype):
    X, y = _data(257, 17)
    cols = [(np.abs(X[:, j] * 10) % 40 if dtype == np.uint8 else X[:, j]).astype(dtype) for j in range(17)]
    ds = nat.DeviceDataset.from_columns(cols, y, ctx, ingest="device")
    _check(ds, np.stack(cols, 1), y)


@pytest.mark.parametrize("k", [256, 257, 65536, 65537])
def test_dictionary_sizes_at_the_width_and_probe_switches(ctx, k):
    """A constant column, one of exactly k values, one of 5: u8 -> u16 at 257, the LDS search ->
    the probe at 257, a set at its full load at 65 536; 65 537 takes the host ingest (u32)."""
    n = 70000
    rng = np.random.default_rng(k)
    X = np.stack([np.full(n, 3.25), rng.permutation(np.arange(n) % k) * 0.5 - 100.0,
                  rng.integers(-2, 3, n) * 1.5], 1)
    y = np.arange(n) % 2.0
    _check(nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device"), X, y,
           "host" if k > 65536 else "device")


def test_value_edges(ctx):
    """+0.0 and -0.0 are one entry (and not code 0: there are negatives), infinities,
    subnormals, neighbours one ulp apart, the ends of the range."""
    v = np.array([0.0, -0.0, -1.5, 2.0, np.inf, -np.inf, 5e-324, -5e-324, 1.0, np.nextafter(1.0, 2.0),
                  1e308, -1e308, -0.0, 0.0])
    X = np.stack([v, v[::-1], np.abs(v)], 1)
    y = np.arange(len(v), dtype=np.float64)
    _check(nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device"), X, y)
    _check(nat.DeviceDataset.from_columns(list(X.T), y, ctx, ingest="device"), X, y)


@pytest.mark.parametrize("resident", ["1", "0"])
def test_several_batches_give_the_one_batch_bytes(ctx, monkeypatch, resident):
    """4 500 rows in batches of 1 000 (the last one short, a value first seen in it), with the
    raw rows kept on the device between the passes or uploaded twice."""
    X, y = _data(4500, 17, seed=3)
    X[4400, 3] = 99.5
    one = _check(nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device"), X, y)
    monkeypatch.setenv("SBAG_INGEST_BATCH_ROWS", "1000")
    monkeypatch.setenv("SBAG_INGEST_RESIDENT", resident)
    assert _check(nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device"), X, y) == one
    cols = [np.ascontiguousarray(X[:, j]) for j in range(17)]
    assert _check(nat.DeviceDataset.from_columns(cols, y, ctx, ingest="device"), X, y) == one


def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    monkeypatch.setenv("SBAG_INGEST_BATCH_ROWS", "1000")
    X, y = _data(4500, 17)
    with pytest.raises(sb.IllegalArgumentException):
        nat.DeviceDataset.from_numpy(X, y, ctx, ingest="gpu")
    X[-1, -1] = np.nan
    with pytest.raises(sb.IllegalArgumentException, match="NaN feature value"):
        nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device")
    X[-1, -1] = 0.0
    _check(nat.DeviceDataset.from_numpy(X[:50], y[:50], ctx, ingest="device"), X[:50], y[:50])


def test_fit_on_the_device_ingested_dataset_is_the_same_forest(ctx):
    X, y = sb.load_libsvm(os.path.join(DATA, "vehicle.svm"))
    kw = dict(replacement=True, sample_ratio=0.8, seed=7, learner_begin=0, learner_end=5, max_depth=6,
              max_bins=32, impurity=nat.IMPURITY_GINI)
    a = nat.fit(ctx, nat.DeviceDataset.from_numpy(X, y, ctx), **kw)
    dd = nat.DeviceDataset.from_numpy(X, y, ctx, ingest="device")
    assert dd.ingest_path == "device"
    b = nat.fit(ctx, dd, **kw)
    assert len(a) == len(b)
    for t in range(len(a)):
        (na, sa), (nb, sb_) = a.tree(t), b.tree(t)
        assert na.tobytes() == nb.tobytes() and (sa == sb_).all(), f"tree {t}"
