#!/usr/bin/env python3
"""Ingest of host data into an sbag_dataset: the device path (sbag_dataset_create_device /
_create_columns_device: k_ingest_distinct, k_ingest_compact, k_ingest_rank, k_ingest_encode)
against the host path (sbag_dataset_create / _create_columns), in one process on the same host
matrix.

Shapes, ROWS x 100 (default 10M; a run below that says so in "rows" and is not scaled):
  rows32      dense fp64 rows, 32 distinct values a feature (the C3 matrix on the host): u8 codes,
              the LDS search
  rows50k     dense fp64 rows, about 50 000 distinct values a feature: u16 codes, the probe
  cols32, cols50k   the same values as fp32 columns

Per shape: one warm-up call of each path, then REPS timed calls of each, alternating, host clock
around calls that return with the dataset resident (whole-call time); one more device call under
SBAG_PROFILE_HOST=1, whose stderr line gives the device time of the raw upload and of each kernel
from events; and the two datasets' codes, dictionaries and labels compared byte for byte.
"mandatory_bytes" is what each kernel has to move (raw values read, codes written), computed from
the shape.  Prints one JSON line per shape."""
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
F = 100
REPS = max(2, int(os.environ.get("REPS", 3)))
SHAPES = os.environ.get("SHAPES", "rows32,rows50k,cols32,cols50k").split(",")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 1), "min_ms": round(min(t), 1), "max_ms": round(max(t), 1)}


def matrix(distinct, seed):
    rng = np.random.default_rng(seed)
    X = np.empty((N, F), np.float64)
    for r0 in range(0, N, 1_000_000):
        blk = X[r0:r0 + 1_000_000]
        blk[:] = rng.integers(0, distinct, blk.shape) * (1.0 if distinct <= 256 else 0.25)
    return X


def profiled(fn):
    """fn() with the library's SBAG_PROFILE_HOST line (written to fd 2) captured"""
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.environ["SBAG_PROFILE_HOST"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            fn().free()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("SBAG_PROFILE_HOST")
        tmp.seek(0)
        line = [ln for ln in tmp.read().decode().splitlines() if ln.startswith("ingest device:")][-1]
    return {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+)", line.split(":", 1)[1])}


def image(ds):
    codes = np.zeros(ds.codes_nbytes(), np.uint8)
    d, off, y = ds.export(codes.ctypes.data)
    return codes, d.view(np.uint64), off, y


ctx = nat.Context(0)
y = (np.arange(N) % 7).astype(np.float64)
for shape in SHAPES:
    distinct = 32 if shape.endswith("32") else 50_000
    X = matrix(distinct, seed=distinct)
    if shape.startswith("rows"):
        make = lambda ingest: nat.DeviceDataset.from_numpy(X, y, ctx, ingest=ingest)  # noqa: E731
        elt = 8
    else:
        cols = [np.ascontiguousarray(X[:, j], np.float32) for j in range(F)]
        del X
        make = lambda ingest: nat.DeviceDataset.from_columns(cols, y, ctx, ingest=ingest)  # noqa: E731
        elt = 4
    host, dev = make("host"), make("device")  # the warm-up calls
    same = dev.ingest_path == "device" and all(np.array_equal(a, b) for a, b in zip(image(host), image(dev)))
    _, _, S, cb, dv = dev.layout()
    host.free()
    dev.free()
    th, td = [], []
    for _ in range(REPS):
        for ingest, t in (("host", th), ("device", td)):
            ms, ds = timed(lambda: make(ingest))
            ds.free()
            t.append(ms)
    prof = profiled(lambda: make("device"))
    raw, codes = N * F * elt, N * S * cb
    print(json.dumps({"shape": shape, "rows": N, "features": F, "dict_values": dv, "code_bytes": cb,
                      "device_equals_host": bool(same), "host": spread(th), "device": spread(td),
                      "speedup_median": round(statistics.median(th) / statistics.median(td), 2),
                      "device_profile": prof,
                      "mandatory_bytes": {"upload": raw, "distinct": raw, "encode": raw + codes}}), flush=True)
ctx.close()
