#!/usr/bin/env python3
"""Per-row feature contributions (TreeSHAP) of a bagged regression forest, in one run:

  tiled      nat.predict_contributions_dataset over resident rows (k_contrib_tiled), at every row
             count of ROWS (default 100 000 and 1 000 000): the whole call, results on the host
  general    the same call under SBAG_CONTRIB_FORCE_FALLBACK=1 (k_contrib_walk), same rows; the
             result is compared byte for byte with the tiled one
  baseline   tests/contrib_ref.restated, the rule in NumPy on one CPU thread, over BASELINE_ROWS
             (10 000; 0 skips it) rows: the only baseline there is.  Reported at its own row count,
             not scaled.  GENERAL=0 skips the general path.

Shape: the C3 regression forest: sbag_dataset_synthetic max(ROWS) x 100, TREES (128) depth-DEPTH (8)
trees fitted on PARTS (128) equal partitions; the smaller row counts are the first rows of the
same data in datasets of their own.  One warm-up of every path, then REPS timed repeats, host
clock around calls that end with their results on the host.  `fp64_ops` counts the rule's fp64
operations (sbag.h) per row from the path table's m, once with every o_k = 1 and once with
every o_k = 0: the true count lies between.  Prints one JSON line.  Kernel (device) times are not
taken here: run the script under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (one call a
path and row count after a warm-up, no baseline)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
import contrib_ref  # noqa: E402

ROWS = sorted(int(v) for v in os.environ.get("ROWS", "100000,1000000").split(","))
NBASE = int(os.environ.get("BASELINE_ROWS", 10_000))
F = 100
L = int(os.environ.get("TREES", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(3, int(os.environ.get("REPS", 3)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
GENERAL = os.environ.get("GENERAL", "1") == "1"  # 0: the tiled path only
KNOB = "SBAG_CONTRIB_FORCE_FALLBACK"
PARTS = int(os.environ.get("PARTS", 128))
N = ROWS[-1]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def ops_per_row(ms):
    """fp64 operations of sbag.h's rule for one row over paths of m distinct features: (every
    o_k = 1, every o_k = 0).  Extension step u: 2 multiplications for j = 0 .. u, and with o_u = 1
    a multiplication and an addition for j = 1 .. u.  Unwound sum of an element: 5 operations a
    step with o_k = 1, 3 with o_k = 0, m steps; d_k (a subtraction with o_k = 1) and the
    accumulation (2 multiplications, 1 addition)."""
    one = sum(sum(2 * (u + 1) + 2 * u for u in range(1, m + 1)) + m * (5 * m + 4) for m in ms)
    zero = sum(sum(2 * (u + 1) for u in range(1, m + 1)) + m * (3 * m + 3) for m in ms)
    return one, zero


ctx = nat.Context(0)
ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=0, ctx=ctx)
forest = nat.fit(ctx, ds, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE, replacement=True,
                 sample_ratio=1.0, seed=1234, learner_begin=0, learner_end=L,
                 partition_offsets=[N * i // PARTS for i in range(PARTS + 1)])
trees, stats = zip(*[forest.tree(t) for t in range(L)])
subs = [forest.subspace(t) for t in range(L)]
ms = [len(els) for t in range(L) for _, els in contrib_ref.paths(trees[t], stats[t], subs[t])]
one, zero = ops_per_row(ms)
res = {"features": F, "trees": L, "depth": DEPTH, "leaves": len(ms), "max_m": max(ms), "mean_m": round(float(np.mean(ms)), 2),
       "fp64_ops_per_row": {"every_o_1": one, "every_o_0": zero}, "runs": []}
for n in ROWS:
    part = ds if n == N else nat.DeviceDataset.from_numpy(ds.features(0, n), np.zeros(n), ctx)
    call = lambda: nat.predict_contributions_dataset(ctx, forest, part)  # noqa: E731
    run = {"rows": n}
    for name, force in (("tiled", None), ("general", "1"))[: 2 if GENERAL else 1]:
        os.environ.pop(KNOB, None) if force is None else os.environ.__setitem__(KNOB, force)
        out = call()  # warm-up
        if PROFILE:
            call()
            continue
        run[name] = spread([timed(call)[0] for _ in range(REPS)])
        if force is None:
            first = out
            pred = nat.predict_dataset(ctx, forest, part, nat.AGG_MEAN)
            run["row_sum_minus_predict_max"] = float(np.abs(out.sum(axis=1) - pred).max())
        else:
            run["general_equals_tiled"] = bool(out.tobytes() == first.tobytes())
    os.environ.pop(KNOB, None)
    run["result_bytes"] = 8 * n * (F + 1)
    res["runs"].append(run)
    print(f"# {n} rows: {run}", file=sys.stderr, flush=True)
    if part is not ds:
        part.free()
if not PROFILE and NBASE > 0:
    X = ds.features(0, NBASE)
    want = nat.predict_contributions(ctx, forest, X)

    def progress_trees():
        out = np.zeros((NBASE, F + 1))
        for t0 in range(0, L, 16):  # restated divides by the trees it is given: undo, sum, divide once
            k = len(trees[t0:t0 + 16])
            out += contrib_ref.restated(trees[t0:t0 + 16], stats[t0:t0 + 16], subs[t0:t0 + 16], X) * k
            print(f"# baseline: {t0 + k} trees", file=sys.stderr, flush=True)
        return out / L

    t_b, base = timed(progress_trees)
    res["baseline_numpy"] = {"rows": NBASE, "ms": round(t_b, 1), "threads": 1,
                             "max_abs_difference_from_device": float(np.abs(base - want).max())}
print(json.dumps(res), flush=True)
forest.free()
ds.free()
ctx.close()
