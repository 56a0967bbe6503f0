#!/usr/bin/env python3
"""Out-of-bag predictions under permuted features (sbag_predict_oob_permuted) against one
plain out-of-bag pass (sbag_predict_oob) of the same process:

  fused     the default path: k_predict_oob_perm, one pass per feature batch
  fallback  SBAG_OOBP_FORCE_FALLBACK=1: a column-substituted copy and one plain pass of the
            global-memory walk per feature
  plain     sbag_predict_oob: what one permuted feature costs without this entry point (plus
            an ingest of the permuted data)

Default shape C3: 10M x 100 synthetic rows, 128 depth-8 trees, P = 128, regression
(CLASSES=n for the gini variant; ROWS / LEARNERS / DEPTH / PARTS to resize), for FEATURES =
16 and 64 permuted features (the first K features, one permutation each).  The C entry
points are called on preallocated, touched host buffers, so the host clock around a call
(each ends synchronized with its results on the host) holds the sampler, the kernels and
the transfers (4 N bytes of source rows up and 8 N bytes of predictions down per feature),
not page faults of fresh result arrays.  One warm-up of each path and shape, then REPS (>= 5)
timed repeats of fused and plain, alternating, and FALLBACK_REPS (>= 3) of the fallback.
Prints one JSON line: median / min / max of every path, the fused and fallback time per
feature, their ratios to the plain pass, and whether the fused and fallback bytes agree.
KERNELS_ONLY=1 runs one warm-up and one repeat of the fused and plain paths only (for a
kernel trace of its own)."""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
L = int(os.environ.get("LEARNERS", 128))
C = int(os.environ.get("CLASSES", 0))
P = int(os.environ.get("PARTS", 128))
F = 100
DEPTH = int(os.environ.get("DEPTH", 8))
KS = [int(k) for k in os.environ.get("FEATURES", "16,64").split(",")]
KERNELS_ONLY = os.environ.get("KERNELS_ONLY", "0") != "0"
REPS = 1 if KERNELS_ONLY else max(5, int(os.environ.get("REPS", 5)))
FB_REPS = 0 if KERNELS_ONLY else max(3, int(os.environ.get("FALLBACK_REPS", 3)))
SEED = 42087812 if C else -1395689524
AGG = nat.AGG_MODE if C else nat.AGG_MEAN

ctx = nat.Context(0)
ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=C, ctx=ctx)
part = np.array([int(round(i * N / P)) for i in range(P + 1)], np.int64)
forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L,
                 partition_offsets=part, max_depth=DEPTH, max_bins=32,
                 impurity=nat.IMPURITY_GINI if C else nat.IMPURITY_VARIANCE)
sp = nat.SamplerParams(1, 0, 1.0, SEED, 0, L)
lib = nat.lib()
KMAX = max(KS)
feats = np.arange(KMAX, dtype=np.int32) % F
rng = np.random.default_rng(20261019)
src = np.stack([rng.permutation(N).astype(np.int32) for _ in range(KMAX)])
out = np.zeros((KMAX, N), np.float64)
out_fb = np.zeros((KMAX, N), np.float64)
base = np.zeros(N, np.float64)
n_oob = np.zeros(N, np.int32)
plain_out = np.zeros(N, np.float64)
plain_n = np.zeros(N, np.int32)


def permuted(k, dst):
    nat.check(lib.sbag_predict_oob_permuted(ctx.handle, forest.handle, ds.handle, ctypes.byref(sp), nat.ptr(part),
                                            P, AGG, nat.ptr(feats), k, nat.ptr(src), nat.ptr(dst), nat.ptr(base),
                                            nat.ptr(n_oob)))


def plain():
    nat.check(lib.sbag_predict_oob(ctx.handle, forest.handle, ds.handle, ctypes.byref(sp), nat.ptr(part), P, AGG,
                                   nat.ptr(plain_out), nat.ptr(plain_n)))


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t0) * 1e3


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


res = {"rows": N, "trees": L, "classes": C, "depth": DEPTH, "partitions": P, "reps": REPS,
       "fallback_reps": FB_REPS, "features": {}}
plain()
t_plain = []
for k in KS:
    permuted(k, out)  # warm-up of the shape
    t_f = []
    for _ in range(REPS):
        t_f.append(timed(permuted, k, out))
        t_plain.append(timed(plain))
    r = {"fused": spread(t_f), "fused_ms_per_feature": round(statistics.median(t_f) / k, 3)}
    if FB_REPS:
        os.environ["SBAG_OOBP_FORCE_FALLBACK"] = "1"
        permuted(k, out_fb)
        t_b = [timed(permuted, k, out_fb) for _ in range(FB_REPS)]
        del os.environ["SBAG_OOBP_FORCE_FALLBACK"]
        r["fallback"] = spread(t_b)
        r["fallback_ms_per_feature"] = round(statistics.median(t_b) / k, 3)
        r["fused_equals_fallback"] = bool(np.array_equal(out[:k].view(np.int64), out_fb[:k].view(np.int64)))
    r["baseline_equals_plain"] = bool(base.tobytes() == plain_out.tobytes() and n_oob.tobytes() == plain_n.tobytes())
    covered = n_oob > 0
    r["rows_changed_mean"] = float(np.mean([(out[i][covered] != base[covered]).mean() for i in range(min(k, 4))]))
    res["features"][str(k)] = r
res["plain_oob"] = spread(t_plain)
for k in KS:
    r = res["features"][str(k)]
    r["fused_per_feature_over_plain"] = round(r["fused_ms_per_feature"] / res["plain_oob"]["median_ms"], 4)
    if FB_REPS:
        r["fallback_per_feature_over_plain"] = round(r["fallback_ms_per_feature"] / res["plain_oob"]["median_ms"], 4)
res["coverage"] = float((n_oob > 0).mean())
print(json.dumps(res))
forest.free()
ds.free()
ctx.close()
