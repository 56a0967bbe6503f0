#!/usr/bin/env python3
"""Stacking's two device calls against the paths composed from the calls before them, in one
process and one run:

  (a) level-1 dataset
      stacked            ds.stacked(base): sbag_dataset_create_stacked (k_stack_walk, the flags to
                         the host, k_stack_codes)
      composed           nat.predict(per_tree=True) on the host rows (K x N fp64 down), a host
                         transpose, DeviceDataset.from_numpy (sbag_dataset_create: host sort +
                         unique + binary search per value, N x S bytes up)
  (b) transform over the resident dataset
      predict_stacked    nat.predict_stacked(ctx, base, stack, ds): k_predict_stacked, N fp64 down
      composed           the same per-tree predictions and transpose, then nat.predict of the
                         stack forest on the K-column matrix

The composed paths share their first two steps, timed once per repeat; `per_tree_resident` is the
per-tree predictions taken from the resident dataset instead (predict_dataset_device, fp64 votes,
copied down): the cheapest way the earlier calls offer to get the same K x N doubles, without the
upload of the host rows.

Default shape: 10M x 100 synthetic rows, K = 8 depth-8 variance trees, a depth-5 stacker (ROWS /
TREES / DEPTH / STACK_DEPTH / REPS / COMPOSED_REPS to resize).  One warm-up of every path, then
REPS (>= 5) timed repeats alternating the paths (the composed steps, tens of seconds of host work,
COMPOSED_REPS times); host clock around calls that end with their results on the host or with a
synchronised context.  Prints one JSON line.  Kernel (device) times are not taken here: run the
script under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (after the warm-up one call of
each device path and one of each composed step) and read k_stack_walk / k_stack_codes /
k_predict_stacked and k_predict / k_quantize / k_predict_tiled there."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
F = 100
K = int(os.environ.get("TREES", 8))
DEPTH = int(os.environ.get("DEPTH", 8))
SDEPTH = int(os.environ.get("STACK_DEPTH", 5))
REPS = max(5, int(os.environ.get("REPS", 5)))
COMPOSED_REPS = max(1, int(os.environ.get("COMPOSED_REPS", 2)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
SEED = 42087812

ctx = nat.Context(0)
dev = torch.device("cuda", 0)
ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=0, ctx=ctx)
base = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=K,
               max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE)
ones = np.ones(N, np.uint8)
l1 = ds.stacked(base)
stack = nat.fit_bag(ctx, l1, ones, np.arange(K, dtype=np.int32), impurity=nat.IMPURITY_VARIANCE,
                    max_depth=SDEPTH, max_bins=32)
l1.free()
X = ds.features()   # the host rows the composed path starts from (not timed)
y = ds.labels()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stacked():
    d = ds.stacked(base)
    return d


def predict_stacked():
    return nat.predict_stacked(ctx, base, stack, ds)


def per_tree_host():
    return nat.predict(ctx, base, X, nat.AGG_MEAN, per_tree=True)[1]


def per_tree_resident():
    votes = torch.empty((K, N), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    nat.predict_dataset_device(ctx, base, ds, nat.OUT_VOTES, 8, votes.data_ptr())
    return votes.cpu().numpy()


def transpose(pt):
    return np.ascontiguousarray(pt.T)


def create(P):
    return nat.DeviceDataset.from_numpy(P, y, ctx)


def stack_predict(P):
    return nat.predict(ctx, stack, P, nat.AGG_MEAN)


def exported(d):
    n, f, s, cb, dv = d.layout()
    codes = np.zeros(n * s * cb, np.uint8)
    dd, off, yy = d.export(codes.ctypes.data)
    return (n, f, s, cb, dv), codes, dd, off, yy


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


# warm-up of every path, and the equality of what is timed
d_dev = stacked()
out_dev = predict_stacked()
pt = per_tree_host()
same_pt = bool(np.array_equal(pt, per_tree_resident()))
P = transpose(pt)
del pt
d_host = create(P)
out_host = stack_predict(P)
a, b = exported(d_dev), exported(d_host)
res = {"rows": N, "features": F, "trees": K, "depth": DEPTH, "stack_depth": SDEPTH,
       "stack_nodes": int(len(stack.tree(0)[0])), "level1_layout": list(a[0]),
       "dataset_equals_composed": bool(a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]))),
       "predict_equals_composed": bool(np.array_equal(out_dev.view(np.uint64), out_host.view(np.uint64))),
       "per_tree_resident_equals_host": same_pt}
del a, b
d_dev.free()
d_host.free()

if PROFILE:
    stacked().free()
    predict_stacked()
    P = transpose(per_tree_host())
    create(P).free()
    stack_predict(P)
    res["profile_run"] = True
else:
    t = {k: [] for k in ("stacked", "predict_stacked")}
    tc = {k: [] for k in ("per_tree_host", "per_tree_resident", "transpose", "create", "stack_predict")}
    for r in range(REPS):
        if r < COMPOSED_REPS:
            ms, pt = timed(per_tree_host)
            tc["per_tree_host"].append(ms)
            tc["per_tree_resident"].append(timed(per_tree_resident)[0])
            ms, P = timed(lambda: transpose(pt))
            tc["transpose"].append(ms)
            del pt
            ms, d = timed(lambda: create(P))
            tc["create"].append(ms)
            d.free()
            tc["stack_predict"].append(timed(lambda: stack_predict(P))[0])
        ms, d = timed(stacked)
        t["stacked"].append(ms)
        d.free()
        t["predict_stacked"].append(timed(predict_stacked)[0])
    res.update({"reps": REPS, "composed_reps": COMPOSED_REPS})
    res.update({k: spread(v) for k, v in t.items()})
    res.update({"composed_" + k: spread(v) for k, v in tc.items()})
    med = {k: statistics.median(v) for k, v in tc.items()}
    res["composed_dataset_median_ms"] = round(med["per_tree_host"] + med["transpose"] + med["create"], 3)
    res["composed_dataset_resident_median_ms"] = round(med["per_tree_resident"] + med["transpose"] + med["create"], 3)
    res["composed_predict_median_ms"] = round(med["per_tree_host"] + med["transpose"] + med["stack_predict"], 3)
    res["composed_predict_resident_median_ms"] = round(
        med["per_tree_resident"] + med["transpose"] + med["stack_predict"], 3)
print(json.dumps(res))
base.free()
stack.free()
ds.free()
ctx.close()
