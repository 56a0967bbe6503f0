#!/usr/bin/env python3
"""Top-k neighbours by forest proximity on the C3 forest (128 depth-8 trees on 100 features,
fitted as scripts/bench_proximity.py fits it), resident rows, in one run:

  whole call   nat.proximity_topk_dataset of NC x NC (8 192) rows, k = 10, against the composed
               path at the same size: nat.proximity_dataset, then NumPy's argpartition and a
               sort of the kept columns under the same key.  The two alternate, REPS times each,
               host clock around calls that end with their results on the host; the results are
               compared.
  pair kernel  NQ (1 000 000) query rows x NC references for every k of KS (1, 10, 64), and one
               moments call of the same shape: the yardstick k_prox_tiled<u8, true>.
  run split    SPLIT_Q (256) query rows x SPLIT_R (1 000 000) references, k = 10.

Writes OUT/bench_topk_c3.json (OUT defaults to profiles/proximity) and, unless TRACE=0, starts
itself once more under `rocprofv3 --kernel-trace --stats` (PROFILE=1: the pair-kernel and
run-split calls once after a warm-up), keeps the statistics as OUT/kernel_stats_topk_c3.csv and
reads the kernels' times from them.  pairs/s = query rows x reference rows / kernel time."""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native

NC = int(os.environ.get("COUNT_ROWS", 8192))
NQ = int(os.environ.get("QUERY_ROWS", 1_000_000))
SPLIT_Q, SPLIT_R = int(os.environ.get("SPLIT_Q", 256)), int(os.environ.get("SPLIT_R", 1_000_000))
NFIT = int(os.environ.get("FIT_ROWS", 1_000_000))
KS = [int(v) for v in os.environ.get("KS", "1,10,64").split(",")]
F, L, DEPTH, GROUPS, PARTS = 100, int(os.environ.get("TREES", 128)), int(os.environ.get("DEPTH", 8)), 5, 128
REPS = max(3, int(os.environ.get("REPS", 5)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
OUT = os.path.abspath(os.environ.get("OUT", os.path.join(ROOT, "profiles", "proximity")))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def composed(k):
    cnt = nat.proximity_dataset(ctx, forest, ref, ref)
    key = cnt.astype(np.int64) * 2**32 + (2**32 - 1 - np.arange(cnt.shape[1]))
    part = np.argpartition(-key, k - 1, axis=1)[:, :k]
    order = np.argsort(-np.take_along_axis(key, part, 1), axis=1)
    idx = np.take_along_axis(part, order, 1)
    return idx.astype(np.int32), np.take_along_axis(cnt, idx, 1)


ctx = nat.Context(0)
fit_ds = nat.DeviceDataset.synthetic(NFIT, F, seed=20261015, num_classes=0, ctx=ctx)
forest = nat.fit(ctx, fit_ds, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE, replacement=True,
                 sample_ratio=1.0, seed=1234, learner_begin=0, learner_end=L,
                 partition_offsets=[NFIT * i // PARTS for i in range(PARTS + 1)])
ref = nat.DeviceDataset.from_numpy(fit_ds.features(0, NC), np.zeros(NC), ctx)
fit_ds.free()
res = {"features": F, "trees": L, "depth": DEPTH, "reps": REPS}

if not PROFILE:
    new, old = nat.proximity_topk_dataset(ctx, forest, ref, ref, 10), composed(10)  # warm-up of both
    t_new, t_old = [], []
    for _ in range(REPS):
        t_new.append(timed(lambda: nat.proximity_topk_dataset(ctx, forest, ref, ref, 10))[0])
        t_old.append(timed(lambda: composed(10))[0])
    res["whole_call"] = {"nq": NC, "nr": NC, "k": 10, "topk": spread(t_new), "composed": spread(t_old),
                         "equal": bool(np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]))}
    print(f"# whole call: {res['whole_call']}", file=sys.stderr, flush=True)

q = nat.DeviceDataset.synthetic(NQ, F, seed=7, num_classes=0, ctx=ctx)
res["pair_kernel"] = {"nq": NQ, "nr": NC, "calls": {}}
for k in KS:
    nat.proximity_topk_dataset(ctx, forest, q, ref, k)  # warm-up
    t = [timed(lambda: nat.proximity_topk_dataset(ctx, forest, q, ref, k))[0] for _ in range(1 if PROFILE else REPS)]
    res["pair_kernel"]["calls"][f"k={k}"] = spread(t)
groups = (np.arange(NC) * 7 % GROUPS).astype(np.int32)
nat.proximity_moments_dataset(ctx, forest, q, ref, groups, GROUPS)
t = [timed(lambda: nat.proximity_moments_dataset(ctx, forest, q, ref, groups, GROUPS))[0]
     for _ in range(1 if PROFILE else REPS)]
res["pair_kernel"]["calls"]["moments"] = spread(t)
big = nat.DeviceDataset.synthetic(SPLIT_R, F, seed=9, num_classes=0, ctx=ctx)
few = nat.DeviceDataset.from_numpy(q.features(0, SPLIT_Q), np.zeros(SPLIT_Q), ctx)
q.free()
nat.proximity_topk_dataset(ctx, forest, few, big, 10)
t = [timed(lambda: nat.proximity_topk_dataset(ctx, forest, few, big, 10))[0] for _ in range(1 if PROFILE else REPS)]
res["run_split"] = {"nq": SPLIT_Q, "nr": SPLIT_R, "k": 10, "call": spread(t)}
for d in (big, few, ref):
    d.free()
forest.free()
ctx.close()
if PROFILE:
    sys.exit(0)
os.makedirs(OUT, exist_ok=True)
if os.environ.get("TRACE", "1") == "1":  # a fresh process under the profiler: kernel times only
    tmp = os.path.join(OUT, "trace_topk_tmp")
    subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "topk", "--output-format", "csv",
                           "--", sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PROFILE="1"))
    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]
    shutil.copy(stats, os.path.join(OUT, "kernel_stats_topk_c3.csv"))
    trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
    with open(trace) as fh:  # the launches in order: two calls (warm-up, timed) of every shape
        launches = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                    for r in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))]
    shutil.rmtree(tmp)
    topk = [ns for nm, ns in launches if "k_prox_topk" in nm]
    mom_ns = sum(ns for nm, ns in launches if "k_prox_tiled" in nm)
    res["kernel"] = {"moments": {"kernel_ms_total": round(mom_ns * 1e-6, 3), "pairs_per_s": 2 * NQ * NC / (mom_ns * 1e-9)}}
    # the launches in order: every k of KS (a warm-up and a timed call, one launch a query batch),
    # then the run-split shape, whose few query rows are one batch: two launches
    per_k, rest = divmod(len(topk) - 2, len(KS))
    if rest == 0 and per_k > 0:
        for i, k in enumerate(KS):
            ns = sum(topk[per_k * i:per_k * (i + 1)])
            rate = 2 * NQ * NC / (ns * 1e-9)
            res["kernel"][f"k={k}"] = {"kernel_ms_total": round(ns * 1e-6, 3), "launches": per_k, "pairs_per_s": rate,
                                       "share_of_moments_rate": round(rate / res["kernel"]["moments"]["pairs_per_s"], 3)}
        ns = sum(topk[per_k * len(KS):])
        res["kernel"]["run_split"] = {"kernel_ms_total": round(ns * 1e-6, 3),
                                      "pairs_per_s": 2 * SPLIT_Q * SPLIT_R / (ns * 1e-9)}
    mrg = sum(ns for nm, ns in launches if "k_topk_merge" in nm)
    res["kernel"]["k_topk_merge_ms_total"] = round(mrg * 1e-6, 3)
with open(os.path.join(OUT, "bench_topk_c3.json"), "w") as fh:
    fh.write(json.dumps(res) + "\n")
print(json.dumps(res), flush=True)
