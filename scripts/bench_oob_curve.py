#!/usr/bin/env python3
"""Staged evaluation (sbag_eval_staged: the out-of-bag score after every learner) against
two things measured in the same run:

  staged    nat.eval_staged: sampler into the workspace + k_eval_staged + k_stage_fold,
            trees x 32 bytes to the host
  (a) oob   one plain nat.predict_oob call: the same sampler and the same walks, one
            aggregation at the end (the floor of the staged pass), 12 N bytes to the host
  (b) composed  the path the entry points allowed before: nat.sample (counts to the host,
            L x N bytes), every tree's fp64 prediction to the host (predict_dataset_device
            OUT_VOTES, 8 L N bytes), and a NumPy loop over the learners keeping the running
            sum (or the class counters and the running first-to-max mode) and scoring each
            prefix

Default shape C3: 10M x 100 synthetic rows, 128 depth-8 trees, P = 128, regression
(CLASSES=n for the gini variant; ROWS / LEARNERS / DEPTH / PARTS / REPS to resize).  The
composed path holds 9 L N bytes on the host, so it runs on the first COMPOSED_ROWS rows
(default 1M; a dataset of that many rows of the same generator, the same forest) and its time
is scaled by ROWS / COMPOSED_ROWS: every step of it is linear in the rows.  Its curve is
compared with the staged call's on those rows (covered / correct equal, the sums to rounding:
NumPy sums in another order).  One fit, one warm-up of each path, then REPS (>= 5) timed
repeats alternating staged and (a), COMPOSED_REPS (default 2) of (b); host clock around calls
that end synchronized.  Prints one JSON line."""
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
NC = min(N, int(os.environ.get("COMPOSED_ROWS", 1_000_000)))
L = int(os.environ.get("LEARNERS", 128))
C = int(os.environ.get("CLASSES", 0))
P = int(os.environ.get("PARTS", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(5, int(os.environ.get("REPS", 5)))
CREPS = max(1, int(os.environ.get("COMPOSED_REPS", 2)))
SEED = 42087812 if C else -1395689524
AGG = nat.AGG_MODE if C else nat.AGG_MEAN

ctx = nat.Context(0)
dev = torch.device("cuda", 0)
ds = nat.DeviceDataset.synthetic(N, 100, seed=20261015, num_classes=C, ctx=ctx)
part = [int(round(i * N / P)) for i in range(P + 1)]
forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L,
                 partition_offsets=part, max_depth=DEPTH, max_bins=32,
                 impurity=nat.IMPURITY_GINI if C else nat.IMPURITY_VARIANCE)
small = nat.DeviceDataset.synthetic(NC, 100, seed=20261015, num_classes=C, ctx=ctx)
part_c = [int(round(i * NC / P)) for i in range(P + 1)]
y_c = small.labels()
votes = torch.empty((L, NC), dtype=torch.float64, device=dev)
torch.cuda.synchronize(dev)
KW = dict(replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L, agg=AGG)


def staged(d=ds, p=part):
    return nat.eval_staged(ctx, forest, d, partition_offsets=p, **KW)


def oob():
    return nat.predict_oob(ctx, forest, ds, partition_offsets=part, **KW)


def composed():
    counts = nat.sample(ctx, True, 1.0, SEED, 0, L, NC, part_c)
    nat.predict_dataset_device(ctx, forest, small, nat.OUT_VOTES, 8, votes.data_ptr())
    torch.cuda.synchronize(dev)
    pt = votes.cpu().numpy()
    out = np.zeros(L, nat.STAGE_DTYPE)
    n = np.zeros(NC, np.int64)
    if C:
        rows = np.arange(NC)
        cnt = np.zeros((C, NC), np.int32)
        best = np.zeros(NC, np.int32)
        acc = np.full(NC, np.nan)
        for i in range(L):
            o = counts[i] == 0
            v = pt[i].astype(np.int64)
            k = cnt[v, rows] + o
            cnt[v, rows] = k
            upd = o & (k > best)
            best = np.where(upd, k, best)
            acc = np.where(upd, pt[i], acc)
            n += o
            out[i] = (int((n > 0).sum()), int((acc == y_c).sum()), 0.0, 0.0)
    else:
        s = np.zeros(NC)
        for i in range(L):
            o = counts[i] == 0
            s = np.where(o, s + pt[i], s)
            n += o
            cov = n > 0
            e = s[cov] / n[cov] - y_c[cov]
            out[i] = (int(cov.sum()), 0, float(np.sum(e * e)), float(np.sum(np.abs(e))))
    return out


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


_, curve = timed(staged)
timed(oob)
_, want = timed(composed)
got = staged(small, part_c)
agree = bool(np.array_equal(got["covered"], want["covered"]) and np.array_equal(got["correct"], want["correct"])
             and np.allclose(got["sum_se"], want["sum_se"], rtol=1e-11, atol=0)
             and np.allclose(got["sum_ae"], want["sum_ae"], rtol=1e-11, atol=0))
t_s, t_a, t_b = [], [], []
for _ in range(REPS):
    t_a.append(timed(oob)[0])
    t_s.append(timed(staged)[0])
for _ in range(CREPS):
    t_b.append(timed(composed)[0] * (N / NC))


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


m = sb.staged_metrics(curve, N, bool(C))
print(json.dumps({"rows": N, "trees": L, "classes": C, "depth": DEPTH, "partitions": P, "reps": REPS,
                  "staged": spread(t_s), "oob": spread(t_a),
                  "composed_scaled": spread(t_b), "composed_rows": NC, "composed_reps": CREPS,
                  "staged_over_oob": round(statistics.median(t_s) / statistics.median(t_a), 4),
                  "staged_over_composed": round(statistics.median(t_s) / statistics.median(t_b), 5),
                  "composed_agrees": agree, "metric": m["metric"],
                  "first_value": float(m["values"][0]), "last_value": float(m["values"][-1]),
                  "first_coverage": float(m["coverage"][0]), "last_coverage": float(m["coverage"][-1])}))
forest.free()
small.free()
ds.free()
ctx.close()
