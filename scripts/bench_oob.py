#!/usr/bin/env python3
"""Out-of-bag prediction (sbag_predict_oob) against the baseline composed from the entry
points that existed before it, in one run:

  fused     nat.predict_oob: sampler into the workspace + k_predict_oob, results on the host
  composed  nat.sample (counts to the host, R x N bytes) -> counts back on the device,
            predict_dataset_device(OUT_VOTES, 8) (every tree's fp64 prediction, L x N x 8
            bytes) -> masked ordered aggregation in torch on the device, results on the host

Default shape C3: 10M x 100 synthetic rows, 128 depth-8 trees, P = 128, regression
(CLASSES=n for the gini variant; ROWS / LEARNERS / DEPTH / PARTS / REPS to resize).  One fit,
one warm-up of each path, then REPS (>= 5) timed repeats alternating the two paths; host
clock around calls that end synchronized (both paths end with their results on the host).
Prints one JSON line: median / min / max of both paths, their ratio, and as context the
fit's sample_ms and the plain predict_dataset time of the same run."""
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
L = int(os.environ.get("LEARNERS", 128))
C = int(os.environ.get("CLASSES", 0))
P = int(os.environ.get("PARTS", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(5, int(os.environ.get("REPS", 5)))
SEED = 42087812 if C else -1395689524
AGG = nat.AGG_MODE if C else nat.AGG_MEAN

ctx = nat.Context(0)
dev = torch.device("cuda", 0)
ds = nat.DeviceDataset.synthetic(N, 100, seed=20261015, num_classes=C, ctx=ctx)
part = [int(round(i * N / P)) for i in range(P + 1)]
forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L,
                 partition_offsets=part, max_depth=DEPTH, max_bins=32,
                 impurity=nat.IMPURITY_GINI if C else nat.IMPURITY_VARIANCE)
sample_ms = forest.timing()["sample_ms"]
votes = torch.empty((L, N), dtype=torch.float64, device=dev)
torch.cuda.synchronize(dev)


def fused():
    return nat.predict_oob(ctx, forest, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0,
                           learner_end=L, partition_offsets=part, agg=AGG)


def composed():
    counts = torch.from_numpy(nat.sample(ctx, True, 1.0, SEED, 0, L, N, part)).to(dev)
    torch.cuda.synchronize(dev)
    nat.predict_dataset_device(ctx, forest, ds, nat.OUT_VOTES, 8, votes.data_ptr())
    n_oob = torch.zeros(N, dtype=torch.int32, device=dev)
    if C:
        rows = torch.arange(N, device=dev)
        cnt = torch.zeros((C, N), dtype=torch.int32, device=dev)
        best = torch.zeros(N, dtype=torch.int32, device=dev)
        acc = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
        for i in range(L):
            oob = counts[i] == 0
            v = votes[i].to(torch.int64)
            k = cnt[v, rows] + oob.to(torch.int32)
            cnt[v, rows] = k
            upd = oob & (k > best)
            best = torch.where(upd, k, best)
            acc = torch.where(upd, votes[i], acc)
            n_oob += oob
        pred = acc
    else:
        s = torch.zeros(N, dtype=torch.float64, device=dev)
        for i in range(L):
            oob = counts[i] == 0
            s = torch.where(oob, s + votes[i], s)
            n_oob += oob
        pred = torch.where(n_oob > 0, s / n_oob.to(torch.float64), torch.full_like(s, float("nan")))
    return pred.cpu().numpy(), n_oob.cpu().numpy()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


_, a = timed(fused)
_, b = timed(composed)
equal = bool(np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1]))
t_f, t_c, t_p = [], [], []
for _ in range(REPS):
    t_c.append(timed(composed)[0])
    t_f.append(timed(fused)[0])
    t_p.append(timed(lambda: nat.predict_dataset(ctx, forest, ds, AGG))[0])


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


print(json.dumps({"rows": N, "trees": L, "classes": C, "depth": DEPTH, "partitions": P, "reps": REPS,
                  "fused": spread(t_f), "composed": spread(t_c),
                  "fused_over_composed": round(statistics.median(t_f) / statistics.median(t_c), 4),
                  "fit_sample_ms": round(sample_ms, 3), "predict_dataset": spread(t_p),
                  "outputs_equal": equal, "coverage": float((a[1] > 0).mean())}))
forest.free()
ds.free()
ctx.close()
