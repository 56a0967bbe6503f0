#!/usr/bin/env python3
"""Per-class raw predictions (sbag_predict_oob_raw, sbag_predict_raw_dataset) against what
the entry points before them can do, in one run:

  oob_raw hard / soft   nat.predict_oob_raw: sampler into the workspace + k_proba_tiled, the
                        N x C fp64 result and n_oob on the host
  raw_dataset soft      nat.predict_raw_dataset: k_proba_tiled over every tree, N x C on the host
  composed hard         nat.sample (counts to the host, L x N bytes) + predict_dataset_device(
                        OUT_VOTES, 1) (u8 votes, L x N bytes, to the host) + a masked bincount
                        on the host: the only earlier route to out-of-bag vote counts
  oob mode              nat.predict_oob(AGG_MODE): the floor of a fused out-of-bag pass (one
                        fp64 and one int32 per row come back instead of C fp64)
  download              a device-to-host copy of 8 N C bytes (torch, pageable memory): the part
                        of the raw calls' wall time that is the result's size, not the kernel

Default shape C3: 10M x 100 synthetic rows, 5 classes, 128 depth-8 gini trees, P = 128 (ROWS /
LEARNERS / CLASSES / DEPTH / PARTS / REPS / COMPOSED_REPS to resize).  One fit, one warm-up of
every path, then REPS (>= 5) timed repeats alternating the paths (the composed baseline, tens
of seconds of host work, COMPOSED_REPS times); host clock around calls that end with their
results on the host.  Prints one JSON line.  Kernel (device) times are not taken here: run
the script under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (one call of each native
path after the warm-up, no baseline) and read k_proba_tiled / k_predict_oob there."""
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
C = int(os.environ.get("CLASSES", 5))
P = int(os.environ.get("PARTS", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(5, int(os.environ.get("REPS", 5)))
COMPOSED_REPS = max(1, int(os.environ.get("COMPOSED_REPS", 2)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
SEED = 42087812

ctx = nat.Context(0)
dev = torch.device("cuda", 0)
ds = nat.DeviceDataset.synthetic(N, 100, seed=20261015, num_classes=C, ctx=ctx)
part = [int(round(i * N / P)) for i in range(P + 1)]
forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L,
                 partition_offsets=part, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_GINI)
NC = forest.num_classes
kw = dict(replacement=True, sample_ratio=1.0, seed=SEED, learner_begin=0, learner_end=L, partition_offsets=part)


def oob_raw(kind):
    return nat.predict_oob_raw(ctx, forest, ds, kind=kind, **kw)


def raw_dataset():
    return nat.predict_raw_dataset(ctx, forest, ds, nat.RAW_LEAF)


def oob_mode():
    return nat.predict_oob(ctx, forest, ds, agg=nat.AGG_MODE, **kw)


def composed_hard():
    counts = nat.sample(ctx, True, 1.0, SEED, 0, L, N, part)
    votes = torch.empty((L, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    nat.predict_dataset_device(ctx, forest, ds, nat.OUT_VOTES, 1, votes.data_ptr())
    v = votes.cpu().numpy()
    cnt = np.zeros((NC, N), np.uint16)
    n_oob = np.zeros(N, np.int32)
    for i in range(L):
        oob = counts[i] == 0
        n_oob += oob
        for c in range(NC):
            cnt[c] += (v[i] == c) & oob
    return np.ascontiguousarray(cnt.T.astype(np.float64)), n_oob


def download():
    buf = torch.empty(N * NC, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    buf.cpu()
    return (time.perf_counter() - t0) * 1e3


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


hard = oob_raw(nat.RAW_VOTES)
soft = oob_raw(nat.RAW_LEAF)
plain = raw_dataset()
mode = oob_mode()
download()
if PROFILE:
    oob_raw(nat.RAW_VOTES)
    oob_raw(nat.RAW_LEAF)
    raw_dataset()
    oob_mode()
    print(json.dumps({"rows": N, "trees": L, "classes": NC, "profile_run": True}))
else:
    t0, base = timed(composed_hard)
    equal = bool(np.array_equal(hard[0], base[0]) and np.array_equal(hard[1], base[1]))
    t = {k: [] for k in ("oob_raw_hard", "oob_raw_soft", "raw_dataset_soft", "oob_mode", "download")}
    t_c = []
    for r in range(REPS):
        if r < COMPOSED_REPS:
            t_c.append(timed(composed_hard)[0])
        t["oob_raw_hard"].append(timed(lambda: oob_raw(nat.RAW_VOTES))[0])
        t["oob_raw_soft"].append(timed(lambda: oob_raw(nat.RAW_LEAF))[0])
        t["raw_dataset_soft"].append(timed(raw_dataset)[0])
        t["oob_mode"].append(timed(oob_mode)[0])
        t["download"].append(download())
    covered = hard[1] > 0
    res = {"rows": N, "trees": L, "classes": NC, "depth": DEPTH, "partitions": P, "reps": REPS,
           "composed_reps": COMPOSED_REPS, "result_bytes": 8 * N * NC}
    res.update({k: spread(v) for k, v in t.items()})
    res["composed_hard"] = spread(t_c)
    res["hard_equals_composed"] = equal
    res["n_oob_equals_mode"] = bool(np.array_equal(hard[1], mode[1]) and np.array_equal(soft[1], mode[1]))
    res["coverage"] = float(covered.mean())
    res["hard_soft_argmax_differ"] = float((hard[0].argmax(axis=1) != soft[0].argmax(axis=1))[covered].mean())
    res["soft_row_sum_minus_n_oob_max"] = float(np.abs(soft[0].sum(axis=1) - hard[1]).max())
    res["plain_row_sum_minus_trees_max"] = float(np.abs(plain.sum(axis=1) - L).max())
    print(json.dumps(res))
forest.free()
ds.free()
ctx.close()
