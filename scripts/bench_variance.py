#!/usr/bin/env python3
"""The infinitesimal-jackknife variance of a bagged regression forest: the fused calls
(sbag_bag_gram, sbag_predict_variance_dataset: k_gram_mfma, k_ij_tiled) against the composed
path the parent commit offers, in one run:

  bag_gram        nat.bag_gram: the sampler's counts of all the trees and their Gram matrix, the
                  T x T int64 result on the host; also under SBAG_GRAM_FORCE_FALLBACK=1 (k_gram_dot)
  variance        nat.predict_variance_dataset over the first SMALL_ROWS (1M) and over all ROWS
                  resident rows, the N x 3 fp64 result on the host; also under
                  SBAG_IJ_FORCE_FALLBACK=1 (the per-tree predict path + k_ij_form)
  quantiles       nat.predict_quantiles_dataset over the same rows, for k_quant_tiled beside
                  k_ij_tiled in the same run
  composed        nat.sample's counts (trees x ROWS bytes to the host), nat.predict(per_tree=True)
                  and NumPy: centred counts against d, squared and summed, COMPOSED_ROWS query
                  rows (default 200) against the full training set; reported at that size,
                  not scaled

Shape: the C3 regression forest, sbag_dataset_synthetic ROWS x 100 (default 10M), TREES (128)
depth-DEPTH (8) trees fitted on PARTS (128) equal partitions.  One warm-up of every path, then
REPS timed repeats, host clock around calls that end with their results on the host.  The fused
result is compared in the run with tests/ij_ref.py (bit for bit) and with the composed value
(relative error).  Prints one JSON line.  Kernel (device) times are not taken here: run the
script under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (the fused calls only, after the
warm-up)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ij_ref  # noqa: E402
import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
NSMALL = min(N, int(os.environ.get("SMALL_ROWS", 1_000_000)))
NCMP = min(N, int(os.environ.get("COMPOSED_ROWS", 200)))
F = 100
L = int(os.environ.get("TREES", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(3, int(os.environ.get("REPS", 5)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
PARTS = int(os.environ.get("PARTS", 128))
OFFSETS = [N * i // PARTS for i in range(PARTS + 1)]
SAMPLER = dict(replacement=True, sample_ratio=1.0, seed=1234, learner_begin=0, learner_end=L,
               partition_offsets=OFFSETS)
GRAM_KNOB, IJ_KNOB = "SBAG_GRAM_FORCE_FALLBACK", "SBAG_IJ_FORCE_FALLBACK"


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def repeat(fn):
    fn()  # warm-up
    return spread([timed(fn)[0] for _ in range(REPS)])


ctx = nat.Context(0)
ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=0, ctx=ctx)
t_fit, forest = timed(lambda: nat.fit(ctx, ds, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE, **SAMPLER))
X_small = ds.features(0, NSMALL)
small = nat.DeviceDataset.from_numpy(X_small, np.zeros(NSMALL), ctx)
del X_small
gram_call = lambda: nat.bag_gram(ctx, num_rows=N, **SAMPLER)  # noqa: E731
gram = gram_call()
var_all = lambda: nat.predict_variance_dataset(ctx, forest, ds, gram)  # noqa: E731
var_small = lambda: nat.predict_variance_dataset(ctx, forest, small, gram)  # noqa: E731
q_all = lambda: nat.predict_quantiles_dataset(ctx, forest, ds, [0.05, 0.5, 0.95])  # noqa: E731
q_small = lambda: nat.predict_quantiles_dataset(ctx, forest, small, [0.05, 0.5, 0.95])  # noqa: E731
res = {"rows": N, "small_rows": NSMALL, "features": F, "trees": L, "partitions": PARTS, "depth": DEPTH,
       "fit_s": round(t_fit / 1e3, 1)}
if PROFILE:
    for call in (gram_call, var_small, var_all, q_small, q_all):
        call()
    res["profile_run"] = True
else:
    out = var_all()
    res["bag_gram"] = repeat(gram_call)
    res["variance_small"] = repeat(var_small)
    res["variance_all"] = repeat(var_all)
    res["quantiles_small"] = repeat(q_small)
    res["quantiles_all"] = repeat(q_all)
    os.environ[GRAM_KNOB] = "1"
    res["gram_dot_equals_mfma"] = bool(np.array_equal(gram_call(), gram))
    res["bag_gram_dot"] = repeat(gram_call)
    os.environ.pop(GRAM_KNOB)
    os.environ[IJ_KNOB] = "1"
    res["fallback_equals_fused"] = bool(np.array_equal(var_small(), out[:NSMALL], equal_nan=True))
    res["variance_small_fallback"] = repeat(var_small)
    os.environ.pop(IJ_KNOB)
    # the composed path: every count to the host, per-tree predictions of NCMP rows, NumPy
    t_s, counts = timed(lambda: nat.sample(ctx, True, 1.0, 1234, 0, L, N, OFFSETS))
    res["gram_equals_counts"] = bool(all(int(gram[a, a]) == int((counts[a].astype(np.int64) ** 2).sum()) for a in range(L)))
    Xq = ds.features(0, NCMP)
    t_pt, (_, pt) = timed(lambda: nat.predict(ctx, forest, Xq, nat.AGG_MEAN, per_tree=True))

    def composed():
        d = pt - pt.mean(axis=0)
        v = np.zeros(NCMP)
        for i0 in range(0, N, 500_000):  # training rows in pieces: [NCMP x piece] fp64 at a time
            cc = counts[:, i0:i0 + 500_000].astype(np.float64)
            cc -= cc.mean(axis=0)
            v += ((d.T @ cc) ** 2).sum(axis=1)
        return v / (L * L)

    t_np, base = timed(composed)
    m, v_ij, v_iju, _ = ij_ref.variance(pt, gram)
    res["composed"] = {"query_rows": NCMP, "count_bytes": int(counts.nbytes), "sample_ms": round(t_s, 1),
                       "per_tree_ms": round(t_pt, 1), "numpy_ms": round(t_np, 1)}
    res["fused_equals_rule"] = bool(np.array_equal(out[:NCMP], np.column_stack([m, v_ij, v_iju])))
    res["max_rel_err_vs_composed"] = float(np.max(np.abs(out[:NCMP, 1] - base) / base))
    res["v_ij_median"] = float(np.median(out[:, 1]))
    res["v_iju_median"] = float(np.median(out[:, 2]))
    res["v_iju_negative_share"] = float((out[:, 2] < 0).mean())
print(json.dumps(res), flush=True)
forest.free()
small.free()
ds.free()
ctx.close()
