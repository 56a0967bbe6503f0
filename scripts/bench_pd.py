#!/usr/bin/env python3
"""Partial dependence of a bagged regression forest on one feature: the fused calls
(sbag_partial_dependence_dataset / sbag_partial_dependence, k_pd_count) against the composed path
the parent commit offers, in one run:

  fused dataset   nat.partial_dependence_dataset over the resident rows: the counts, the fold,
                  G doubles on the host
  fused host      nat.partial_dependence over HOST_ROWS host rows (default: all): upload in row
                  batches, k_quantize, the same kernel, the counts accumulating across batches
  fallback        the dataset call under SBAG_PD_FORCE_FALLBACK=1 (k_pd_walk + k_pd_prefix)
  composed        for every grid value: overwrite the column of the host rows, nat.predict, the
                  mean on the host.  COMPOSED_ROWS rows (default 1 000 000): the pass is linear
                  in the rows, and the figure is reported at its own row count, not scaled.

Shape: the C3 regression forest, sbag_dataset_synthetic ROWS x 100 (default 10M), TREES (128)
depth-DEPTH (8) trees fitted on PARTS (128) equal partitions, feature FEATURE (the one the
forest tests most often), GRID (32) points over the feature's values (0 .. 31, at half steps
past 32 points).  One warm-up of every path, then REPS timed repeats, host clock around calls
that end with their results on the host.  The fused results are compared in the run: fallback
and host rows bit for bit with the dataset call, the composed means within the rounding bound of
tests/test_gpu_pd.py.  Prints one JSON line.  Kernel (device) times are not taken here: run the
script under `rocprofv3 --kernel-trace --stats` with PROFILE=1 (the fused and fallback dataset
calls only, after the warm-up)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
NCMP = min(N, int(os.environ.get("COMPOSED_ROWS", 1_000_000)))
NHOST = min(N, int(os.environ.get("HOST_ROWS", N)))
F = 100
L = int(os.environ.get("TREES", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
G = int(os.environ.get("GRID", 32))
REPS = max(3, int(os.environ.get("REPS", 5)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
KNOB = "SBAG_PD_FORCE_FALLBACK"
PARTS = int(os.environ.get("PARTS", 128))
OFFSETS = [N * i // PARTS for i in range(PARTS + 1)]
SAMPLER = dict(replacement=True, sample_ratio=1.0, seed=1234, learner_begin=0, learner_end=L,
               partition_offsets=OFFSETS)


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
trees = [forest.tree(t)[0] for t in range(L)]
tests = np.zeros(F, np.int64)
for t, nodes in enumerate(trees):
    inner = nodes["left"] >= 0
    np.add.at(tests, forest.subspace(t)[nodes["feature"][inner]], 1)
J = int(os.environ.get("FEATURE", int(tests.argmax())))
GRID = np.arange(G) * (1.0 if G <= 32 else 32.0 / G)
leaves = [n["prediction"][n["left"] < 0] for n in trees]
res = {"rows": N, "features": F, "trees": L, "partitions": PARTS, "depth": DEPTH, "grid": G, "feature": J,
       "nodes_testing_feature": int(tests[J]), "leaves": int(sum(len(v) for v in leaves)), "fit_s": round(t_fit / 1e3, 1)}
fused = lambda: nat.partial_dependence_dataset(ctx, forest, ds, J, GRID)  # noqa: E731
os.environ.pop(KNOB, None)
if PROFILE:
    for force in (None, "1"):
        os.environ.pop(KNOB, None) if force is None else os.environ.__setitem__(KNOB, force)
        fused()
        fused()
    res["profile_run"] = True
else:
    out = fused()
    res["pd"] = [float(v) for v in out]
    res["fused_dataset"] = repeat(fused)
    os.environ[KNOB] = "1"
    res["fallback_equals_fused"] = bool(fused().tobytes() == out.tobytes())
    res["fallback_dataset"] = repeat(fused)
    os.environ.pop(KNOB, None)
    t_feat, X = timed(lambda: ds.features(0, NHOST))
    host = lambda: nat.partial_dependence(ctx, forest, X, J, GRID)  # noqa: E731
    res["fused_host"] = dict(repeat(host), rows=NHOST, features_ms=round(t_feat, 1))
    if NHOST == N:
        res["host_equals_dataset"] = bool(host().tobytes() == out.tobytes())
    # the composed path, at NCMP rows: G transforms and G host means
    Xc = np.ascontiguousarray(X[:NCMP]) if NHOST >= NCMP else ds.features(0, NCMP)
    del X
    part = nat.partial_dependence(ctx, forest, Xc, J, GRID)

    def composed():
        o = np.zeros(G)
        for g, v in enumerate(GRID):
            Xc[:, J] = v
            o[g] = nat.predict(ctx, forest, Xc, nat.AGG_MEAN).mean()
        return o

    t_c = []
    for r in range(3):  # the first is the warm-up
        t, base = timed(composed)
        if r:
            t_c.append(t)
        print(f"# composed pass {r}: {t:.0f} ms for {G} grid values over {NCMP} rows", file=sys.stderr, flush=True)
    res["composed"] = dict(spread(t_c), rows=NCMP, transforms=G, bytes_down=8 * NCMP * G)
    # np.mean sums pairwise: allow its own rounding (log2(N) + 1 half ulps) on top of the rule's
    bound = (max(len(v) for v in leaves) + L + 3 + np.log2(NCMP) + 1) * 2.0 ** -53 * max(np.abs(v).max() for v in leaves)
    res["fused_minus_composed_max"] = float(np.abs(part - base).max())
    res["fused_within_bound_of_composed"] = bool(np.abs(part - base).max() <= bound)
    res["result_bytes"] = 8 * G
print(json.dumps(res), flush=True)
forest.free()
ds.free()
ctx.close()
