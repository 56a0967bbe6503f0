#!/usr/bin/env python3
"""Per-row quantiles across a bagged regression forest: the fused calls
(sbag_predict_quantiles_dataset / sbag_predict_oob_quantiles, k_quant_tiled) against the
composed path the parent commit offers, in one run:

  fused dataset   nat.predict_quantiles_dataset over the resident rows: one kernel, the
                  N x Q fp64 result on the host
  fused oob       nat.predict_oob_quantiles: the sampler's counts of all the trees, then the
                  same kernel's out-of-bag instance
  fallback        the same two calls under SBAG_QUANT_FORCE_FALLBACK=1 (k_quant_walk +
                  k_quant_select)
  composed        model.transform(per_tree=True) semantics: dataset.features() (timed apart,
                  features_ms), nat.predict(per_tree=True) (the [trees x N] fp64 matrix to the
                  host) and np.quantile(method="linear") over it; out of bag: nat.sample's
                  counts and a masked loop over the rows.  COMPOSED_ROWS rows (default
                  1 000 000; the out-of-bag loop OOB_ROWS, default 20 000): the [trees x N]
                  matrix is 8 * trees * N bytes, and both composed passes are linear in N.

Shape: the C3 regression forest, sbag_dataset_synthetic ROWS x 100 (default 10M), TREES
(128) depth-DEPTH (8) trees fitted on PARTS (128) equal partitions, probabilities
[0.05, 0.5, 0.95].  One warm-up of every path, then
REPS timed repeats, host clock around calls that end with their results on the host.  The
fused results are compared with the composed ones in the run: exactly where the rule yields an
order statistic, to within 4 ulp of the row's largest magnitude elsewhere (np.quantile
interpolates by another formula), and exactly with tests/quantiles_ref.py's rule.  Prints one
JSON line.  Kernel (device) times are not taken here: run the script under
`rocprofv3 --kernel-trace --stats` with PROFILE=1 (the fused and fallback calls only, after
the warm-up)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import quantiles_ref as qr  # noqa: E402
import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native
N = int(os.environ.get("ROWS", 10_000_000))
NCMP = min(N, int(os.environ.get("COMPOSED_ROWS", 1_000_000)))
NOOB = min(NCMP, int(os.environ.get("OOB_ROWS", 20_000)))
F = 100
L = int(os.environ.get("TREES", 128))
DEPTH = int(os.environ.get("DEPTH", 8))
REPS = max(3, int(os.environ.get("REPS", 5)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
PROBS = [0.05, 0.5, 0.95]
KNOB = "SBAG_QUANT_FORCE_FALLBACK"
PARTS = int(os.environ.get("PARTS", 128))  # the sampler draws a (learner, partition) stream in sequence
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


def close(got, want, scale):
    """Equal, or within 4 ulp of the row's largest magnitude (NaN == NaN)."""
    with np.errstate(invalid="ignore"):
        return bool(((got == want) | (np.isnan(got) & np.isnan(want)) |
                     (np.abs(got - want) <= 4 * np.spacing(scale)[:, None])).all())


ctx = nat.Context(0)
ds = nat.DeviceDataset.synthetic(N, F, seed=20261015, num_classes=0, ctx=ctx)
t_fit, forest = timed(lambda: nat.fit(ctx, ds, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE, **SAMPLER))
fused = lambda: nat.predict_quantiles_dataset(ctx, forest, ds, PROBS)  # noqa: E731
fused_oob = lambda: nat.predict_oob_quantiles(ctx, forest, ds, PROBS, **SAMPLER)  # noqa: E731
res = {"rows": N, "features": F, "trees": L, "partitions": PARTS, "depth": DEPTH, "probs": PROBS, "fit_s": round(t_fit / 1e3, 1),
       "distinct_leaf_values": int(len(np.unique(np.concatenate(
           [(lambda n: n["prediction"][n["left"] < 0])(forest.tree(t)[0]) for t in range(L)]) + 0.0)))}
os.environ.pop(KNOB, None)
if PROFILE:
    for force in (None, "1"):
        os.environ.pop(KNOB, None) if force is None else os.environ.__setitem__(KNOB, force)
        fused()
        fused_oob()
    res["profile_run"] = True
else:
    out = fused()
    out_oob, n_oob = fused_oob()
    res["fused_dataset"] = repeat(fused)
    res["fused_oob"] = repeat(fused_oob)
    os.environ[KNOB] = "1"
    res["fallback_equals_fused"] = bool(np.array_equal(fused(), out, equal_nan=True) and
                                        np.array_equal(fused_oob()[0], out_oob, equal_nan=True))
    res["fallback_dataset"] = repeat(fused)
    res["fallback_oob"] = repeat(fused_oob)
    os.environ.pop(KNOB, None)
    # the composed path, at NCMP rows
    t_feat, X = timed(lambda: ds.features(0, NCMP))
    t_pt, t_q = [], []
    for r in range(3):  # the first is the warm-up
        tp, (_, pt) = timed(lambda: nat.predict(ctx, forest, X, nat.AGG_MEAN, per_tree=True))
        tq, base = timed(lambda: np.quantile(pt, PROBS, axis=0, method="linear").T)
        if r:
            t_pt.append(tp)
            t_q.append(tq)
        print(f"# composed pass {r}: per-tree {tp:.0f} ms, np.quantile {tq:.0f} ms", file=sys.stderr, flush=True)
    ref = qr.quantiles(pt, PROBS)[0]
    res["composed"] = {"rows": NCMP, "per_tree_bytes": 8 * L * NCMP, "features_ms": round(t_feat, 1),
                       "per_tree": spread(t_pt), "np_quantile": spread(t_q)}
    res["fused_equals_rule"] = bool(np.array_equal(out[:NCMP], ref))
    res["fused_within_4ulp_of_np_quantile"] = close(out[:NCMP], base, np.abs(pt).max(axis=0))
    res["median_equals_np_quantile"] = bool(np.array_equal(out[:NCMP, 1], base[:, 1])) if L % 2 else None
    # out of bag: nat.sample and a masked loop, at NOOB rows (the counts are drawn for all N)
    t_s, counts = timed(lambda: nat.sample(ctx, True, 1.0, 1234, 0, L, N, OFFSETS))

    def masked_loop():
        o = np.full((NOOB, len(PROBS)), np.nan)
        for r in range(NOOB):
            v = pt[counts[:, r] == 0, r]
            if len(v):
                o[r] = np.quantile(v, PROBS, method="linear")
        return o

    t_loop, base_oob = timed(masked_loop)
    ref_oob, ref_n = qr.quantiles(pt[:, :NOOB], PROBS, counts[:, :NOOB])
    res["composed_oob"] = {"rows": NOOB, "sample_ms_all_rows": round(t_s, 1), "masked_loop_ms": round(t_loop, 1)}
    res["oob_equals_rule"] = bool(np.array_equal(out_oob[:NOOB], ref_oob, equal_nan=True) and
                                  np.array_equal(n_oob[:NOOB], ref_n))
    res["oob_within_4ulp_of_np_quantile"] = close(out_oob[:NOOB], base_oob, np.abs(pt[:, :NOOB]).max(axis=0))
    res["result_bytes"] = 8 * N * len(PROBS)
print(json.dumps(res), flush=True)
forest.free()
ds.free()
ctx.close()
