#!/usr/bin/env python3
"""Forest proximities of the C3 forest (128 depth-8 trees on 100 features), in one run:

  counts     nat.proximity_dataset of COUNT_ROWS x COUNT_ROWS (8 192) resident rows: the whole call,
             the uint16 pair matrix on the host
  moments    nat.proximity_moments_dataset of MOMENT_ROWS (1 000 000 and 10 000 000) resident query
             rows against COUNT_ROWS references in 5 groups: the whole call, sums on the host
  baseline   the composed path: nat.predict_leaves_dataset and NumPy's
             (A[:, None, :] == B[None, :, :]).sum(-1) in row blocks of 64, over BASELINE_ROWS (2 048)
             x BASELINE_ROWS rows.  Reported at its own size, not scaled; compared with the counts.

The forest is fitted on FIT_ROWS (1 000 000) synthetic rows; the query rows are synthetic rows of
their own.  One warm-up of every call, then REPS timed repeats, host clock around calls that end
with their results on the host.  Writes OUT/bench_c3.json (OUT defaults to profiles/proximity) and,
unless TRACE=0, starts itself once more under `rocprofv3 --kernel-trace --stats` (PROFILE=1: one
call of each mode after a warm-up, no counters) and keeps the kernel statistics as
OUT/kernel_stats_c3.csv, from which the kernels' own times and the pair rates are read.

pairs/s = query rows x reference rows / kernel time.  The VALU ceiling is CUS x 64 lanes x CLOCK_GHZ
(256, 2.4: the figures DESIGN.md uses throughout) over VALU_PER_PAIR_DWORD (5.5: counted in the
emitted code of k_prox_tiled's inner loop) x the signature's dwords."""
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
MROWS = sorted(int(v) for v in os.environ.get("MOMENT_ROWS", "1000000,10000000").split(","))
NBASE = int(os.environ.get("BASELINE_ROWS", 2048))
NFIT = int(os.environ.get("FIT_ROWS", 1_000_000))
F, L, DEPTH, GROUPS, PARTS = 100, int(os.environ.get("TREES", 128)), int(os.environ.get("DEPTH", 8)), 5, 128
REPS = max(3, int(os.environ.get("REPS", 5)))
PROFILE = os.environ.get("PROFILE", "0") == "1"
OUT = os.path.abspath(os.environ.get("OUT", os.path.join(ROOT, "profiles", "proximity")))
CUS, CLOCK_GHZ, VALU_PER_PAIR_DWORD = 256, 2.4, 5.5


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def measure(call):
    out = call()  # warm-up
    if PROFILE:
        call()
        return None, out
    return spread([timed(call)[0] for _ in range(REPS)]), out


ctx = nat.Context(0)
fit_ds = nat.DeviceDataset.synthetic(NFIT, F, seed=20261015, num_classes=0, ctx=ctx)
forest = nat.fit(ctx, fit_ds, max_depth=DEPTH, max_bins=32, impurity=nat.IMPURITY_VARIANCE, replacement=True,
                 sample_ratio=1.0, seed=1234, learner_begin=0, learner_end=L,
                 partition_offsets=[NFIT * i // PARTS for i in range(PARTS + 1)])
leaves = [int((forest.tree(t)[0]["left"] < 0).sum()) for t in range(L)]
sig_dwords = ((L * (1 if max(leaves) <= 256 else 2) + 15) // 16 * 16) // 4
ref = nat.DeviceDataset.from_numpy(fit_ds.features(0, NC), np.zeros(NC), ctx)
fit_ds.free()
groups = (np.arange(NC) * 7 % GROUPS).astype(np.int32)
res = {"features": F, "trees": L, "depth": DEPTH, "max_leaves": max(leaves), "signature_dwords": sig_dwords,
       "valu_per_pair_dword": VALU_PER_PAIR_DWORD, "cus": CUS, "clock_ghz": CLOCK_GHZ,
       "valu_ceiling_pairs_per_s": CUS * 64 * CLOCK_GHZ * 1e9 / (VALU_PER_PAIR_DWORD * sig_dwords)}

t, cnt = measure(lambda: nat.proximity_dataset(ctx, forest, ref, ref))
res["counts"] = {"nq": NC, "nr": NC, "call": t, "result_bytes": 2 * NC * NC,
                 "diagonal_is_trees": bool((np.diag(cnt) == L).all())}
res["moments"] = []
for n in MROWS:
    q = nat.DeviceDataset.synthetic(n, F, seed=7, num_classes=0, ctx=ctx)
    t, mom = measure(lambda: nat.proximity_moments_dataset(ctx, forest, q, ref, groups, GROUPS))
    res["moments"].append({"nq": n, "nr": NC, "groups": GROUPS, "call": t, "result_bytes": 16 * n * GROUPS})
    q.free()
    print(f"# moments {n}: {res['moments'][-1]}", file=sys.stderr, flush=True)
if not PROFILE and NBASE > 0:
    part = nat.DeviceDataset.from_numpy(ref.features(0, NBASE), np.zeros(NBASE), ctx)

    def composed():
        A = nat.predict_leaves_dataset(ctx, forest, part)
        return np.concatenate([(A[i:i + 64, None, :] == A[None, :, :]).sum(-1) for i in range(0, NBASE, 64)])

    t_b, base = timed(composed)
    res["baseline_composed"] = {"nq": NBASE, "nr": NBASE, "ms": round(t_b, 1), "pairs_per_s": NBASE * NBASE / (t_b * 1e-3),
                                "equals_counts": bool(np.array_equal(base, cnt[:NBASE, :NBASE]))}
    part.free()
ref.free()
forest.free()
ctx.close()
if PROFILE:
    sys.exit(0)
os.makedirs(OUT, exist_ok=True)
if os.environ.get("TRACE", "1") == "1":  # a fresh process under the profiler: kernel times only
    tmp = os.path.join(OUT, "trace_tmp")
    subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "prox", "--output-format", "csv",
                           "--", sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PROFILE="1"))
    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]
    shutil.copy(stats, os.path.join(OUT, "kernel_stats_c3.csv"))
    shutil.rmtree(tmp)
    with open(os.path.join(OUT, "kernel_stats_c3.csv")) as fh:
        rows = {r["Name"]: r for r in csv.DictReader(fh)}
    # the profiled run makes two calls of each mode: the pairs of both, over the kernels' total time
    for name, pairs in (("false", 2 * NC * NC), ("true", 2 * NC * sum(MROWS))):
        k = [r for nm, r in rows.items() if "k_prox_tiled" in nm and f", {name}>" in nm]
        if k:
            ns = sum(float(r["TotalDurationNs"]) for r in k)
            rate = pairs / (ns * 1e-9)
            res["kernel_counts" if name == "false" else "kernel_moments"] = {
                "kernel_ms_total": round(ns * 1e-6, 3), "calls": sum(int(r["Calls"]) for r in k),
                "pairs_per_s": rate, "share_of_valu_ceiling": round(rate / res["valu_ceiling_pairs_per_s"], 3)}
with open(os.path.join(OUT, "bench_c3.json"), "w") as fh:
    fh.write(json.dumps(res) + "\n")
print(json.dumps(res), flush=True)
