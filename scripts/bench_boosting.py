"""Time the boosted bag (sbag_sample_boosted) at C3's row count: 10M rows, P = 128.

Two sets of means, both summing to the row count as proba * numLines does:
  uniform   every mean 1.0 (the first boosting iteration)
  skewed    weights after boosting has concentrated them: 85 % of the rows near 0.19, 10 %
            near 3.1, 3 % at 7.5, 1.5 % at 11 and 0.5 % at 28, interleaved
For each: the whole call (means up, counts down) and the two kernels (device events), and
the share of rows that left the register path.  Next to them sbag_sample for one learner on
the same rows (one stream per partition, about two generator steps per row) and the CPU
oracle's per-row loop on a subsample, scaled to the row count.

usage: python3 scripts/bench_boosting.py [--rows N] [--partitions P] [--reps K] [--lib SO]
  --lib   time another build of the library (e.g. sbag_boostbag.hip compiled with
          -DSBAG_BB_STEPS=32, the register path's step count)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

import oracle  # noqa: E402
import sbag_loader  # noqa: E402

sb = sbag_loader.load()
nat = sb._native

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--partitions", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu-rows", type=int, default=20_000)
ap.add_argument("--lib", default=None)
a = ap.parse_args()
if a.lib:
    nat.LIB_PATH = os.path.abspath(a.lib)
N = a.rows
off = np.linspace(0, N, a.partitions + 1).astype(np.int64)
rng = np.random.default_rng(20261020)
skew = rng.choice([0.2, 3.3, 8.0, 12.0, 30.0], size=N, p=[0.85, 0.10, 0.03, 0.015, 0.005])
skew = skew * (N / float(skew.sum()))
sets = {"uniform": np.ones(N), "skewed": skew}
seed = 779462656
ctx = nat.Context(0)
print(f"rows {N}, partitions {a.partitions}, library {nat.LIB_PATH}", flush=True)
for name, mean in sets.items():
    nat.sample_boosted(ctx, mean, seed, off)  # warm-up: workspace allocation
    for k in range(a.reps):
        t0 = time.perf_counter()
        got = nat.sample_boosted(ctx, mean, seed, off)
        dt = time.perf_counter() - t0
        s = nat.sample_boosted_stats(ctx)
        print(f"{name} rep {k}: call {dt * 1e3:.1f} ms, kernels {s['fast_ms'] + s['general_ms']:.2f} ms "
              f"(register path {s['fast_ms']:.2f}, LDS ring {s['general_ms']:.2f}), general-path rows "
              f"{s['rows_general']} = {100.0 * s['rows_general'] / N:.2f} %, zero rows {s['rows_zero']}, "
              f"max mean {mean.max():.2f}, max count {int(got.max())}, mean count {got.mean():.4f}, "
              f"register path covers {s['fast_doubles']} doubles", flush=True)
nat.sample(ctx, True, 1.0, seed, 0, 1, N, off)
for k in range(a.reps):
    t0 = time.perf_counter()
    got = nat.sample(ctx, True, 1.0, seed, 0, 1, N, off)
    dt = time.perf_counter() - t0
    print(f"sbag_sample, 1 learner, rep {k}: call {dt * 1e3:.1f} ms, mean count {got[0].mean():.4f}", flush=True)
ctx.close()
for name, mean in sets.items() if a.cpu_rows > 0 else ():
    sub = mean[: a.cpu_rows]
    t0 = time.perf_counter()
    for j in range(len(sub)):
        oracle.poisson(float(sub[j]), seed + j, 1)
    dt = time.perf_counter() - t0
    print(f"CPU oracle loop, {name}: {dt * 1e3:.1f} ms for {len(sub)} rows (one thread, one library call "
          f"per row) -> {dt * N / len(sub):.1f} s scaled to {N} rows", flush=True)
