"""bench.py's command line on one MI355X: a plain run prints the headline alone, --full adds
the other figures, --dump-outputs writes the forest of the last timed step -- the arrays a
caller of nat.fit reads back -- and the same arguments give the same inputs in every run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

ROWS, FEATURES, LEARNERS, DEPTH, P = 200_003, 37, 5, 4, 128
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "breakdown_ms", "sampler_at_nproc_partitions", "nondyadic_labels",
             "continuous_features", "build", "cpu_baseline")
NODE_FIELDS = ("id", "left", "right", "feature", "split_bin", "threshold", "prediction",
               "impurity", "gain")


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(ROWS),
           "--features", str(FEATURES), "--learners", str(LEARNERS), "--depth", str(DEPTH),
           *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_forest(tmp_path):
    d = str(tmp_path / "dump")
    out = run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", d)
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(LEARNERS * ROWS / (out["ms_per_step"] / 1e3), rel=1e-3)
    assert not any(k in out for k in FULL_ONLY), sorted(out)

    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["nodes", "stats", "stats_rows", "subspace", "tree_offsets"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 1000 * 1000

    # the same fit in this process: same generator seed, bag seed, partitions and parameters
    ctx = nat.Context(0)
    ds = nat.DeviceDataset.synthetic(ROWS, FEATURES, seed=20261015, num_classes=0, ctx=ctx)
    part = [int(round(i * ROWS / P)) for i in range(P + 1)]
    forest = nat.fit(ctx, ds, replacement=True, sample_ratio=1.0, seed=-1395689524, learner_begin=0,
                     learner_end=LEARNERS, partition_offsets=part, max_depth=DEPTH, max_bins=32,
                     impurity=nat.IMPURITY_VARIANCE)
    off = got["tree_offsets"].astype(np.int64)
    assert len(off) == LEARNERS + 1 and off[-1] == len(got["nodes"]) == len(got["stats"])
    np.testing.assert_array_equal(got["stats_rows"], np.arange(off[-1]))
    for t in range(LEARNERS):
        nodes, stats = forest.tree(t)
        rows = got["nodes"][off[t]:off[t + 1]]
        assert len(rows) == len(nodes) > 1, t
        assert (rows[:, 0] == t).all()
        for k, name in enumerate(NODE_FIELDS):
            np.testing.assert_array_equal(rows[:, 1 + k], nodes[name].astype(np.float64), err_msg=f"{t} {name}")
        np.testing.assert_array_equal(got["stats"][off[t]:off[t + 1]], stats)
        mask = np.zeros(FEATURES, np.float32)
        mask[forest.subspace(t)] = 1.0
        np.testing.assert_array_equal(got["subspace"][t], mask)
    forest.free()
    ds.free()
    ctx.close()


def test_full_run_adds_the_other_figures():
    out = run_bench("--steps", "1", "--warmup", "1", "--full", "--cpu-rows", "20000",
                    "--cpu-learners", "2", "--nondyadic-steps", "1", "--continuous-steps", "1",
                    "--sampler-partitions", "64")
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["steps"] == 1 and out["ms_per_step"] > 0
    assert out["roofline"]["kernel"] and out["breakdown_ms"]["total_ms"] > 0
    assert out["nondyadic_labels"]["ms_per_step"] > 0
    assert out["sampler_at_nproc_partitions"]["partitions"] == 64
    assert out["cpu_baseline"]["value"] > 0
    # (the continuous-feature line belongs to the default workload's own shape)
    assert out["continuous_features"]["rows"] == ROWS
