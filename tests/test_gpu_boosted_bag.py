"""GPU: sbag_sample_boosted against the oracle, byte for byte.

BoostingParams.extractBoostedBag (ml/boosting/BoostingParams.scala:127-148) gives every row
with a non-zero mean a PoissonDistribution of its own, reseeded with seed + i + j.  The
library draws the bag in two kernels: rows that finish within `fast_doubles` nextDouble()
calls on a register path, the others on a second pass with the generator state in LDS.  The
inputs below put rows on both sides of that boundary (exactly fast_doubles doubles under
every seed, exactly fast_doubles + 1 under four of the five), of the zero-mean shortcut, and of generator step 70 (35 doubles),
from where a step reads words the generator itself rewrote; the per-path row counts the
library reports must be the ones the reference's counts imply.

The 255 cap of the bag column cannot be reached below a mean of 40 (P(Poisson(39.999999) >
255) is zero at any sample size a test can draw), so that error code has no case here.
"""
import ctypes
import functools

import numpy as np
import pytest

import boosting_ref as br

import spark_bagging_amd as sb
from spark_bagging_amd import _native as nat

pytestmark = pytest.mark.gpu

N = 4097
MEANS = np.array([0.0, 1e-300, 1e-12, 0.05, 1.0, 7.5, 39.9, 39.999999])
# uneven partitions: an empty one first, a one-row one, an empty one in the middle
PART = [0, 0, 1, 700, 700, 2500, 2563, N]
SEEDS = [-2**63, -1, 0, 2**32, 2**63 - 1]


@pytest.fixture(scope="module")
def ctx():
    return sb.default_context(0)


def means():
    """Runs of 128 rows per value over the first half, interleaved draws over the second."""
    rng = np.random.default_rng(20261020)
    m = np.empty(N)
    half = 2048
    m[:half] = MEANS[(np.arange(half) // 128) % len(MEANS)]
    m[half:] = MEANS[rng.integers(0, len(MEANS), N - half)]
    return m


@functools.lru_cache(maxsize=None)
def reference(seed):
    return br.boosted_bag(means(), PART, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_boosted_bag_matches_oracle(ctx, seed):
    m = means()
    want = reference(seed)
    got = nat.sample_boosted(ctx, m, seed, PART)
    stats = nat.sample_boosted_stats(ctx)
    assert got.dtype == np.uint8 and got.shape == (N,)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]], m[bad[:8]])
    assert int(want.max()) <= 255
    # the paths: every boundary has rows on both sides, and the library took them there
    d = br.doubles_drawn(m, want)
    D = stats["fast_doubles"]
    assert (d == D).any() and (d > D).any(), "no row at the register path's last double"
    assert (d >= 35).any() and ((d > D) & (d < 35)).any(), "no row on both sides of step 70"
    assert (m == 0.0).any() and (d == 1).any()
    assert stats["rows_zero"] == int((m == 0.0).sum())
    assert stats["rows_general"] == int((d > D).sum())
    assert stats["rows_fast"] == int(((d > 0) & (d <= D)).sum())
    assert stats["rows_fast"] > 0 and stats["rows_general"] > 0
    assert (got[m == 0.0] == 0).all()


def test_rows_one_double_past_the_register_path(ctx):
    """The first row the second pass must take: fast_doubles + 1 doubles."""
    nat.sample_boosted(ctx, means(), 0, PART)
    D = nat.sample_boosted_stats(ctx)["fast_doubles"]
    hits = [int((br.doubles_drawn(means(), reference(s)) == D + 1).sum()) for s in SEEDS]
    assert sum(h > 0 for h in hits) >= 4, hits


def test_seed_wraps_inside_a_partition():
    """seed + i + j passes 2^63 - 1 inside the partitions (the addition is Long's)."""
    assert br.wrap64(2**63 - 1 + 1 + 0) == -2**63
    a = reference(2**63 - 1)
    b = reference(-2**63)
    assert not np.array_equal(a, b)


def test_loop_bound_ends_tiny_means(ctx):
    """1000 * mean < 1: nextPoisson's loop runs once, whatever the product does."""
    m = np.full(512, 1e-12)
    m[::2] = 1e-300
    got = nat.sample_boosted(ctx, m, 12345, [0, 100, 512])
    assert np.array_equal(got, br.boosted_bag(m, [0, 100, 512], 12345))
    assert int(got.max()) <= 1


def test_empty_and_single_row(ctx):
    assert nat.sample_boosted(ctx, np.zeros(0), 7).shape == (0,)
    for mean in (0.0, 1.0, 39.9):
        got = nat.sample_boosted(ctx, np.array([mean]), -5)
        assert np.array_equal(got, br.boosted_bag([mean], [0, 1], -5))
    got = nat.sample_boosted(ctx, np.array([1.0]), -5, [0, 0, 1])  # the row is in partition 1
    assert np.array_equal(got, br.boosted_bag([1.0], [0, 0, 1], -5))


def _raw_call(ctx, m, seed, part, fill=0xAB):
    m = np.ascontiguousarray(m, np.float64)
    off = np.ascontiguousarray(part, np.int64)
    out = np.full(len(m), fill, np.uint8)
    rc = nat.lib().sbag_sample_boosted(ctx.handle, nat.ptr(m), seed, nat.ptr(off), len(off) - 1, len(m),
                                       nat.ptr(out))
    return rc, out


@pytest.mark.parametrize("bad,code", [(-1e-300, nat.SBAG_EINVAL), (float("nan"), nat.SBAG_EINVAL),
                                      (float("inf"), nat.SBAG_EINVAL), (-float("inf"), nat.SBAG_EINVAL),
                                      (40.0, nat.SBAG_EUNSUPPORTED), (1e300, nat.SBAG_EUNSUPPORTED)])
def test_bad_means_are_refused_and_the_context_stays_usable(ctx, bad, code):
    m = means()
    m[3001] = bad
    rc, out = _raw_call(ctx, m, 0, PART)
    assert rc == code
    assert len(nat.lib().sbag_last_error()) > 0
    assert (out == 0xAB).all(), "counts_out was written before the failure"
    # the next call on the same context gives a fresh context's bytes
    got = nat.sample_boosted(ctx, means(), 0, PART)
    fresh = nat.Context(0)
    try:
        assert np.array_equal(got, nat.sample_boosted(fresh, means(), 0, PART))
    finally:
        fresh.close()
    assert np.array_equal(got, reference(0))


def test_invalid_before_unsupported(ctx):
    m = means()
    m[10], m[4000] = 45.0, -1.0
    rc, _ = _raw_call(ctx, m, 0, PART)
    assert rc == nat.SBAG_EINVAL


def test_partitions_are_validated_as_in_sample(ctx):
    m = np.ones(100)
    for part in ([0, 50, 99], [1, 50, 100], [0, 60, 50, 100]):
        rc, out = _raw_call(ctx, m, 0, part)
        assert rc == nat.SBAG_EINVAL
        assert (out == 0xAB).all()
    assert nat.lib().sbag_sample_boosted(None, None, 0, None, 1, 5, None) == nat.SBAG_EINVAL
    assert nat.lib().sbag_sample_boosted(ctx.handle, None, 0, None, 1, 5, None) == nat.SBAG_EINVAL
    assert ctypes.c_int(nat.lib().sbag_sample_boosted_stats(ctx.handle, None)).value == nat.SBAG_EINVAL
