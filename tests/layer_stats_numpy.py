"""fp64 restatement of csrc/layer_stats.hip in numpy: the rules of include/mvfnet_hip.h written down a second time, serially, for the tests to compare against.

flat_segment_stats: d_i = float64(x_i) (- float64(y_i)); per segment the sum of d_i^2 and the largest |d_i| over the finite d_i, the counts of NaN and of
+-inf.  The sum is numpy's pairwise fp64 sum -- one more order of the same non-negative additions, inside the bound the header states.
bn_stats_nonfinite: per segment the number of values that are not finite."""
import numpy as np

FLAT_STATS_DTYPE = np.dtype([("sumsq", "<f8"), ("absmax", "<f8"), ("n_nan", "<i8"), ("n_inf", "<i8")])      # mvf_flat_stats_t
STAT_DTYPE = np.dtype([("ptr", "<u8"), ("first", "<i8")])                                                   # mvf_stat_segment_t
EPS = 2.0 ** -52


def flat_segment_stats(x, y, first):
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    first = [int(f) for f in first]
    assert first[0] == 0 and all(a < b for a, b in zip(first, first[1:])) and first[-1] < n
    with np.errstate(invalid="ignore", over="ignore"):
        d = x.astype(np.float64) if y is None else x.astype(np.float64) - np.asarray(y, dtype=np.float32).astype(np.float64)
    out = np.zeros(len(first), FLAT_STATS_DTYPE)
    for k, (b, e) in enumerate(zip(first, first[1:] + [n])):
        seg = d[b:e]
        fin = seg[np.isfinite(seg)]
        out[k] = (float(np.sum(fin * fin)), float(np.abs(fin).max()) if fin.size else 0.0, int(np.isnan(seg).sum()), int(np.isinf(seg).sum()))
    return out


def lengths(first, n):
    first = [int(f) for f in first]
    return np.diff(np.array(first + [int(n)], dtype=np.int64))


def sumsq_bound(n_s):
    """Relative bound on sumsq for a segment of n_s elements: squares of floats are exact in double, only the order of at most n_s non-negative additions
    differs ((n_s - 1) roundings each way), plus the roundings of the difference and of its square in the difference mode."""
    return (np.asarray(n_s, dtype=np.float64) + 4.0) * EPS


def assert_stats(got, ref, n_s, what=""):
    """Counts and absmax exactly equal, sumsq within sumsq_bound."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    for f in ("n_nan", "n_inf", "absmax"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.flatnonzero(got[f] != ref[f])[:8], got[f][:8], ref[f][:8])
    err = np.abs(got["sumsq"] - ref["sumsq"])
    bad = np.flatnonzero(~(err <= sumsq_bound(n_s) * ref["sumsq"]))
    assert bad.size == 0, (what, bad[:8], got["sumsq"][bad[:8]], ref["sumsq"][bad[:8]])


def bn_stats_nonfinite(values):
    """values: one float32 array per segment."""
    return np.array([int((~np.isfinite(np.asarray(v, dtype=np.float32))).sum()) for v in values], dtype=np.int64)
