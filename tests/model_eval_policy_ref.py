"""NumPy restatements of what `mobody_ens_evaluate_policy` / `mobody_eval_summary` add (include/mobody_hip.h): the member
rule of member mode and the summary's summation order in float32, with its fp64 counterpart and the derived bound.  Shared by
the CPU tests (random tables) and the GPU tests (the kernel's words)."""
import math

import numpy as np

THREADS = 256


def members(B, elites):
    """member[b] = elites[b % n_elites] (k_eval_members)."""
    e = np.asarray(elites, np.int32)
    return e[np.arange(B) % len(e)]


def group_count(B, G, g):
    """Rows b < B with b % G == g (the kernel's closed form)."""
    return (B - g - 1) // G + 1 if B > g else 0


def _tree(parts):
    """The fixed tree over 256 partial results: r[t] += r[t + h] for h = 128, 64, ..., 1, in the array's dtype."""
    r = np.array(parts)
    h = THREADS // 2
    while h >= 1:
        r[:h] = r[:h] + r[h:2 * h]
        h //= 2
    return r[0]


def _strided_sum(x, mask, dtype):
    """Thread t adds the rows t, t + 256, ... it owns AND `mask` selects, in ascending order, from zero; then the tree."""
    parts = np.zeros(THREADS, dtype)
    for b in np.nonzero(mask)[0]:                       # ascending b: each thread sees its rows in ascending order
        parts[b % THREADS] = dtype(parts[b % THREADS] + dtype(x[b]))
    return _tree(parts)


def summary32(ret, pen_sum, length, alive, G):
    """(out float32 [G + 1][4], nan_flag) by the kernel's rule: per group b % G and over all rows, fp32 sums of ret / pen_sum in
    the strided order and one fp32 division by the count; integer sums exact, divided in fp64 and rounded once."""
    ret, pen_sum = np.asarray(ret, np.float32), np.asarray(pen_sum, np.float32)
    length, alive = np.asarray(length, np.int64), (np.asarray(alive) != 0).astype(np.int64)
    B = ret.shape[0]
    out = np.full((G + 1, 4), np.nan, np.float32)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        for row in range(G + 1):
            mask = np.ones(B, bool) if row == G else rows % G == row
            n = B if row == G else group_count(B, G, row)
            assert n == int(mask.sum())
            if n == 0:
                continue
            out[row, 0] = _strided_sum(ret, mask, np.float32) / np.float32(n)
            out[row, 1] = np.float32(float(length[mask].sum()) / float(n))
            out[row, 2] = _strided_sum(pen_sum, mask, np.float32) / np.float32(n)
            out[row, 3] = np.float32(float(alive[mask].sum()) / float(n))
    return out, int(np.isnan(ret).any() or np.isnan(pen_sum).any())


def summary64(ret, pen_sum, length, alive, G):
    """(out fp64 [G + 1][4], magnitudes [G + 1][2] = sum |ret|, sum |pen_sum| per group, counts [G + 1])."""
    ret, pen_sum = np.asarray(ret, np.float64), np.asarray(pen_sum, np.float64)
    length, alive = np.asarray(length, np.int64), (np.asarray(alive) != 0).astype(np.int64)
    B = ret.shape[0]
    out, mag, cnt = np.full((G + 1, 4), np.nan), np.zeros((G + 1, 2)), np.zeros(G + 1, np.int64)
    rows = np.arange(B)
    for row in range(G + 1):
        mask = np.ones(B, bool) if row == G else rows % G == row
        n = cnt[row] = int(mask.sum())
        if n == 0:
            continue
        out[row] = (math.fsum(ret[mask]) / n, int(length[mask].sum()) / n, math.fsum(pen_sum[mask]) / n, int(alive[mask].sum()) / n)
        mag[row] = (np.abs(ret[mask]).sum(), np.abs(pen_sum[mask]).sum())
    return out, mag, cnt


def mean_bound(B, mag, count):
    """|fp32 mean - exact mean| <= (ceil(B / 256) + 9) 2^-24 sum|x| / count: at most ceil(B / 256) sequential adds per thread,
    eight tree levels and one division, each rounding at most 2^-24 relative of a partial result no larger than sum|x|."""
    return (math.ceil(B / THREADS) + 9) * 2.0 ** -24 * mag / count
