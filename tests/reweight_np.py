"""A float64 NumPy restatement of what naima_amd.reweight's kernels compute (nh_row_sums_select,
nh_psis_weights, nh_weighted_moments, nh_weighted_select, nh_resample_systematic), written from
the definitions.  The generalised-Pareto fit and the tail rule are those of tests/infocrit_np.py
(psis_column), applied to x = lr - max.  No GPU, no naima_amd import."""
import math

import numpy as np

from infocrit_np import LOG_TINY, gpd_fit, logsumexp, tail_length  # noqa: F401


def row_sums(L, groups, sign):
    """[M][G]: column g = sign * the sum of the columns groups[g] of L, added in their order"""
    L = np.asarray(L, dtype=float)
    out = np.zeros((L.shape[0], len(groups)))
    for g, cols in enumerate(groups):
        for c in cols:
            out[:, g] = out[:, g] + sign * L[:, c]
    return out


def psis_weights_column(lr, Mt):
    """(lw [M], pareto_k, n_tail, ess, lmean, status) of one column of log-ratios"""
    lr = np.asarray(lr, dtype=float)
    M = len(lr)
    bad = int(np.sum(np.isnan(lr) | np.isposinf(lr)))
    if bad == 0 and not np.any(np.isfinite(lr)):
        bad = M
    if bad:
        return np.full(M, np.nan), np.nan, 0, np.nan, np.nan, bad
    with np.errstate(all="ignore"):
        x = lr - lr.max()
        cut = max(np.sort(x)[M - Mt - 1], LOG_TINY)
        tail = np.flatnonzero(x > cut)
        n = len(tail)
        k = np.inf
        if Mt > 0 and n > 4:
            order = tail[np.lexsort((tail, x[tail]))]  # ascending by (value, row index)
            t = np.exp(x[order]) - np.exp(cut)
            k, sigma = gpd_fit(t)
            if np.isfinite(k):
                lp = np.log1p(-(np.arange(n) + 0.5) / n)
                g = -lp if abs(k) < np.finfo(float).eps else np.expm1(-k * lp) / k
                v = np.log(g * sigma + np.exp(cut))
                x = x.copy()
                x[order] = np.where(v > 0.0, 0.0, v)
        lw = x - logsumexp(x)
        ess = 1.0 / np.sum(np.exp(2.0 * lw))
        lmean = logsumexp(lr) - math.log(M)
    return lw, float(k), n, float(ess), float(lmean), 0


def psis_weights_np(lr, Mt):
    """dict of lw [M][K], pareto_k, n_tail, ess, lmean, status [K] for log-ratios [M][K]"""
    lr = np.asarray(lr, dtype=float)
    if lr.ndim == 1:
        lr = lr[:, None]
    cols = [psis_weights_column(lr[:, c], Mt) for c in range(lr.shape[1])]
    return dict(lw=np.column_stack([c[0] for c in cols]), pareto_k=np.array([c[1] for c in cols]),
                n_tail=np.array([c[2] for c in cols], dtype=np.int64),
                ess=np.array([c[3] for c in cols]), lmean=np.array([c[4] for c in cols]),
                status=np.array([c[5] for c in cols], dtype=np.int32))


def weighted_moments_np(x, lw):
    """(n_used, mean, var) [ncol] of the columns of x [M][ncol] under log-weights lw [M]; rows
    with lw = -inf are left out whatever they hold"""
    x = np.asarray(x, dtype=float)
    live = ~np.isneginf(lw)
    w, v = np.exp(lw[live]), x[live]
    n = np.full(x.shape[1], int(live.sum()), dtype=np.int64)
    with np.errstate(all="ignore"):
        sw = w.sum()
        mean = (w[:, None] * v).sum(axis=0) / sw
        var = (w[:, None] * (v - mean) ** 2).sum(axis=0) / sw
    bad = ~np.all(np.isfinite(v), axis=0) | (live.sum() == 0)
    mean[bad] = np.nan
    var[bad] = np.nan
    return n, mean, var


def weighted_quantile_np(x, lw, q):
    """(out [nq], margin): the value of the first row, ascending by (value, row index) among the
    rows with lw > -inf, whose running weight c reaches q C (and is positive); margin = the
    smallest |c_i - q_j C| / C over all i, j, which tells how far the answer is from a tie that
    rounding could decide (two pairs cannot be one and are left out: q = 0, which c > 0 decides
    exactly, and the last running sum against q = 1, which is C itself however it is summed).  A
    NaN among those rows gives NaN."""
    x, q = np.asarray(x, dtype=float), np.atleast_1d(np.asarray(q, dtype=float))
    rows = np.flatnonzero(~np.isneginf(lw))
    v = x[rows]
    if len(rows) == 0 or np.any(np.isnan(v)):
        return np.full(len(q), np.nan), np.inf
    order = np.lexsort((rows, v + 0.0))  # (-0.0 + 0.0 = +0.0: the two tie)
    c = np.cumsum(np.exp(lw[rows[order]]))
    C = c[-1]
    if not C > 0:
        return np.full(len(q), np.nan), np.inf
    out = np.empty(len(q))
    for j, qq in enumerate(q):
        i = np.flatnonzero((c >= qq * C) & (c > 0))[0]
        out[j] = v[order][i]
    d = np.abs(c[:, None] - q[None, :] * C) / C
    d[:, q == 0.0] = np.inf   # (c > 0 decides q = 0, and no rounding moves that)
    d[-1, q == 1.0] = np.inf  # (the last running sum IS C, in any order of summation)
    return out, float(d.min())


def systematic_np(lw, u0, n_out):
    """(idx int64 [n_out], margin): the first row i, in row order, with c_i >= ((u0 + j) / n_out) C
    and w_i > 0; margin as in weighted_quantile_np"""
    w = np.where(np.isneginf(lw), 0.0, np.exp(lw))
    c = np.cumsum(w)
    C = c[-1]
    thr = ((u0 + np.arange(n_out)) / n_out) * C
    idx = np.empty(n_out, dtype=np.int64)
    for j in range(n_out):
        idx[j] = np.flatnonzero((c >= thr[j]) & (w > 0))[0]
    at = np.searchsorted(c, thr)  # (c ascends: the nearest running sums lie on either side)
    near = np.minimum(np.abs(c[np.minimum(at, len(c) - 1)] - thr), np.abs(c[np.maximum(at - 1, 0)] - thr))
    return idx, float(near.min() / C)
