"""A float64 NumPy restatement of what naima_amd.infocrit's kernels compute (nh_pointwise_lnl,
nh_lnl_column_stats, nh_psis_columns), written from the definitions: the per-point terms of
core.lnprobmodel, WAIC, and Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao &
Gabry) with the generalised-Pareto fit of Zhang & Stephens (2009) and the weak priors of the loo
package.  The tests hold the device to it; tests/test_infocrit_host.py holds IT to a closed form.
No GPU, no naima_amd import."""
import math
import warnings

import numpy as np

LOG_TINY = math.log(np.finfo(float).tiny)


def pointwise_lnl(x, conv, flux, elo, ehi, ul, cl):
    """L[s][k] for spectra x [M][nE] in the model's unit: -(d*d)/(2*sg*sg) with d = x*conv - flux,
    sg = ehi where d > 0 else elo, for a point that is not an upper limit; for an upper limit
    log(1 - cl[nviol_s]) where x*conv > flux else 0, nviol_s the row's number of violated limits
    (cl is indexed by the count: core.py:89-92; cl has nE or nE + 1 entries)"""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    ul = np.asarray(ul, dtype=bool)
    cl = np.broadcast_to(np.asarray(cl, dtype=float), (max(np.size(cl), len(flux)),))
    mc = x * conv
    d = mc - flux
    sg = np.where(d > 0, ehi, elo)
    with np.errstate(divide="ignore", invalid="ignore"):  # (an upper limit's errors may be zero)
        L = -(d * d) / (2.0 * (sg * sg))
    viol = (mc > flux) & ul
    nviol = viol.sum(axis=1)
    with np.errstate(divide="ignore"):
        pen = np.log(1.0 - cl[np.minimum(nviol, len(cl) - 1)])
    L = np.where(ul, np.where(viol, pen[:, None], 0.0), L)
    return L


def logsumexp(a, axis=None):
    a = np.asarray(a, dtype=float)
    m = np.max(a, axis=axis, keepdims=True)
    out = m + np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def column_stats(L):
    """max, mean, variance (ddof = 1: NaN for one row), lse and min of every column"""
    L = np.asarray(L, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = L.var(axis=0, ddof=1) if L.shape[0] > 1 else np.full(L.shape[1], np.nan)
    return dict(max=L.max(axis=0), mean=L.mean(axis=0), var=var, lse=logsumexp(L, axis=0),
                min=L.min(axis=0))


def _se(v):
    return float(np.sqrt(len(v) * np.var(v, ddof=1))) if len(v) > 1 else float("nan")


def waic(L):
    L = np.asarray(L, dtype=float)
    M, nE = L.shape
    st = column_stats(L)
    lppd_i = st["lse"] - math.log(M)
    p_i = st["var"]
    elpd_i = lppd_i - p_i
    return dict(elpd_waic=float(elpd_i.sum()), p_waic=float(p_i.sum()), lppd=float(lppd_i.sum()),
                se=_se(elpd_i), elpd_waic_i=elpd_i, p_waic_i=p_i, lppd_i=lppd_i, n_samples=M,
                n_data=nE)


def tail_length(M, reff=1.0):
    return min(M // 5, int(math.ceil(3.0 * math.sqrt(M / reff))))


def gpd_fit(t):
    """(k, sigma) of the generalised Pareto distribution fitted to the ascending t > 0"""
    n = len(t)
    m = 30 + int(math.floor(math.sqrt(n)))
    b = 1.0 - np.sqrt(m / (np.arange(1, m + 1, dtype=float) - 0.5))
    b /= 3.0 * t[int(n / 4 + 0.5) - 1]
    b += 1.0 / t[n - 1]
    kj = np.log1p(-b[:, None] * t).mean(axis=1)
    lj = n * (np.log(-b / kj) - kj - 1.0)
    w = 1.0 / np.exp(lj - lj[:, None]).sum(axis=1)
    keep = w >= 10.0 * np.finfo(float).eps
    b, w = b[keep], w[keep]
    w = w / w.sum()
    bp = np.sum(b * w)
    kp = np.log1p(-bp * t).mean()
    sigma = -kp / bp
    k = (n * kp + 5.0) / (n + 10.0)
    return k, sigma


def psis_column(Lk, Mt):
    """(pareto_k, n_tail, elpd_loo_k) of one column of L with tail length Mt"""
    Lk = np.asarray(Lk, dtype=float)
    M = len(Lk)
    x = -Lk
    x = x - x.max()
    cut = max(np.sort(x)[M - Mt - 1], LOG_TINY)
    tail = np.flatnonzero(x > cut)
    n = len(tail)
    k = np.inf
    if Mt > 0 and n > 4:
        order = tail[np.lexsort((tail, x[tail]))]  # ascending by (value, row index)
        t = np.exp(x[order]) - np.exp(cut)
        with np.errstate(all="ignore"):
            k, sigma = gpd_fit(t)
            if np.isfinite(k):
                lp = np.log1p(-(np.arange(n) + 0.5) / n)
                g = -lp if abs(k) < np.finfo(float).eps else np.expm1(-k * lp) / k
                v = np.log(g * sigma + np.exp(cut))
                x = x.copy()
                x[order] = np.where(v > 0.0, 0.0, v)
    lw = x - logsumexp(x)
    return float(k), n, float(logsumexp(lw + Lk))


def loo(L, reff=1.0):
    L = np.asarray(L, dtype=float)
    M, nE = L.shape
    Mt = tail_length(M, reff)
    cols = [psis_column(L[:, c], Mt) for c in range(nE)]
    k = np.array([c[0] for c in cols])
    n = np.array([c[1] for c in cols], dtype=np.int64)
    elpd_i = np.array([c[2] for c in cols])
    lppd_i = logsumexp(L, axis=0) - math.log(M)
    if np.any(k > 0.7):
        warnings.warn("the Pareto k of %d of the %d data points is above 0.7"
                      % (int(np.sum(k > 0.7)), nE), UserWarning)
    return dict(elpd_loo=float(elpd_i.sum()), p_loo=float((lppd_i - elpd_i).sum()), se=_se(elpd_i),
                elpd_loo_i=elpd_i, pareto_k=k, n_tail=n, tail_length=Mt, lppd_i=lppd_i,
                n_samples=M, n_data=nE)
