"""A float64 NumPy restatement of what naima_amd.evidence's kernels compute (nh_chain_cov,
nh_mvn_draw, nh_mvn_logpdf, nh_bridge_l2, nh_bridge_sums) and of ``bridge_sampling`` itself,
written from the definitions (Meng & Wong 1996; Gronau et al. 2017, the "normal" method).  It
shares Philox4x32-10 with tests/predictive_np.py.  The tests hold the device to it;
tests/test_evidence_host.py holds IT to closed-form evidences.  No GPU, no naima_amd import."""
import math

import numpy as np

from predictive_np import MASK, S32, philox4x32

MVN_STREAM = 0x4D564E31  # counter word 3 of the proposal stream (nh_ppc_rows' is 0)
LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------
def pooled(x, row0, nrows, ld, cstride, npool, d):
    """the pooled rows [nrows * npool][d] of the flat buffer x, as the kernels address them"""
    x = np.asarray(x, dtype=float).ravel()
    t = np.arange(nrows)[:, None, None]
    j = np.arange(npool)[None, :, None]
    c = np.arange(d)[None, None, :]
    return x[(row0 + t) * ld + j * cstride + c].reshape(nrows * npool, d)


def chain_cov(rows):
    """(mean [d], cov [d][d]) of rows [S][d], unbiased; a column with a non-finite value is NaN in
    the mean and in its row and column of the covariance; S = 1 gives a NaN covariance"""
    rows = np.atleast_2d(np.asarray(rows, dtype=float))
    S, d = rows.shape
    bad = ~np.isfinite(rows).all(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(bad, np.nan, np.where(bad, 0.0, rows).sum(axis=0) / S)
        c = np.where(bad, 0.0, rows) - np.where(bad, 0.0, mean)
        cov = (c.T @ c) / np.float64(S - 1)
    cov[bad, :] = np.nan
    cov[:, bad] = np.nan
    return mean, cov


def u52(hi, lo):
    return (((hi << np.uint64(20)) | (lo >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52


def normals(n, d, seed=0, row0=0, stream=MVN_STREAM):
    """z [n][d]: Box-Muller on Philox4x32-10 of counter (lo32(row), hi32(row), c >> 1, stream)
    under key (lo32(seed), hi32(seed)); an even column takes the cosine, an odd one the sine"""
    seed = int(seed) & (2 ** 64 - 1)
    row = (np.arange(n, dtype=np.uint64) + np.uint64(row0))[:, None]
    c = np.arange(d, dtype=np.uint64)[None, :]
    r0, r1, r2, r3 = np.broadcast_arrays(*philox4x32(
        (row & MASK, row >> S32, c >> np.uint64(1), stream), (seed & 0xFFFFFFFF, seed >> 32)))
    rad = np.sqrt(-2.0 * np.log(u52(r0, r1)))
    ang = 2.0 * np.pi * u52(r2, r3)
    return rad * np.where((c & np.uint64(1)).astype(bool), np.sin(ang), np.cos(ang))


def mvn_draw(mean, L, n, seed=0, row0=0):
    """(theta [n][d] = mean + L z, z2 [n] = |z|^2)"""
    mean, L = np.asarray(mean, dtype=float), np.tril(np.asarray(L, dtype=float))
    z = normals(n, len(mean), seed, row0)
    return mean + z @ L.T, (z * z).sum(axis=1)


def lognorm(L):
    L = np.asarray(L, dtype=float)
    return -0.5 * len(L) * LOG_2PI - np.log(np.diag(L)).sum()


def mvn_logpdf(theta, mean, L):
    """log N(theta; mean, L L^T) of every row by forward substitution; NaN for a row with a
    non-finite entry"""
    theta = np.atleast_2d(np.asarray(theta, dtype=float))
    mean, L = np.asarray(mean, dtype=float), np.tril(np.asarray(L, dtype=float))
    d = len(mean)
    ok = np.isfinite(theta).all(axis=1)
    y = np.zeros((len(theta), d))
    c = np.where(ok[:, None], theta, 0.0) - mean
    for i in range(d):
        y[:, i] = (c[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    out = lognorm(L) - 0.5 * (y * y).sum(axis=1)
    out[~ok] = np.nan
    return out


def bridge_l2(lp, z2, L):
    return np.asarray(lp, dtype=float) - (lognorm(L) - 0.5 * np.asarray(z2, dtype=float))


def bridge_terms(l1, l2, lstar, s1, s2, r):
    """(f1 [N2], f2 [N1]): f(l2 - lstar) = e^x / (s1 e^x + s2 r) and g(l1 - lstar) =
    1 / (s1 e^x + s2 r), both through e^-x where x > 0"""
    def both(l):
        x = np.asarray(l, dtype=float) - lstar
        pos = x > 0
        em = np.exp(-np.where(pos, x, 0.0))
        ex = np.exp(np.where(pos, 0.0, x))
        f = np.where(pos, 1.0 / (s1 + s2 * r * em), ex / (s1 * ex + s2 * r))
        g = np.where(pos, em / (s1 + s2 * r * em), 1.0 / (s1 * ex + s2 * r))
        return f, g
    return both(l2)[0], both(l1)[1]


def bridge_sums(l1, l2, lstar, s1, s2, r):
    f1, f2 = bridge_terms(l1, l2, lstar, s1, s2, r)
    return f1.sum(), f2.sum()


# ---------------------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------------------
def bridge_from_l(l1, l2, neff, log_prior_norm=0.0, tol=1e-10, maxiter=1000, tau=1.0):
    """the iteration and its error from l1 [N1] (posterior) and l2 [N2] (proposal);
    ``tau`` is the integrated autocorrelation time of the f2 sequence (1 for independent draws)"""
    l1, l2 = np.asarray(l1, dtype=float), np.asarray(l2, dtype=float)
    N1, N2 = len(l1), len(l2)
    lstar = float(np.median(l1))
    s1, s2 = neff / (neff + N2), N2 / (neff + N2)
    r, it, done = 1.0, 0, False
    while it < maxiter and not done:
        num, den = bridge_sums(l1, l2, lstar, s1, s2, r)
        new = (num / N2) / (den / N1)
        it += 1
        done = abs(new - r) / new < tol
        r = new
    f1, f2 = bridge_terms(l1, l2, lstar, s1, s2, r)
    re2 = f1.var(ddof=1) / (f1.mean() ** 2 * N2) + tau * f2.var(ddof=1) / (f2.mean() ** 2 * N1)
    top = l2[np.isfinite(l2)].max()
    logz_is = top + math.log(np.exp(l2 - top).sum()) - math.log(N2) - log_prior_norm
    return dict(logz=math.log(r) + lstar - log_prior_norm, logz_err=math.sqrt(re2),
                logz_is=logz_is, iterations=it, converged=done, n_post=N1, n_draws=N2,
                neff=float(neff), lstar=lstar, r=r, s1=s1, s2=s2)


def bridge_sampling(fit, post, logp, log_prob_fn, seed=0, n_draws=None, neff=None,
                    log_prior_norm=0.0, tol=1e-10, maxiter=1000, tau=1.0):
    """``bridge_sampling`` of pooled rows: ``fit`` [S0][d] gives the proposal, ``post`` [N1][d]
    with its log-probabilities ``logp`` [N1] is iterated on; ``neff`` defaults to N1"""
    fit, post = np.atleast_2d(fit), np.atleast_2d(post)
    mean, cov = chain_cov(fit)
    L = np.linalg.cholesky(cov)
    N1 = len(post)
    N2 = N1 if n_draws is None else int(n_draws)
    l1 = np.asarray(logp, dtype=float) - mvn_logpdf(post, mean, L)
    theta, z2 = mvn_draw(mean, L, N2, seed)
    lq = np.asarray(log_prob_fn(theta), dtype=float)
    out = bridge_from_l(l1, bridge_l2(lq, z2, L), N1 if neff is None else neff, log_prior_norm,
                        tol, maxiter, tau)
    out.update(forbidden_fraction=float(np.mean(lq == -np.inf)), mean=mean, cov=cov, l1=l1,
               l2=bridge_l2(lq, z2, L))
    return out
