"""The marginal likelihood (evidence) of a fit and Bayes factors between fits, by bridge sampling
on the GPU.

READ THIS FIRST.  ``Z`` is the integral of ``exp(lnprob(theta))`` over the parameters, of the
log-probability EXACTLY AS IT IS WRITTEN.  naima's ``uniform_prior`` returns 0 inside its interval
(not ``-log(umax - umin)``) and its ``normal_prior`` is not normalised either, so the number is an
evidence only when

* every parameter has a PROPER prior -- a bounded ``uniform_prior`` or a ``normal_prior``; with
  an improper prior (no prior at all, a half-open interval) the integral has no meaning and
  neither has the number returned, although one IS returned; and
* ``log_prior_norm`` carries the normalisation the priors leave out: the sum over the parameters
  of ``log(umax - umin)`` for a uniform prior, and the like.  It is subtracted from ``logz``.

The likelihood's own constant (the normalisation of the errors, a function of the data table
alone) is left out as it is under ``BIC``, ``waic`` and ``loo``: it cancels in a Bayes factor
between models fitted to the SAME table, and only such differences mean anything.

The estimator is Meng & Wong's (1996) iterative bridge-sampling estimate with a multivariate
normal proposal, the "normal" method of Gronau et al. (2017) and of R's ``bridgesampling``.  The
stored rows behind ``discard`` are split by step into two halves.  The first gives the mean and
covariance of the proposal g (``nh_chain_cov``).  With ``l1 = lnprob - log g`` at the N1 pooled
samples of the second half (``nh_mvn_logpdf``), ``l2`` the same at N2 draws from g
(``nh_mvn_draw``, one batched call of the log-probability function, ``nh_bridge_l2``),
``lstar = median(l1)``, ``s1 = neff / (neff + N2)`` and ``s2 = N2 / (neff + N2)``::

    r <- [ 1/N2 sum_j f(l2_j - lstar) ] / [ 1/N1 sum_i g(l1_i - lstar) ]
    f(x) = e^x / (s1 e^x + s2 r),   g(x) = 1 / (s1 e^x + s2 r)

from r = 1 until ``|delta r| / r < tol`` (``nh_bridge_sums``: a launch pair and a 16-byte
download per iteration), and ``logz = log r + lstar - log_prior_norm``.  ``neff`` is the
effective size of the second half, which discounts its autocorrelation.

The chain and its log-probabilities are read where they lie in HBM; only the d x d covariance
(whose Cholesky factor is host arithmetic), the N2 proposals (for the log-probability function)
and a few scalars cross the bus.  Every floating-point sum has a fixed order and the draws come
from a counter-based stream (Philox4x32-10 under ``seed``), so a call is reproducible bit for bit.
There is no CPU fallback.  Importing this module creates no GPU context; argument errors come
before any device work.
"""
import math
import warnings

import numpy as np

from ._lib import NH_EVID_MAX_DIM
from .dview import DeviceChain, as_chain, chain_dims, matrix_on

__all__ = ["bridge_sampling", "bayes_factor", "EvidenceMixin"]


# ---------------------------------------------------------------------------------------
# arguments (no device)
# ---------------------------------------------------------------------------------------
def _pos_int(name, v, hi=2 ** 31):
    try:
        ok = int(v) == v and not isinstance(v, bool)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 1 <= int(v) < hi:
        raise ValueError("%s must be a positive integer below 2^%d, not %r"
                         % (name, hi.bit_length() - 1, v))
    return int(v)


def _pos_float(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError("%s must be a positive finite number, not %r" % (name, v))
    return f


def _logp(chain, log_prob, rows, nw):
    """the log-probabilities of a chain of (rows, nw) as ``as_chain`` takes them: a host array of
    that shape beside a host chain, the DeviceMatrix of a device array of rows * nw values (or of
    a tuple that starts with one) beside a device chain, None for those a DeviceChain carries"""
    if log_prob is None and getattr(chain, "logp", None) is not None:
        return None
    dev = log_prob[0] if isinstance(log_prob, tuple) and len(log_prob) else log_prob
    if hasattr(dev, "ptr") != isinstance(chain, (tuple, DeviceChain)):
        raise ValueError("chain and log_prob must both be host arrays or both device blocks")
    if hasattr(dev, "ptr"):  # (a tuple's own shape: the chain refuses one that is not its own)
        return matrix_on(dev, *(log_prob[1:3] if isinstance(log_prob, tuple) else (rows, nw)))
    if np.shape(log_prob) != (rows, nw):
        raise ValueError("log_prob must be (rows, nwalkers) = (%d, %d), not %r"
                         % (rows, nw, np.shape(log_prob)))
    return log_prob


def _check(chain, log_prob, log_prob_fn, seed, n_draws, neff, log_prior_norm, tol, maxiter,
           discard, batch):
    from .predictive import _int_in
    rows, nw, ndim = chain_dims(chain, discard, 2)
    if ndim > NH_EVID_MAX_DIM:
        raise ValueError("%d parameters are more than the %d the covariance kernels take"
                         % (ndim, NH_EVID_MAX_DIM))
    discard = int(discard)
    n = rows - discard
    h = n // 2
    logp = _logp(chain, log_prob, rows, nw)
    if not callable(log_prob_fn):
        raise ValueError("log_prob_fn must be callable")
    seed = _int_in("seed", seed, 2 ** 64)
    N1 = (n - h) * nw
    N2 = N1 if n_draws is None else _pos_int("n_draws", n_draws)
    if N1 >= 2 ** 31:
        raise ValueError("the second half holds 2^31 samples or more")
    neff = None if neff is None else _pos_float("neff", neff)
    lpn = float(log_prior_norm)
    if not math.isfinite(lpn):
        raise ValueError("log_prior_norm must be finite")
    tol = _pos_float("tol", tol)
    maxiter = _pos_int("maxiter", maxiter)
    batch = nw if batch is None else _pos_int("batch", batch)
    return dict(logp=logp, nw=nw, ndim=ndim, discard=discard, h=h, n2=n - h, N1=N1, N2=N2,
                seed=seed, neff=neff, lpn=lpn, tol=tol, maxiter=maxiter, batch=batch)


def bayes_factor(a, b):
    """(log B_ab, its standard error) of two ``bridge_sampling`` results (or any mappings with
    ``logz`` and ``logz_err``): ``logz_a - logz_b`` and the root sum of squares of the two errors.
    Positive favours ``a``.  Both fits must be to the same data table (module docstring)."""
    try:
        za, zb = float(a["logz"]), float(b["logz"])
        ea, eb = float(a["logz_err"]), float(b["logz_err"])
    except (TypeError, KeyError, IndexError):
        raise ValueError("bayes_factor takes two results of bridge_sampling (logz, logz_err)")
    return za - zb, math.hypot(ea, eb)


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
def _evaluate(log_prob_fn, theta, batch):
    """the log-probability at the proposals theta [N2][ndim] (host), ``batch`` rows a call"""
    out = np.empty(len(theta))
    for a in range(0, len(theta), batch):
        v = np.asarray(log_prob_fn(theta[a:a + batch]), dtype=float)
        out[a:a + batch] = np.broadcast_to(v, (len(theta[a:a + batch]),))
    if np.any(np.isnan(out)):
        raise ValueError("Probability function returned NaN")
    if np.any(out == np.inf):
        raise ValueError("Probability function returned +inf")
    return out


def bridge_sampling(chain, log_prob, log_prob_fn, seed=0, n_draws=None, neff=None,
                    log_prior_norm=0.0, tol=1e-10, maxiter=1000, discard=0, batch=None):
    """The log marginal likelihood of a chain by bridge sampling (module docstring: the priors
    must be proper and ``log_prior_norm`` must carry their normalisation).

    ``chain`` (rows, nwalkers, ndim) and ``log_prob`` (rows, nwalkers) are host arrays, as
    ``get_chain()`` and ``get_log_prob()`` return them, which are uploaded once; or device blocks:
    ``(DeviceArray, rows, nwalkers, ndim)`` laid out [rows][nwalkers * ndim], and a DeviceArray
    [rows][nwalkers] (or a tuple ``(DeviceArray, rows, nwalkers)``); or a ``dview.DeviceChain``,
    with ``log_prob=None`` where it carries its ``logp``.  ``log_prob_fn(theta[n, ndim])
    -> lnprob[n]`` is the function the chain was sampled from, called with host arrays of
    ``batch`` rows (default ``nwalkers``); ``-inf`` marks a point the prior forbids; NaN and +inf
    raise ``ValueError``.  ``n_draws`` = N2 proposals (default N1, the size of the second half);
    ``neff`` defaults to the median over the parameters of ``posterior.ess(second half, "bulk")``,
    capped at N1 (N1 itself, with a warning, where no parameter has a finite one).  ndim <= 32.

    Returns a dict: ``logz``; ``logz_err``, its standard error from the relative mean-squared
    error ``Var(f1) / (mean(f1)^2 N2) + tau Var(f2) / (mean(f2)^2 N1)`` of Fruehwirth-Schnatter
    (2004), f1 and f2 the terms of the two sums at the last iteration and ``tau`` emcee's
    integrated autocorrelation time (in steps) of the f2 sequence (NaN when a walker did not move
    in the second half); ``logz_is``, the plain importance-sampling estimate
    ``logsumexp(l2) - log N2 - log_prior_norm`` from the same draws, a cross-check with a much
    wider scatter; ``iterations``, ``converged``, ``n_post`` = N1, ``n_draws`` = N2, ``neff``,
    ``forbidden_fraction`` (the share of proposals with lnprob = -inf: a large one says the
    posterior leans on a prior bound, which a normal proposal covers badly), and the proposal's
    ``mean`` [ndim] and ``cov`` [ndim][ndim].

    Raises ``ValueError`` when the first half's covariance is not positive definite (too few
    rows, a parameter that never moved, a non-finite value), when a stored log-probability or a
    sample of the second half is not finite, and when every proposal is forbidden.  Reaching
    ``maxiter`` warns and sets ``converged`` to False."""
    a = _check(chain, log_prob, log_prob_fn, seed, n_draws, neff, log_prior_norm, tol, maxiter,
               discard, batch)
    from .posterior import _taus, column_stats, ess
    from .plot import column_select
    nw, ndim, N1, N2 = a["nw"], a["ndim"], a["N1"], a["N2"]
    chain = as_chain(chain, a["discard"], 2, logp=a["logp"])
    ctx = chain.ctx
    fit, post = chain.rows(0, a["h"]), chain.behind(a["h"])

    # the proposal: mean and covariance of the first half, its Cholesky factor
    mean_d, cov_d = ctx.empty((ndim,)), ctx.empty((ndim, ndim))
    ctx.call("nh_chain_cov", *fit.pooled(), mean_d, cov_d)
    mean, cov = mean_d.get(), cov_d.get()
    try:
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))):
            raise np.linalg.LinAlgError("not finite")
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError("the covariance of the first half of the chain (%d samples of %d "
                         "parameters) is not positive definite" % (a["h"] * nw, ndim))
    L_d = ctx.array(L)

    # l1 = lnprob - log g at the second half
    l1 = ctx.empty((N1,))
    ctx.call("nh_mvn_logpdf", *post.pooled(), mean_d, L_d, post.logp.ptr, l1)
    v1 = matrix_on(l1, N1, 1)
    if int(column_stats(v1)["n"][0]) != N1:
        raise ValueError("the second half of the chain holds a non-finite log-probability or "
                         "sample (a walker that started outside the prior and has not moved in "
                         "yet? discard more rows, or start every walker inside)")
    if a["neff"] is None:
        e = ess(post, "bulk")
        if np.any(np.isfinite(e)):
            neff = min(float(np.nanmedian(e)), float(N1))
        else:
            warnings.warn("the effective sample size of the second half cannot be estimated (a "
                          "walker that never moved, too few rows): neff = N1 = %d is used, which "
                          "ignores the chain's autocorrelation; pass neff" % N1)
            neff = float(N1)
    else:
        neff = a["neff"]

    # l2 = lnprob - log g at N2 draws from g
    theta, z2 = ctx.empty((N2, ndim)), ctx.empty((N2,))
    ctx.call("nh_mvn_draw", mean_d, L_d, ndim, a["seed"], 0, N2, theta, ndim, z2)
    lq = _evaluate(log_prob_fn, theta.get(), a["batch"])
    forbidden = float(np.mean(lq == -np.inf))
    if forbidden == 1.0:
        raise ValueError("every proposal is forbidden by the prior (lnprob = -inf)")
    l2 = ctx.empty((N2,))
    ctx.call("nh_bridge_l2", ctx.array(lq), z2, N2, L_d, ndim, l2)

    # the iteration
    S = N1
    v = column_select(v1, [(S - 1) // 2, S // 2])
    lstar = 0.5 * float(v[0, 0] + v[1, 0])
    s1, s2 = neff / (neff + N2), N2 / (neff + N2)
    sums = ctx.empty((2,))
    r, it, done = 1.0, 0, False
    while it < a["maxiter"] and not done:
        ctx.call("nh_bridge_sums", l1, N1, l2, N2, lstar, s1, s2, r, sums, None, None)
        num, den = sums.get()
        new = (num / N2) / (den / N1)
        if not (new > 0.0 and math.isfinite(new)):
            raise ValueError("the bridge-sampling iteration left the positive numbers (r = %r): "
                             "the proposal does not overlap the posterior" % new)
        it += 1
        done = abs(new - r) / new < a["tol"]
        r = new
    if not done:
        warnings.warn("bridge sampling did not converge in %d iterations (tol = %g)"
                      % (a["maxiter"], a["tol"]))

    # the error, from the terms at the r reached
    f1, f2 = ctx.empty((N2,)), ctx.empty((N1,))
    ctx.call("nh_bridge_sums", l1, N1, l2, N2, lstar, s1, s2, r, sums, f1, f2)
    m1, m2 = column_stats(matrix_on(f1, N2, 1)), column_stats(matrix_on(f2, N1, 1))
    f2_chain = DeviceChain(matrix_on(f2, a["n2"], nw), nw, 1)  # (one parameter: f2 per walker)
    tau = float(_taus(f2_chain, 5)[0]) if a["n2"] > 1 else 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = (m1["var"][0] / (m1["mean"][0] ** 2 * N2)) if N2 > 1 else 0.0
        t2 = (tau * m2["var"][0] / (m2["mean"][0] ** 2 * N1)) if N1 > 1 else 0.0
        err = float(np.sqrt(t1 + t2))

    # importance sampling from the same draws: sum_j exp(l2_j - max l2) is the numerator's sum
    # with s1 = 0, s2 r = 1
    top = float(column_stats(matrix_on(l2, N2, 1))["max"][0])
    ctx.call("nh_bridge_sums", l1, N1, l2, N2, top, 0.0, 1.0, 1.0, sums, None, None)
    logz_is = top + math.log(float(sums.get()[0])) - math.log(N2) - a["lpn"]

    return dict(logz=math.log(r) + lstar - a["lpn"], logz_err=err, logz_is=logz_is,
                iterations=it, converged=bool(done), n_post=N1, n_draws=N2, neff=float(neff),
                forbidden_fraction=forbidden, mean=mean, cov=cov)


# ---------------------------------------------------------------------------------------
# a sampler's chain
# ---------------------------------------------------------------------------------------
class EvidenceMixin:
    """``log_evidence`` of an EnsembleSampler"""

    def log_evidence(self, discard=0, **kw):
        """``evidence.bridge_sampling`` of the stored chain and its stored log-probabilities --
        read from the history block in HBM where the device loop still holds the whole chain
        there, else from ``get_chain()`` and ``get_log_prob()`` -- with the sampler's own
        log-probability function (``compute_log_prob``, so ``nan_policy`` applies as in a run).
        ``kw`` are bridge_sampling's (``seed``, ``n_draws``, ``neff``, ``log_prior_norm``, ``tol``,
        ``maxiter``, ``batch``).  PRIORS MUST BE PROPER and ``log_prior_norm`` must carry their
        normalisation: see the module docstring of ``naima_amd.evidence``.

        One rank only (``NotImplementedError`` with walkers sharded over several).  The result of
        ``read_run`` has no such method, because a saved run has no log-probability function:
        call ``evidence.bridge_sampling(run.get_chain(), run.get_log_prob(), fn)`` with one."""
        if self.comm.size > 1:
            raise NotImplementedError("log_evidence with walkers sharded over several ranks")
        if "log_prob_fn" in kw:
            raise ValueError("log_evidence evaluates the sampler's own log-probability function")

        def fn(theta):
            return self.compute_log_prob(np.ascontiguousarray(theta))[0]

        block = self._chain_block(1)
        if block is not None:
            return bridge_sampling(block, None, fn, discard=discard, **kw)
        return bridge_sampling(self.get_chain(), self.get_log_prob(), fn, discard=discard, **kw)
