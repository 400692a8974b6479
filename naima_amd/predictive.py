"""Posterior predictive checks from a chain's stored spectra: does the fitted model describe the
data at all?  ``BIC``, ``waic`` and ``loo`` rank models against each other; two bad models still
get ranked.  Here the data are compared with what the fitted model itself would have produced.

A fit keeps every walker's model spectrum at the data's energies for every stored step (blob 0).
For each of those M spectra ``nh_ppc_rows`` draws one replicated data set from the sampling
distribution naima's likelihood implies (core.py:76-85 and ``infocrit``'s docstring): a datum y
given the model m is split normal, with scale ``flux_error_hi`` on the side y < m and
``flux_error_lo`` on the side y > m.  Of the observed and of the replicated data it takes three
discrepancy statistics over the points that are not upper limits, with the standardised residual
r = (data - model) / error, the error being the one the likelihood uses on that side:

  chi2    sum r^2: for the observed data -2 x the likelihood's sum over those points;
  maxabs  max |r|: a single outlier;
  runs    1 + the number of sign changes of r between neighbouring points in energy (Wald &
          Wolfowitz): residuals that stay inside their error bars but on one side of the model
          over a stretch of energies -- a smooth feature the model cannot make -- leave chi2
          unremarkable and runs far too low.

The Bayesian p-values (Gelman, Meng & Stern 1996) are the fractions of posterior samples whose
replicate is at least as extreme: ``p_chi2 = P(chi2_rep >= chi2_obs)``, ``p_max`` likewise,
``p_runs = P(runs_rep <= runs_obs)``; a SMALL p is a misfit in all three (``nh_ppc_counts``).
``pit`` is the probability integral transform of each datum under its posterior predictive
distribution, the mean over the samples of the split-normal CDF (``nh_pit_columns``): values
near 0 or 1 are points in the tails, and a run of values on one side of 1/2 is the same
structure ``runs`` counts.  Upper limits are not replicated; for them ``ul_violation`` is the
fraction of samples above the limit.

The random stream is counter-based (Philox4x32-10, key = ``seed``, counter = (row, column)): a
value depends on (seed, global row, column) alone, so results are reproducible, independent of
the launch shape and the same however the rows are cut into calls (``row0``).

Every function takes the model as ``pointwise_log_likelihood`` does.  Importing this module
creates no GPU context; argument errors come before any device work; there is no CPU fallback.
"""
import numpy as np

from .dview import as_matrix, matrix_on, matrix_shape

__all__ = ["posterior_predictive", "ppc", "pit", "predictive_quantiles", "PredictiveMixin",
           "T_COLUMNS"]

# the columns of the statistics matrix ``ppc`` returns as ``T``
T_COLUMNS = ("chi2_obs", "chi2_rep", "maxabs_obs", "maxabs_rep", "runs_obs", "runs_rep")


# ---------------------------------------------------------------------------------------
# arguments (no device)
# ---------------------------------------------------------------------------------------
def _int_in(name, v, hi):
    try:
        ok = int(v) == v and not isinstance(v, bool)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 0 <= int(v) < hi:
        raise ValueError("%s must be an integer in [0, 2^%d), not %r"
                         % (name, hi.bit_length() - 1, v))
    return int(v)


def _check(model, data, unit, seed=0, row0=0):
    """(values, unit, M, nE, seed, row0) of the arguments, without a device"""
    from .infocrit import _model_values
    seed, row0 = _int_in("seed", seed, 2 ** 64), _int_in("row0", row0, 2 ** 63)
    return _model_values(model, data, unit) + (seed, row0)


def _n_ul(data):
    return int(np.count_nonzero(np.asarray(data["ul"])))


def _check_q(q):
    q = np.atleast_1d(np.asarray(q, dtype=float))
    if q.ndim != 1 or q.size == 0 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("quantiles must lie in [0, 1]")
    return q


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
def _rows(values, unit, data, M, nE, seed, row0, want_y, want_t):
    """nh_ppc_rows: (the spectra's handle, Y handle or None, T handle or None)"""
    from .core import _data_on_device
    s = as_matrix(values)
    ctx = s.ctx
    dd = _data_on_device(ctx, data)
    Y = ctx.empty((M, nE)) if want_y else None
    T = ctx.empty((M, 6)) if want_t else None
    ctx.call("nh_ppc_rows", s.ptr, M, nE, s.ld, dd.conv(unit), dd.flux, dd.elo, dd.ehi, dd.ul,
             seed, row0, Y, nE, T)
    return (s, None if Y is None else matrix_on(Y, M, nE),
            None if T is None else matrix_on(T, M, 6))


def _pit(s, unit, data, nE):
    from .core import _data_on_device
    dd = _data_on_device(s.ctx, data)
    out = s.ctx.empty((2, nE))
    s.ctx.call("nh_pit_columns", s.ptr, s.M, nE, s.ld, dd.conv(unit), dd.flux, dd.elo, dd.ehi,
               dd.ul, out)
    return out.get()


def posterior_predictive(model, data, unit=None, seed=0, row0=0):
    """One replicated data set per posterior sample, in the data's unit, as a device matrix
    handle (M, n_data) (``.get()`` downloads it; ``predictive_quantiles`` takes it as it is): row
    s is a draw from the likelihood's sampling distribution around spectrum s (module docstring);
    the column of an upper limit holds the model itself.

    ``model`` is a ``Quantity`` (M, n_data) in host memory, or a device matrix as
    ``dview.as_matrix`` accepts it together with its ``unit``.  Row s uses the stream of global
    row ``row0 + s``: a chain replicated in pieces gives the rows it gives in one call."""
    values, unit, M, nE, seed, row0 = _check(model, data, unit, seed, row0)
    return _rows(values, unit, data, M, nE, seed, row0, True, False)[1]


def pit(model, data, unit=None):
    """(pit, ul_violation), arrays [n_data]: the probability integral transform of every datum
    that is not an upper limit under its posterior predictive distribution (NaN at upper
    limits), and for every upper limit the fraction of samples above it (NaN elsewhere)."""
    values, unit, M, nE, _, _ = _check(model, data, unit)
    out = _pit(as_matrix(values), unit, data, nE)
    return out[0], out[1]


def ppc(model, data, unit=None, seed=0):
    """The posterior predictive check of M spectra against a data table (module docstring), as a
    dict: the Bayesian p-values ``p_chi2``, ``p_max``, ``p_runs`` (small = misfit); ``chi2_obs``
    and ``chi2_rep``, each a dict of ``mean`` (of the finite values), ``median``, ``q16``,
    ``q84`` over the samples, taken on the device; ``n_points`` (not upper limits), ``n_ul``,
    ``n_samples``, ``n_bad`` (samples with a non-finite statistic, left out of the p-values);
    ``pit`` and ``ul_violation`` [n_data]; and ``T``, the device handle of the matrix
    [M][6] = chi2_obs, chi2_rep, maxabs_obs, maxabs_rep, runs_obs, runs_rep
    (``posterior.histogram(T)`` and the like take it).  Raises ``ValueError`` when every point is
    an upper limit, and when no sample has finite statistics."""
    from .posterior import _quantiles, column_stats
    values, unit, M, nE, seed, _ = _check(model, data, unit, seed)
    n_ul = _n_ul(data)
    if n_ul == nE:
        raise ValueError("every data point is an upper limit: nothing to check")
    s, _, T = _rows(values, unit, data, M, nE, seed, 0, False, True)
    ctx = s.ctx
    counts = ctx.empty((4,), np.int64)
    ctx.call("nh_ppc_counts", T.ptr, M, counts)
    c = [int(v) for v in counts.get()]
    good = M - c[3]
    if good == 0:
        raise ValueError("none of the %d samples has finite statistics (a NaN in every "
                         "spectrum, a zero error?)" % M)
    mean = column_stats(T)["mean"]
    q = _quantiles(T, [0.16, 0.5, 0.84])
    out = dict(p_chi2=c[0] / good, p_max=c[1] / good, p_runs=c[2] / good)
    for j, name in ((0, "chi2_obs"), (1, "chi2_rep")):
        out[name] = dict(mean=float(mean[j]), median=float(q[1][j]), q16=float(q[0][j]),
                         q84=float(q[2][j]))
    pv = _pit(s, unit, data, nE)
    out.update(n_points=nE - n_ul, n_ul=n_ul, n_samples=M, n_bad=c[3], pit=pv[0],
               ul_violation=pv[1], T=T)
    return out


def predictive_quantiles(y_rep, q):
    """``np.percentile(y_rep, 100 q, axis=0)``: the quantiles ``q`` (in [0, 1]) of every column
    of a replicate matrix (what ``posterior_predictive`` returns, or a host array), [len(q)]
    [n_data], from exact order statistics taken on the device (``nh_column_select``).  These are
    PREDICTIVE bands: they hold the noise of the data, unlike ``plot_fit``'s model bands."""
    from .posterior import _quantiles
    q = _check_q(q)
    matrix_shape(y_rep, pointwise=True)
    return _quantiles(as_matrix(y_rep), q)


# ---------------------------------------------------------------------------------------
# a sampler's (or a read run's) stored spectra
# ---------------------------------------------------------------------------------------
class PredictiveMixin:
    """``get_posterior_predictive`` and ``ppc`` of an object with ``get_blobs``, ``blob_units``
    and ``data`` (EnsembleSampler, read_run's result); collective on several ranks, as
    ``get_blobs``"""

    def get_posterior_predictive(self, discard=0, thin=1, modelidx=0, seed=0):
        """``predictive.posterior_predictive`` of the stored spectra of blob ``modelidx`` of
        every (step, walker) that ``get_blobs(discard=discard, thin=thin)`` selects"""
        from .infocrit import sampler_spectra
        _int_in("seed", seed, 2 ** 64)
        return posterior_predictive(*sampler_spectra(self, discard, thin, modelidx), seed=seed)

    def ppc(self, discard=0, thin=1, modelidx=0, seed=0):
        """``predictive.ppc`` of the same spectra"""
        from .infocrit import sampler_spectra
        _int_in("seed", seed, 2 ** 64)
        return ppc(*sampler_spectra(self, discard, thin, modelidx), seed=seed)
