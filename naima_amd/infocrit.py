"""Model comparison from a chain's stored spectra: the pointwise log-likelihood matrix, WAIC and
Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO), reduced on the GPU.

A fit keeps every walker's model spectrum at the data's energies for every stored step (blob 0).
``pointwise_log_likelihood`` turns those M spectra into the matrix ``L[sample][data point]`` of
the likelihood's per-point terms (``nh_pointwise_lnl``); ``waic`` and ``loo`` reduce its columns
on the device (``nh_lnl_column_stats``, ``nh_column_select``, ``nh_psis_columns``) and bring
``n_data`` numbers back; ``compare`` ranks several models fitted to the same data table, which is
host arithmetic on those numbers.  There is no CPU fallback for the reductions.

The constant.  naima's likelihood (core.py:64-94) omits the normalisation of the errors, which
depends on the data alone; for asymmetric errors the term is that of a split normal, whose
normalisation sqrt(2/pi) / (elo + ehi) does not depend on the model either.  Every elpd here is
therefore defined up to a constant of the data table, like the ``ML`` under ``BIC``: DIFFERENCES
between models on the same table are what is meaningful.  ``p_waic`` and ``p_loo`` do not depend
on the constant.  An upper limit contributes ``log(1 - cl[nviol])`` when the model violates it,
``nviol`` being the number of limits that SAMPLE violates (the reference's quirk, core.py:89-92:
cl is indexed by the count); for a uniform ``cl`` this is the natural per-point penalty, and the
columns of a row sum to ``lnprobmodel`` of that row for any ``cl``.

PSIS follows Vehtari, Simpson, Gelman, Yao & Gabry with the generalised-Pareto fit of Zhang &
Stephens (2009) and the weak priors of the ``loo`` package: per data point k, with x = -L[:, k]
shifted to a maximum of 0, the tail is the rows above the order statistic M - Mt - 1 of x
(strictly: ties at the cutoff leave fewer than Mt), Mt = min(M // 5, ceil(3 sqrt(M / reff)));
with at most 4 tail rows ``pareto_k`` is +inf and nothing is smoothed; otherwise the sorted tail
is replaced by the fitted distribution's quantiles at (i + 0.5) / n, capped at 0.  Where a
smoothed value would be positive it becomes exactly 0 (``loo`` truncates at the largest raw
weight, which is 0 after the shift).  The tail lives in one workgroup's LDS: Mt above
``NH_PSIS_MAX_TAIL`` = 4096 (a chain of more than 1.8 million rows at reff = 1) raises, thin the
chain.

Every function takes ``L`` as a host array ``(M, n_data)``, which is uploaded once per call, or
as a device matrix: a ``dview.DeviceMatrix`` (what ``pointwise_log_likelihood`` returns), or
``(DeviceArray, M, ncol, ld)``.  Importing this module creates no GPU context; argument errors
come before any device work.
"""
import math
import warnings

import numpy as np

from ._lib import NH_PSIS_MAX_TAIL
from .dview import as_matrix, matrix_on, matrix_shape

__all__ = ["pointwise_log_likelihood", "waic", "loo", "compare", "tail_length", "PARETO_K_WARN"]

PARETO_K_WARN = 0.7  # above it the PSIS estimate of a point is not reliable (Vehtari et al.)


# ---------------------------------------------------------------------------------------
# host arithmetic
# ---------------------------------------------------------------------------------------
def tail_length(M, reff=1.0):
    """Mt = min(M // 5, ceil(3 sqrt(M / reff))), the number of largest importance ratios the
    generalised Pareto distribution is fitted to; ``reff`` is the relative efficiency of the
    chain, n_eff / M (1 for independent draws)"""
    try:
        reff = float(reff)
    except (TypeError, ValueError):
        raise ValueError("reff must be a positive finite number")
    if not (reff > 0.0 and math.isfinite(reff)):
        raise ValueError("reff must be a positive finite number, not %r" % (reff,))
    M = int(M)
    if M < 1:
        raise ValueError("no samples")
    Mt = min(M // 5, int(math.ceil(3.0 * math.sqrt(M / reff))))
    if Mt > NH_PSIS_MAX_TAIL:
        raise ValueError("a tail of %d of the %d samples is more than the %d one workgroup sorts: "
                         "thin the chain (get_pointwise_log_likelihood(thin=...))"
                         % (Mt, M, NH_PSIS_MAX_TAIL))
    return Mt


def _se(elpd_i):
    """sqrt(n var(elpd_i, ddof=1)): the standard error of a sum of n pointwise values"""
    n = len(elpd_i)
    return float(np.sqrt(n * np.var(elpd_i, ddof=1))) if n > 1 else float("nan")


def compare(results, names=None, ic="loo"):
    """Rank the ``loo`` (``ic="loo"``) or ``waic`` (``ic="waic"``) results of several models
    fitted to the SAME data table by their elpd, best first.  Returns a list of dicts: ``name``
    (``names[i]``, default the index in ``results``), ``rank``, ``elpd``, ``p`` (the effective
    number of parameters), ``se``, ``elpd_diff`` to the best model (0 for it, negative below) and
    ``dse = sqrt(n_data var(elpd_i^best - elpd_i^m, ddof=1))``, the standard error of that
    difference (0 for the best model).  The constant of the data table cancels in ``elpd_diff``
    and ``dse``."""
    if ic not in ("loo", "waic"):
        raise ValueError("ic must be 'loo' or 'waic'")
    results = list(results)
    if not results:
        raise ValueError("no results to compare")
    if names is None:
        names = list(range(len(results)))
    names = list(names)
    if len(names) != len(results):
        raise ValueError("%d names for %d results" % (len(names), len(results)))
    key = "elpd_%s_i" % ic
    pw = []
    for name, r in zip(names, results):
        if key not in r:
            raise ValueError("result %r has no %s: not a %s() result" % (name, key, ic))
        pw.append(np.asarray(r[key], dtype=float))
    n_data = {int(r["n_data"]) for r in results} | {len(v) for v in pw}
    if len(n_data) != 1:
        raise ValueError("the results are of different data tables: n_data = %s"
                         % sorted(n_data))
    elpd = [float(r["elpd_%s" % ic]) for r in results]
    order = sorted(range(len(results)), key=lambda i: -elpd[i])
    best = order[0]
    out = []
    for rank, i in enumerate(order):
        d = pw[best] - pw[i]
        out.append(dict(name=names[i], rank=rank, elpd=elpd[i], p=float(results[i]["p_%s" % ic]),
                        se=float(results[i]["se"]), elpd_diff=elpd[i] - elpd[best],
                        dse=0.0 if i == best else _se(d)))
    return out


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
def _model_values(model, data, unit):
    """(values, unit, M, nE) of a model argument -- a ``Quantity`` (M, n_data), or a matrix as
    ``dview.as_matrix`` accepts it together with its ``unit`` -- checked against the data
    table, without a device"""
    from . import units as u
    if isinstance(model, u.Quantity):
        if unit is not None and u.Unit(unit) != model.unit:
            raise ValueError("unit= contradicts the Quantity's own unit")
        unit, values = model.unit, model.value
    else:
        values = model
    if unit is None:
        raise ValueError("a model that is not a Quantity needs unit=")
    unit = u.Unit(unit)
    M, nE = matrix_shape(values, pointwise=True)
    n_data = int(np.size(data["flux"].value))
    if nE != n_data:
        raise ValueError("model has %d energies, data table has %d" % (nE, n_data))
    if M >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 samples")
    return values, unit, M, nE


def pointwise_log_likelihood(model, data, unit=None, totals=False):
    """L[s][k], the term of data point k in ``lnprobmodel`` of spectrum s (module docstring), as
    a device matrix handle (``.get()`` downloads it; ``waic`` and ``loo`` take it as it is).

    ``model`` is a ``Quantity`` (M, n_data) in host memory, or a device matrix as
    ``dview.as_matrix`` accepts it together with its ``unit``; the conversion to the data's
    unit is ``core._conversion_to_data``, the one the fit itself used (SED <-> differential
    included).  ``totals=True`` returns (L, row sums as a device array [M]) instead.  A
    non-finite term raises ``ValueError`` with their number."""
    from .core import _data_on_device
    values, unit, M, nE = _model_values(model, data, unit)
    s = as_matrix(values)
    ctx = s.ctx
    dd = _data_on_device(ctx, data)
    L = ctx.empty((M, nE))
    total = ctx.empty((M,)) if totals else None
    nbad = ctx.empty((1,), np.int64)
    ctx.call("nh_pointwise_lnl", s.ptr, M, nE, s.ld, dd.conv(unit), dd.flux, dd.elo, dd.ehi, dd.ul,
             dd.cl, L, nE, total, nbad)
    bad = int(nbad.get()[0])
    if bad:
        raise ValueError("%d of the %d pointwise log-likelihood terms are not finite (a NaN in a "
                         "spectrum, a zero error, cl = 1?)" % (bad, M * nE))
    out = matrix_on(L, M, nE)
    return (out, total) if totals else out


def _column_stats(s):
    """nh_lnl_column_stats of a device matrix: the device array [5][ncol] = max, mean, var, lse,
    min"""
    stats = s.ctx.empty((5, s.ncol))
    s.ctx.call("nh_lnl_column_stats", s.ptr, s.M, s.ncol, s.ld, stats)
    return stats


def waic(L):
    """The widely applicable information criterion of a pointwise matrix ``L`` (Watanabe 2010;
    Vehtari, Gelman & Gabry 2017), as a dict: ``lppd_i = logsumexp_s L[s][i] - log M``,
    ``p_waic_i`` = the variance over the samples (ddof = 1), ``elpd_waic_i = lppd_i - p_waic_i``,
    their sums ``elpd_waic`` and ``p_waic`` (and ``lppd``), ``se = sqrt(n_data var(elpd_waic_i,
    ddof=1))``, ``n_samples`` and ``n_data``.  elpd is on the log-score scale (multiply by -2 for
    the deviance scale) and defined up to the data table's constant (module docstring)."""
    M, nE = matrix_shape(L, pointwise=True)
    s = as_matrix(L)
    st = _column_stats(s).get()
    lppd_i = st[3] - math.log(M)
    p_i = st[2]
    elpd_i = lppd_i - p_i
    return dict(elpd_waic=float(elpd_i.sum()), p_waic=float(p_i.sum()), lppd=float(lppd_i.sum()),
                se=_se(elpd_i), elpd_waic_i=elpd_i, p_waic_i=p_i, lppd_i=lppd_i, n_samples=M,
                n_data=nE)


def loo(L, reff=1.0):
    """PSIS leave-one-out cross-validation of a pointwise matrix ``L`` (module docstring), as a
    dict: ``elpd_loo_i``, their sum ``elpd_loo``, ``p_loo = sum(lppd_i - elpd_loo_i)``,
    ``se = sqrt(n_data var(elpd_loo_i, ddof=1))``, ``pareto_k`` [n_data] (+inf where the tail has
    at most 4 rows), ``n_tail`` [n_data] (int64), ``tail_length`` = Mt, ``lppd_i``, ``n_samples``
    and ``n_data``.  ``reff`` is the chain's relative efficiency n_eff / M (1 / tau of
    ``get_autocorr_time`` for a thinned-by-one chain); it only sets the tail length.  Warns when
    a ``pareto_k`` exceeds 0.7, naming how many points."""
    import ctypes as C
    M, nE = matrix_shape(L, pointwise=True)
    Mt = tail_length(M, reff)
    s = as_matrix(L)
    ctx = s.ctx
    stats = _column_stats(s)
    lsel = ctx.empty((1, nE))
    ctx.call("nh_column_select", s.ptr, M, nE, s.ld, (C.c_int * 1)(Mt), 1, lsel)
    k, n, elpd = ctx.empty((nE,)), ctx.empty((nE,), np.int64), ctx.empty((nE,))
    ctx.call("nh_psis_columns", s.ptr, M, nE, s.ld, Mt, stats, lsel, k, n, elpd)
    k, n, elpd_i = k.get(), n.get(), elpd.get()
    lppd_i = stats.get()[3] - math.log(M)
    high = int(np.sum(k > PARETO_K_WARN))
    if high:
        warnings.warn("the Pareto k of %d of the %d data points is above %.1f: their PSIS-LOO "
                      "estimates are not reliable" % (high, nE, PARETO_K_WARN), UserWarning)
    return dict(elpd_loo=float(elpd_i.sum()), p_loo=float((lppd_i - elpd_i).sum()), se=_se(elpd_i),
                elpd_loo_i=elpd_i, pareto_k=k, n_tail=n, tail_length=Mt, lppd_i=lppd_i,
                n_samples=M, n_data=nE)


# ---------------------------------------------------------------------------------------
# a sampler's (or a read run's) stored spectra
# ---------------------------------------------------------------------------------------
def sampler_spectra(sampler, discard=0, thin=1, modelidx=0):
    """(spectra, data): stored blob ``modelidx`` of every (step, walker) that
    ``get_blobs(discard=discard, thin=thin)`` selects as a ``Quantity`` (M, n_data), rows in its
    flattened order, and the sampler's data table.  A blob that is not a spectrum at the data's
    energies raises the ``TypeError`` of ``plot._process_blob``.  Collective on several ranks, as
    ``get_blobs``."""
    from . import units as u
    wrong = TypeError("Model {0} has wrong blob format".format(modelidx))
    data = getattr(sampler, "data", None)
    if data is None:
        raise ValueError("the sampler has no data table")
    blobs = sampler.get_blobs(discard=discard, thin=thin)
    if blobs is None or not 0 <= modelidx < len(blobs):
        raise wrong
    unit = list(getattr(sampler, "blob_units", None) or [None] * len(blobs))[modelidx]
    b = np.asarray(blobs[modelidx], dtype=float)
    if b.ndim != 3 or b.shape[2] != np.size(data["energy"].value) or unit is None:
        raise wrong
    if b.shape[0] * b.shape[1] == 0:
        raise ValueError("discard = %d leaves no stored step" % discard)
    return u.Quantity(b.reshape(-1, b.shape[2]), unit), data


def sampler_pointwise(sampler, discard=0, thin=1, modelidx=0):
    """The pointwise matrix of stored blob ``modelidx`` of every (step, walker) that
    ``get_blobs(discard=discard, thin=thin)`` selects, rows in its flattened order: uploaded once,
    returned as the device handle.  A blob that is not a spectrum at the data's energies raises
    the ``TypeError`` of ``plot._process_blob``.  Collective on several ranks, as ``get_blobs``."""
    return pointwise_log_likelihood(*sampler_spectra(sampler, discard, thin, modelidx))


class InfoCritMixin:
    """``get_pointwise_log_likelihood``, ``waic`` and ``loo`` of an object with ``get_blobs``,
    ``blob_units`` and ``data`` (EnsembleSampler, read_run's result)"""

    def get_pointwise_log_likelihood(self, discard=0, thin=1, modelidx=0):
        """``infocrit.sampler_pointwise``: the device matrix L[(step, walker)][data point] of the
        stored spectra of blob ``modelidx``"""
        return sampler_pointwise(self, discard, thin, modelidx)

    def waic(self, discard=0, thin=1, modelidx=0):
        """``infocrit.waic`` of ``get_pointwise_log_likelihood(discard, thin, modelidx)``"""
        return waic(sampler_pointwise(self, discard, thin, modelidx))

    def loo(self, discard=0, thin=1, modelidx=0, reff=1.0):
        """``infocrit.loo`` of ``get_pointwise_log_likelihood(discard, thin, modelidx)``"""
        return loo(sampler_pointwise(self, discard, thin, modelidx), reff=reff)
