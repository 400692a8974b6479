"""Reweight a finished fit: what would this posterior be under a slightly different target?

A fit ends with the chain, the log-probabilities and every walker's spectrum at the data's
energies.  Leaving data points out, adding new ones or changing a prior turns the target density
into another one, and the samples already held become a sample of it under the importance weights
``w_s ~ exp(log_ratio_s)``.  ``psis_weights`` turns log-ratios into Pareto-smoothed, self-
normalised log-weights on the GPU (``nh_psis_weights``: the tail rule and the generalised-Pareto
fit of ``infocrit.loo``), together with the diagnostic that says whether they can be trusted:
a ``pareto_k`` above ``infocrit.PARETO_K_WARN`` = 0.7 means refit, do not reweight.
``weighted_stats`` and ``weighted_quantiles`` reduce columns under the weights
(``nh_weighted_moments``, ``nh_weighted_select``); ``resample`` turns the weights back into an
equal-weight sample (``nh_resample_systematic``, ``nh_gather_rows``) that ``posterior.histogram``,
``gaussian_kde``, ``corner`` and ``plot.column_select`` take as it is; ``drop_points`` and
``add_points`` build log-ratios from the pointwise matrix (``nh_row_sums_select``).  There is no
CPU fallback.

Zero weights.  A sample the new target forbids has log-ratio -inf and weight zero; it is left out
of every reduction whatever its value, a NaN included.

Levels.  ``weighted_quantiles`` takes levels q as they are: the value of the first row, in
ascending order, whose running weight reaches q times the total.  ``summary`` and
``Reweighted.bands`` compare with unweighted order statistics, which naima takes at the rank
r = int(q (M - 1)); they ask for the level (r + 0.5) / M, the middle of the mass that rank holds
under equal weights, so that equal weights give exactly the unweighted statistic.

Every ``x`` or ``L`` argument is a host array (uploaded once) or anything ``dview.as_matrix``
takes; rows are in the flattened (step, walker) order of ``get_chain(flat=True)`` and of
``infocrit.sampler_spectra``.  Importing this module creates no GPU context and does not import
matplotlib; argument errors come before any device work.
"""
import ctypes as C
import math
import warnings

import numpy as np

from .dview import as_matrix, matrix_on, matrix_shape
from .infocrit import PARETO_K_WARN, tail_length

__all__ = ["Weights", "Reweighted", "ReweightMixin", "psis_weights", "weighted_stats",
           "weighted_quantiles", "resample", "resample_index", "drop_points", "add_points",
           "summary"]

_MAX_Q = 16  # levels one nh_weighted_select call takes


class Weights:
    """normalised log-weights of K targets: ``lw`` (DeviceMatrix [M][K]) and the host arrays [K]
    ``pareto_k``, ``n_tail`` (int64), ``ess`` (Kish) and ``log_mean_ratio`` (the estimate of
    log(Z_new / Z_old)); ``tail_length`` = Mt, ``n_samples`` = M"""

    def __init__(self, lw, pareto_k, n_tail, ess, log_mean_ratio, tail_length, n_samples):
        self.lw, self.pareto_k, self.n_tail, self.ess = lw, pareto_k, n_tail, ess
        self.log_mean_ratio, self.tail_length, self.n_samples = log_mean_ratio, tail_length, n_samples

    n_targets = property(lambda self: self.lw.ncol)

    def column(self, k=0):
        """(pointer, row stride) of weight column k, as the kernels take one"""
        return self.lw.ptr + 8 * _target(self, k), self.lw.ld


# ---------------------------------------------------------------------------------------
# checks without a device
# ---------------------------------------------------------------------------------------
def _target(weights, k):
    if not isinstance(weights, Weights):
        raise ValueError("weights must be what psis_weights returns")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < weights.lw.ncol:
        raise ValueError("k = %r is not one of the %d targets" % (k, weights.lw.ncol))
    return int(k)


def _samples(x, weights, k):
    """(M, ncol) of ``x``, whose rows must be the weights'"""
    _target(weights, k)
    M, ncol = matrix_shape(x)
    if M != weights.n_samples:
        raise ValueError("%d rows of samples for weights of %d" % (M, weights.n_samples))
    return M, ncol


def _levels(q):
    try:
        q = np.atleast_1d(np.asarray(q, dtype=float))
    except (TypeError, ValueError):
        raise ValueError("q must be numbers in [0, 1]")
    if q.ndim != 1 or q.size == 0 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("q must be one or more numbers in [0, 1]")
    return q


def _rank_levels(q, M):
    """naima's rank r = int(q (M - 1)) of every level and the weighted level (r + 0.5) / M that
    gives order statistic r under equal weights (module docstring)"""
    r = [int(v * (M - 1)) for v in q]
    return r, [(v + 0.5) / M for v in r]


def _groups_of_columns(groups, ncol):
    try:
        groups = [[int(c) for c in np.atleast_1d(np.asarray(g, dtype=np.int64))] for g in groups]
    except (TypeError, ValueError):
        raise ValueError("groups must be a list of lists of column indices")
    if not groups:
        raise ValueError("no group of points")
    for g in groups:
        for c in g:
            if not 0 <= c < ncol:
                raise ValueError("point %d is not one of the %d columns" % (c, ncol))
    return groups


def _count(n, weights, k):
    if n is None:
        e = float(weights.ess[k])
        if not math.isfinite(e):
            raise ValueError("target %d has no weights" % k)
        return max(1, int(round(e)))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n < 2 ** 31:
        raise ValueError("n must be an integer in [1, 2^31)")
    return int(n)


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
def psis_weights(log_ratio, reff=1.0, smooth=True):
    """Pareto-smoothed self-normalised importance weights of ``log_ratio`` [M] or [M][K] (K
    targets at once: every data group left out in turn), as a ``Weights``.  The tail length is
    ``infocrit.tail_length(M, reff)``; ``smooth=False`` gives the plain self-normalised weights
    (``pareto_k`` = +inf).  -inf entries are legal (weight zero).  Warns when a ``pareto_k``
    exceeds 0.7 -- a finite one, or the +inf of a tail of 1 to 4 rows, too few to fit and
    possibly one row carrying all the weight -- but not for the +inf of a target with NO row
    above the cutoff (``n_tail`` = 0): with smoothing, more than the tail length of rows then
    share the largest ratio and no weight can dominate (equal ratios); ``smooth=False`` fits
    nothing and diagnoses nothing.  Raises ``ValueError`` naming the count when a column holds a NaN or +inf, or no finite entry."""
    M, K = matrix_shape(log_ratio)
    if M >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 samples")
    Mt = tail_length(M, reff)
    if not smooth:
        Mt = 0
    s = as_matrix(log_ratio)
    ctx = s.ctx
    lsel = ctx.empty((1, K))
    ctx.call("nh_column_select", s.ptr, M, K, s.ld, (C.c_int * 1)(M - Mt - 1), 1, lsel)
    lw = ctx.empty((M, K))
    pk, nt, ess, lm = ctx.empty((K,)), ctx.empty((K,), np.int64), ctx.empty((K,)), ctx.empty((K,))
    status = ctx.empty((K,), np.int32)
    ctx.call("nh_psis_weights", s.ptr, M, K, s.ld, Mt, lsel, lw, K, pk, nt, ess, lm, status)
    status = status.get()
    if status.any():
        raise ValueError("%d of the %d log-ratios of %d of the %d targets are NaN or +inf, or a "
                         "target has no finite log-ratio: no weights"
                         % (int(status.sum()), M * K, int(np.count_nonzero(status)), K))
    pk, nt = pk.get(), nt.get()
    # (n_tail = 0: k = +inf by rule while more than Mt rows share the largest ratio -- no heavy
    # tail; with 1 to 4 tail rows k = +inf means "could not be fitted", and that is warned of)
    high = int(np.sum((pk > PARETO_K_WARN) & (nt > 0)))
    if high:
        warnings.warn("Some Pareto k diagnostic values are too high: %d of the %d targets are "
                      "above %.1f. Refit, do not reweight" % (high, K, PARETO_K_WARN), UserWarning)
    return Weights(matrix_on(lw, M, K), pk, nt, ess.get(), lm.get(), Mt, M)


def weighted_stats(x, weights, k=0):
    """Per column of ``x`` under weight column ``k``: ``mean``, ``var`` (sum w (x - mean)^2 /
    sum w), ``sd`` and ``n_used``, the number of rows with positive weight (int64)"""
    _samples(x, weights, k)
    s = as_matrix(x)
    out = s.ctx.empty((3, s.ncol))
    ptr, ldw = weights.column(k)
    s.ctx.call("nh_weighted_moments", s.ptr, s.M, s.ncol, s.ld, ptr, ldw, out)
    v = out.get()
    return dict(mean=v[1], var=v[2], sd=np.sqrt(v[2]), n_used=v[0].astype(np.int64))


def weighted_quantiles(x, weights, q, k=0):
    """out[j][c] = the value of column c at which the running weight, rows ascending by (value,
    row index), first reaches q[j] of the total: host array [nq][ncol]"""
    _samples(x, weights, k)
    q = _levels(q)
    s = as_matrix(x)
    ptr, ldw = weights.column(k)
    out = np.empty((len(q), s.ncol))
    for a in range(0, len(q), _MAX_Q):
        qs = q[a:a + _MAX_Q]
        dev = s.ctx.empty((len(qs), s.ncol))
        s.ctx.call("nh_weighted_select", s.ptr, s.M, s.ncol, s.ld, ptr, ldw,
                   (C.c_double * len(qs))(*qs), len(qs), dev)
        out[a:a + len(qs)] = dev.get()
    return out


def _draw(weights, n, seed, k):
    """the device int64 [n] of systematic resampling"""
    ctx = weights.lw.ctx
    u0 = float(np.random.default_rng(seed).random())
    idx = ctx.empty((n,), np.int64)
    ptr, ldw = weights.column(k)
    ctx.call("nh_resample_systematic", ptr, ldw, weights.n_samples, u0, n, idx)
    return idx


def resample_index(weights, n=None, seed=0, k=0):
    """the rows systematic resampling draws (host int64 [n], ascending): row i appears
    floor(n w_i) or ceil(n w_i) times; ``n`` defaults to round(ess[k]), at least 1; the offset is
    ``np.random.default_rng(seed).random()``"""
    k = _target(weights, k)
    return _draw(weights, _count(n, weights, k), seed, k).get()


def resample(x, weights, n=None, seed=0, k=0):
    """an equal-weight sample of ``n`` rows of ``x`` under weight column ``k``, as a
    ``DeviceMatrix`` [n][ncol] (``resample_index`` gives the rows)"""
    _samples(x, weights, k)
    n = _count(n, weights, k)
    s = as_matrix(x)
    idx = _draw(weights, n, seed, k)
    out = s.ctx.empty((n, s.ncol))
    s.ctx.call("nh_gather_rows", s.ptr, s.ld, idx, n, s.ncol, out, s.ncol)
    return matrix_on(out, n, s.ncol)


def _point_sums(L, groups, sign):
    M, ncol = matrix_shape(L, pointwise=True)
    groups = _groups_of_columns(groups, ncol)
    s = as_matrix(L)
    G = len(groups)
    out = s.ctx.empty((M, G))
    for g, cols in enumerate(groups):
        arr = (C.c_int * max(len(cols), 1))(*cols)
        s.ctx.call("nh_row_sums_select", s.ptr, M, ncol, s.ld, arr, len(cols), sign, out.ptr + 8 * g, G)
    return matrix_on(out, M, G)


def drop_points(L, groups):
    """the log-ratios of leaving data points out of the fit: ``DeviceMatrix`` [M][G], column g
    = -sum of the columns ``groups[g]`` of the pointwise matrix ``L``"""
    return _point_sums(L, groups, -1)


def add_points(L, groups):
    """the log-ratios of adding data points to the fit: ``drop_points`` with +"""
    return _point_sums(L, groups, +1)


def summary(x, weights, k=0, labels=None):
    """Per column of ``x``, as a dict of arrays [ncol]: the weighted ``mean``, ``sd``, ``median``,
    ``q16``, ``q84`` and ``n_used``; their unweighted counterparts ``mean_unweighted`` ...
    (``posterior.column_stats``, ``plot.column_select`` at naima's ranks int(q (M - 1)); the
    weighted ones at the matching levels, module docstring); ``shift`` = (mean - mean_unweighted)
    / sd_unweighted; ``labels``"""
    from .plot import column_select
    from .posterior import column_stats
    M, ncol = _samples(x, weights, k)
    if labels is None:
        labels = ["col%d" % i for i in range(ncol)]
    labels = list(labels)
    if len(labels) != ncol:
        raise ValueError("%d labels for %d columns" % (len(labels), ncol))
    s = as_matrix(x)
    ranks, levels = _rank_levels((0.5, 0.16, 0.84), M)
    ws = weighted_stats(s, weights, k)
    wq = weighted_quantiles(s, weights, levels, k)
    us = column_stats(s)
    uq = column_select(s, ranks)
    sd0 = np.sqrt(us["var"])
    with np.errstate(invalid="ignore", divide="ignore"):
        shift = (ws["mean"] - us["mean"]) / sd0
    return dict(labels=labels, mean=ws["mean"], sd=ws["sd"], median=wq[0], q16=wq[1], q84=wq[2],
                n_used=ws["n_used"], mean_unweighted=us["mean"], sd_unweighted=sd0,
                median_unweighted=uq[0], q16_unweighted=uq[1], q84_unweighted=uq[2], shift=shift)


# ---------------------------------------------------------------------------------------
# a sampler's (or a read run's) chain and stored spectra
# ---------------------------------------------------------------------------------------
def _drop_columns(data, drop):
    """the data-point indices of ``drop``: a list of them, or {"group": g}"""
    n = int(np.size(data["energy"].value))
    if isinstance(drop, dict):
        if set(drop) != {"group"}:
            raise ValueError("drop as a dict is {'group': g}")
        from .plot import _groups
        cols = np.flatnonzero(_groups(data) == drop["group"])
        if cols.size == 0:
            raise ValueError("the table has no group %r" % (drop["group"],))
        return [int(c) for c in cols]
    return _groups_of_columns([drop], n)[0]


def _new_data_ratio(sampler, new_data, discard, thin, modelidx):
    """the total log-likelihood of the points of ``new_data`` under every selected sample, the
    model evaluated at their energies in chunks of ``plot._EVAL_BATCH``: DeviceMatrix [M][1]"""
    from . import _lib
    from . import plot as P
    from .datatable import validate_data_table
    from .infocrit import pointwise_log_likelihood
    if getattr(sampler, "modelfn", None) is None:
        raise ValueError("new_data needs the model function, and this sampler has none: pass "
                         "modelfn= to read_run() to evaluate a saved run's model at new energies")
    data = validate_data_table(new_data)
    # (the parameters come from the host chain and go up chunk by chunk inside plot._evaluate, as
    # for the bands of an e_range: not a hot path, the model evaluation dominates)
    pars = np.asarray(sampler.get_chain(flat=True, discard=discard, thin=thin), dtype=float)
    if len(pars) == 0:
        raise ValueError("discard = %d leaves no stored step" % discard)
    ctx = _lib.get_context()
    whole = unit = None
    for a in range(0, len(pars), P._EVAL_BATCH):
        _, un, s = P._evaluate(ctx, sampler, pars[a:a + P._EVAL_BATCH], data, modelidx)
        if whole is None:
            unit = un
            whole = s if s.M == len(pars) else matrix_on(ctx.empty((len(pars), s.ncol)), len(pars),
                                                         s.ncol)
        elif un != unit or s.ncol != whole.ncol:
            raise TypeError("Model {0} has wrong blob format: chunks of samples differ in unit or "
                            "length".format(modelidx))
        if whole is not s:
            ctx.call("nh_copy", whole.rows(a, a + s.M).ptr, s.ptr, 8 * s.M * s.ncol)
        del s
    _, total = pointwise_log_likelihood(whole, data, unit=unit, totals=True)
    return matrix_on(total, len(pars), 1)


class Reweighted:
    """a sampler's posterior under new weights: ``weights`` and the reductions of the flat chain
    and of stored blob ``modelidx`` under them"""

    def __init__(self, sampler, weights, discard=0, thin=1, modelidx=0):
        self.sampler, self.weights = sampler, weights
        self.discard, self.thin, self.modelidx = discard, thin, modelidx
        self._flat = None

    def _chain(self):
        # (get_chain is the one accessor EnsembleSampler and read_run's result share: the flat
        # chain is uploaded once per Reweighted and reused by summary, quantiles and resample)
        if self._flat is None:
            self._flat = as_matrix(np.asarray(
                self.sampler.get_chain(flat=True, discard=self.discard, thin=self.thin), dtype=float))
        return self._flat

    log_evidence_ratio = property(lambda self: float(self.weights.log_mean_ratio[0]),
                                  doc="the estimate of log(Z_new / Z_old)")

    def summary(self):
        """``reweight.summary`` of the flat chain with the sampler's labels"""
        return summary(self._chain(), self.weights, labels=getattr(self.sampler, "labels", None) or None)

    def quantiles(self, q):
        """``weighted_quantiles`` of the flat chain: [nq][ndim]"""
        return weighted_quantiles(self._chain(), self.weights, q)

    def resample(self, n=None, seed=0):
        """the flat chain as an equal-weight ``DeviceMatrix`` of ``n`` rows (default round(ess))"""
        return resample(self._chain(), self.weights, n, seed)

    def bands(self, confs=[3, 1]):
        """(modelx, [(ymin, ymax) per conf]), the shape of ``plot._calc_CI``: the weighted bands
        of stored blob ``modelidx`` at naima's two-sided ranks (module docstring).  Collective on
        several ranks, as ``get_blobs``."""
        from . import units as u
        from .infocrit import sampler_spectra
        from .plot import _band_ranks
        spectra, data = sampler_spectra(self.sampler, self.discard, self.thin, self.modelidx)
        M = spectra.value.shape[0]
        levels = [(r + 0.5) / M for r in _band_ranks(M, confs)]
        vals = weighted_quantiles(spectra.value, self.weights, levels)
        CI = [(u.Quantity(vals[2 * j], spectra.unit), u.Quantity(vals[2 * j + 1], spectra.unit))
              for j in range(len(confs))]
        return data["energy"], CI


class ReweightMixin:
    """``reweight`` and ``influence`` of an object with ``get_chain``, ``get_blobs``,
    ``blob_units``, ``data`` and, for ``new_data=``, ``modelfn`` (EnsembleSampler, read_run's
    result).  Collective on several ranks exactly where ``get_blobs`` is."""

    def reweight(self, log_ratio=None, drop=None, new_data=None, discard=0, thin=1, modelidx=0,
                 reff=1.0, smooth=True):
        """The posterior under another target, as a ``Reweighted``.  Exactly one of: ``drop``, a
        list of data-point indices or ``{"group": g}`` (a value of the table's ``group`` column),
        left out of the fit; ``new_data``, a data table whose points are ADDED to the fit's
        likelihood (the model is evaluated at its energies for every selected sample: needs
        ``modelfn``); ``log_ratio`` [M], the user's own log-ratio of the new target to the old
        for every row of ``get_chain(flat=True, discard=discard, thin=thin)`` (a prior change, a
        tempering)."""
        from .infocrit import sampler_pointwise
        if sum(a is not None for a in (log_ratio, drop, new_data)) != 1:
            raise ValueError("exactly one of log_ratio, drop and new_data must be given")
        tail_length(1, reff)  # (reff checked before any device work)
        if drop is not None:
            if getattr(self, "data", None) is None:
                raise ValueError("the sampler has no data table")
            cols = _drop_columns(self.data, drop)
            lr = drop_points(sampler_pointwise(self, discard, thin, modelidx), [cols])
        elif new_data is not None:
            lr = _new_data_ratio(self, new_data, discard, thin, modelidx)
        else:
            lr = np.asarray(log_ratio, dtype=float)
            M = len(self.get_chain(flat=True, discard=discard, thin=thin))
            if lr.shape != (M,):
                raise ValueError("log_ratio must be one number for each of the %d rows of the "
                                 "flat chain; got shape %s" % (M, lr.shape))
        return Reweighted(self, psis_weights(lr, reff=reff, smooth=smooth), discard, thin, modelidx)

    def influence(self, discard=0, thin=1, modelidx=0, reff=1.0):
        """Every distinct ``group`` of the data table left out in turn, in one ``psis_weights``
        call: a list of dicts ``group``, ``n_points``, ``pareto_k``, ``ess`` and ``shift`` (per
        parameter: the weighted minus the fitted mean over the fitted sd).  A table with one
        group raises ``ValueError``."""
        from .infocrit import sampler_pointwise
        from .plot import _groups
        from .posterior import column_stats
        if getattr(self, "data", None) is None:
            raise ValueError("the sampler has no data table")
        groups = _groups(self.data)
        names = list(np.unique(groups))
        if len(names) < 2:
            raise ValueError("the data table has one group: nothing to leave out")
        tail_length(1, reff)
        cols = [[int(c) for c in np.flatnonzero(groups == g)] for g in names]
        w = psis_weights(drop_points(sampler_pointwise(self, discard, thin, modelidx), cols),
                         reff=reff)
        chain = as_matrix(np.asarray(self.get_chain(flat=True, discard=discard, thin=thin),
                                     dtype=float))
        us = column_stats(chain)
        out = []
        for k, g in enumerate(names):
            ws = weighted_stats(chain, w, k)
            with np.errstate(invalid="ignore", divide="ignore"):
                shift = (ws["mean"] - us["mean"]) / np.sqrt(us["var"])
            out.append(dict(group=g.item() if hasattr(g, "item") else g, n_points=len(cols[k]),
                            pareto_k=float(w.pareto_k[k]), ess=float(w.ess[k]), shift=shift))
        return out
