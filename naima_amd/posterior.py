"""Posterior densities of a chain from GPU reductions, and a corner figure built on them.

The samples are a matrix of M rows and ncol columns in HBM (``get_chain(flat=True)``, the values
of a scalar blob); per column the device returns the moments (``nh_column_moments``), the 1-D
histograms and the 2-D histograms of column pairs (``nh_hist_columns``: NumPy's bin rule on
``np.linspace`` edges, integer counts) and a Gaussian kernel density (``nh_kde_columns``:
``scipy.stats.gaussian_kde`` in one dimension).  All of them are deterministic.  There is no CPU
fallback for the reductions; only the edges, the bandwidths and the contour levels of ``nb * nb``
counts are host arithmetic.

Every function takes a host array ``(M,)`` or ``(M, ncol)``, which is uploaded once per call, or a
device matrix: a ``dview.DeviceMatrix``, or ``(DeviceArray, M, ncol, ld)``; a chain is a host array
``(rows, nwalkers, ndim)``, a ``dview.DeviceChain`` or ``(DeviceArray, rows, nwalkers, ndim)``.

``group_moments`` and ``rhat`` read a chain of several independent ensembles
(``EnsembleSampler(..., ensembles=k)``): per (part of the rows, ensemble, parameter) the device
pools the ensemble's walkers into one sequence and returns its count, mean and variance
(``nh_group_moments``); the Gelman-Rubin formula over those ``m * ndim`` moments is host arithmetic.

``rank_columns``, ``rank_normalize``, ``rhat(method="rank")``, ``ess`` and ``summary`` are the
rank-normalised statistics of Vehtari et al. 2021: every pooled column of a chain is ranked on the
device (``nh_rank_columns``: average ranks from a radix sort), the ranks become normal scores
(``nh_rank_normal_scores``), and the moments and autocorrelation kernels read those exactly as they
read a chain.

``covariance`` is the mean and the unbiased covariance matrix of a chain's pooled rows or of a
matrix (``nh_chain_cov``, two passes), what ``evidence.bridge_sampling`` fits its proposal to.

Importing this module creates no GPU context; argument errors come before any device work.
matplotlib is imported by ``corner`` only.
"""
import ctypes as C

import numpy as np

from ._lib import (NH_EVID_MAX_DIM, NH_HIST_MAX_BINS_1D, NH_HIST_MAX_BINS_2D, NH_HIST_MAX_COLS,
                   NH_HIST_MAX_PAIRS)
from .dview import (DeviceChain, DeviceMatrix, as_chain, as_matrix, chain_dims, matrix_on,
                    matrix_shape)

__all__ = ["column_stats", "histogram", "histogram_pairs", "gaussian_kde", "contour_thresholds",
           "corner", "DEFAULT_LEVELS", "group_moments", "rhat", "rhat_from_moments",
           "rank_columns", "rank_normalize", "ess", "summary", "covariance"]

# the mass of a 2-D Gaussian inside 0.5, 1, 1.5 and 2 sigma (corner's default contours)
DEFAULT_LEVELS = tuple(1.0 - np.exp(-0.5 * np.array([0.5, 1.0, 1.5, 2.0]) ** 2))


# ---------------------------------------------------------------------------------------
# host arithmetic
# ---------------------------------------------------------------------------------------
def _check_bins(bins, with_pairs):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        raise ValueError("bins must be an integer, the same number for every column")
    bins = int(bins)
    if bins < 1:
        raise ValueError("bins must be at least 1")
    cap = NH_HIST_MAX_BINS_2D if with_pairs else NH_HIST_MAX_BINS_1D
    if bins > cap:
        raise ValueError("bins = %d is more than the %d the %s histograms take"
                         % (bins, cap, "pair" if with_pairs else "1-D"))
    return bins


def _check_pairs(pairs, ncol):
    if pairs is None:
        pairs = [(i, j) for i in range(ncol) for j in range(i + 1, ncol)]
    out = []
    for pr in pairs:
        i, j = (int(v) for v in pr)
        if not (0 <= i < ncol and 0 <= j < ncol):
            raise ValueError("pair (%d, %d) is outside the %d columns" % (i, j, ncol))
        out.append((i, j))
    if len(out) > NH_HIST_MAX_PAIRS:
        raise ValueError("%d pairs are more than the %d one call takes"
                         % (len(out), NH_HIST_MAX_PAIRS))
    return out


def _edges(lo, hi, bins):
    """np.histogram's edges for ``range=(lo, hi)`` per column: [ncol][bins+1]; lo == hi widens
    to lo - 0.5, hi + 0.5"""
    lo, hi = np.array(lo, dtype=float, ndmin=1), np.array(hi, dtype=float, ndmin=1)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("the range of a column is not finite (a column without finite values?)")
    if np.any(lo > hi):
        raise ValueError("max must be larger than min in range")
    flat = lo == hi
    lo, hi = np.where(flat, lo - 0.5, lo), np.where(flat, hi + 0.5, hi)
    return np.stack([np.linspace(a, b, bins + 1) for a, b in zip(lo, hi)])


def _range(range, ncol):
    """(lo, hi) arrays [ncol] of an explicit range: one (lo, hi) for every column, or one each"""
    r = np.asarray(range, dtype=float)
    if r.shape == (2,):
        r = np.tile(r, (ncol, 1))
    if r.shape != (ncol, 2):
        raise ValueError("range must be (lo, hi) or one (lo, hi) per column")
    return r[:, 0], r[:, 1]


def _bandwidth_factor(bw_method, n):
    """scipy.stats.gaussian_kde's factor for n samples in one dimension"""
    n = np.asarray(n, dtype=float)
    if bw_method is None or bw_method == "scott":
        return n ** (-1.0 / 5.0)
    if bw_method == "silverman":
        return (n * 3.0 / 4.0) ** (-1.0 / 5.0)
    if np.isscalar(bw_method) and not isinstance(bw_method, str):
        return np.full(n.shape, float(bw_method))
    raise ValueError("bw_method should be 'scott', 'silverman' or a scalar")


def _bandwidths(bw_method, n, var):
    """h [ncol] = factor * sqrt(var); a zero-variance column cannot have a density"""
    var = np.asarray(var, dtype=float)
    if np.any(~(var > 0)):
        raise ValueError("a Gaussian KDE needs a positive variance: column(s) %s have none"
                         % np.flatnonzero(~(var > 0)).tolist())
    h = _bandwidth_factor(bw_method, n) * np.sqrt(var)
    if np.any(~(h > 0) | ~np.isfinite(h)):
        raise ValueError("the bandwidth must be positive and finite")
    return h


def contour_thresholds(H, levels=None):
    """The counts at which the contours enclosing the fractions ``levels`` of a 2-D histogram's
    mass lie, one per level in the levels' order: the counts sorted in descending order, their
    cumulative fraction taken, the threshold of a level is the smallest count still inside that
    fraction (the largest count when not even that one is).  ``corner.hist2d``'s rule."""
    levels = DEFAULT_LEVELS if levels is None else levels
    h = np.sort(np.asarray(H, dtype=float).ravel())[::-1]
    if h.size == 0 or not h[0] > 0:
        raise ValueError("the histogram is empty")
    sm = np.cumsum(h)
    sm /= sm[-1]
    out = np.empty(len(levels))
    for k, v in enumerate(levels):
        inside = h[sm <= v]
        out[k] = inside[-1] if inside.size else h[0]
    return out


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
def column_stats(x):
    """Per column: ``n`` finite values, ``n_nan`` NaNs (int64), and ``min``, ``max``, ``mean``,
    ``var`` (unbiased, ddof=1) of the finite values, as a dict of arrays [ncol]."""
    s = as_matrix(x)
    ctx = s.ctx
    counts, stats = ctx.empty((2, s.ncol), np.int64), ctx.empty((4, s.ncol))
    ctx.call("nh_column_moments", s.ptr, s.M, s.ncol, s.ld, counts, stats)
    c, v = counts.get(), stats.get()
    return dict(n=c[0], n_nan=c[1], min=v[0], max=v[1], mean=v[2], var=v[3])


def _histograms(s, bins, range, pairs):
    """(h1 [ncol][nb], H [npairs][nb][nb], edges [ncol][nb+1]) in one pass over the samples"""
    if s.ncol > NH_HIST_MAX_COLS:
        raise ValueError("%d columns are more than the %d one call takes"
                         % (s.ncol, NH_HIST_MAX_COLS))
    if range is None:
        st = column_stats(s)
        lo, hi = st["min"], st["max"]
    else:
        lo, hi = _range(range, s.ncol)
    edges = _edges(lo, hi, bins)
    ctx = s.ctx
    h1 = ctx.empty((s.ncol, bins), np.int64)
    H = ctx.empty((len(pairs), bins, bins), np.int64) if pairs else None
    flat = (C.c_int * (2 * len(pairs)))(*[v for pr in pairs for v in pr]) if pairs else None
    ctx.call("nh_hist_columns", s.ptr, s.M, s.ncol, s.ld, ctx.array(edges), bins, flat, len(pairs),
             h1, H)
    return h1.get(), (H.get() if pairs else np.zeros((0, bins, bins), np.int64)), edges


def histogram(x, bins=20, range=None):
    """``np.histogram(col, bins, range)`` of every column: (counts int64 [ncol][bins], edges
    [ncol][bins+1]).  ``range`` is (lo, hi) for every column or one per column; None takes each
    column's finite minimum and maximum.  NaN, +-inf and values outside the range are dropped."""
    bins = _check_bins(bins, False)
    if range is not None:
        _range(range, matrix_shape(x)[1])
    h1, _, edges = _histograms(as_matrix(x), bins, range, [])
    return h1, edges


def histogram_pairs(x, bins=20, range=None, pairs=None):
    """``np.histogram2d(col_i, col_j, bins=[edges_i, edges_j])`` of the column pairs ``pairs``
    (default: every i < j): (H int64 [npairs][bins][bins], pairs, edges [ncol][bins+1]), with
    ``H[p][a][b]`` counting the rows in bin a of column i and bin b of column j."""
    bins = _check_bins(bins, True)
    ncol = matrix_shape(x)[1]
    pairs = _check_pairs(pairs, ncol)
    if range is not None:
        _range(range, ncol)
    _, H, edges = _histograms(as_matrix(x), bins, range, pairs)
    return H, pairs, edges


def gaussian_kde(x, points, bw_method=None):
    """``scipy.stats.gaussian_kde(col, bw_method)(points)`` of every column: [ncol][G].
    ``points`` is (G,) for every column or (ncol, G); ``bw_method`` None / "scott", "silverman"
    or a scalar factor; the bandwidth is factor * sqrt(var) over the column's finite values."""
    _bandwidth_factor(bw_method, 2.0)
    s = as_matrix(x)
    p = np.asarray(points, dtype=np.float64)
    if p.ndim == 1:
        p = np.tile(p, (s.ncol, 1))
    if p.ndim != 2 or p.shape[0] != s.ncol or p.shape[1] == 0:
        raise ValueError("points must be (G,) or (ncol, G)")
    st = column_stats(s)
    h = _bandwidths(bw_method, st["n"], st["var"])
    ctx = s.ctx
    out = ctx.empty(p.shape)
    ctx.call("nh_kde_columns", s.ptr, s.M, s.ncol, s.ld, ctx.array(np.ascontiguousarray(p)),
             p.shape[1], ctx.array(h), out)
    return out.get()


# ---------------------------------------------------------------------------------------
# Gelman-Rubin R-hat over independent ensembles
# ---------------------------------------------------------------------------------------
def _chain_shape(x, ensembles, discard, nsplit):
    """(rows, nwalkers, ndim, k, n) of a chain as ``dview.chain_dims`` takes it that holds
    ``ensembles`` = k ensembles of n walkers, checked without a device"""
    if isinstance(ensembles, bool) or not isinstance(ensembles, (int, np.integer)):
        raise ValueError("ensembles must be an integer")
    k = int(ensembles)
    if k < 2:
        raise ValueError("R-hat compares independent ensembles: ensembles must be at least 2")
    rows, nw, ndim = chain_dims(x)
    if nw % k:
        raise ValueError("%d walkers do not split into %d ensembles" % (nw, k))
    if ndim > 256:
        raise ValueError("more than 256 parameters")
    discard = int(discard)
    if discard < 0:
        raise ValueError("discard must not be negative")
    if rows - discard < 2 * nsplit:
        raise ValueError("%d rows behind discard = %d: every sequence needs two at least"
                         % (max(0, rows - discard), discard))
    return rows, nw, ndim, k, nw // k


def group_moments(x, ensembles, discard=0, nsplit=1):
    """The chain ``x`` -- a host array (rows, nwalkers, ndim) as ``get_chain()`` returns it, which
    is uploaded, a ``dview.DeviceChain`` or the block ``(DeviceArray, rows, nwalkers, ndim)`` laid
    out [rows][nwalkers * ndim] -- holds ``ensembles`` = k ensembles, walkers [r n, (r+1) n) being
    ensemble r.  The rows behind ``discard`` are cut into ``nsplit`` equal parts (a remainder is
    dropped from the front); per (part, ensemble, parameter), all walkers of the ensemble pooled:
    ``n`` finite values (int64), their ``mean`` and ``var`` (unbiased), arrays [nsplit][k][ndim],
    and ``draws``, the number of values of each such sequence."""
    nsplit = int(nsplit)
    if nsplit < 1:
        raise ValueError("nsplit must be at least 1")
    _, nw, ndim, k, n = _chain_shape(x, ensembles, discard, nsplit)
    m = as_chain(x, discard).m
    ctx = m.ctx
    nq = nsplit * k * ndim
    counts, stats = ctx.empty((nq,), np.int64), ctx.empty((2, nq))
    ctx.call("nh_group_moments", m.base, m.row0, m.M, nw * ndim, k, n, ndim, nsplit, counts,
             stats)
    c, v = counts.get(), stats.get()
    shape = (nsplit, k, ndim)
    return dict(n=c.reshape(shape), mean=v[0].reshape(shape), var=v[1].reshape(shape),
                draws=m.M // nsplit * n)


def rhat_from_moments(count, mean, var, draws):
    """The BDA3 formula over m sequences of ``draws`` = L values each, given per sequence and
    parameter ([m][ndim]) the number of finite values, their mean and unbiased variance:
    W = the mean of the variances, B/L = the variance (ddof=1) of the means,
    R-hat = sqrt(((L-1)/L W + B/L) / W).  NaN for a parameter of which any sequence is constant
    (variance 0) or holds a non-finite value (fewer than L finite ones)."""
    count, mean, var = np.asarray(count), np.asarray(mean, float), np.asarray(var, float)
    L = float(draws)
    W = var.mean(axis=0)
    BL = mean.var(axis=0, ddof=1)
    bad = np.any(count != draws, axis=0) | np.any(~(var > 0), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(((L - 1.0) / L * W + BL) / W)
    r[bad] = np.nan
    return r


def rhat(x, ensembles, discard=0, split=True, method="moments", folded=True):
    """Gelman-Rubin R-hat per parameter of a chain of ``ensembles`` >= 2 independent ensembles
    (``x`` as ``group_moments`` takes it).  The walkers of ONE ensemble are not independent chains
    -- every proposal is built from another walker of it -- so each ensemble is pooled into one
    sequence; ``split=True`` cuts each into its first and second half (split-R-hat, which also
    sees a drift within the run), giving m = 2 k sequences, else m = k.  Every sequence has
    L = (rows per part) x (walkers of an ensemble) draws; the formula is ``rhat_from_moments``'s.
    Only the m x ndim moments come to the host.

    ``method="rank"`` is the statistic the threshold 1.01 of Vehtari et al. 2021 is defined for:
    the same pooling, ``split`` and formula applied to the rank-normalised scores ``z`` of the
    chain (``rank_normalize``) and, with ``folded=True``, to those of ``|x - median|`` (the median
    over a parameter's pooled values), the larger of the two per parameter.  The first is blind
    to neither heavy tails nor infinite variances, the second sees ensembles that agree in
    location and differ in scale.  NaN for a parameter with a non-finite value.  ``folded`` has no
    meaning for ``method="moments"``."""
    _check_method(method)
    nsplit = 2 if split else 1
    if method == "moments":
        return _rhat_moments(x, ensembles, discard, nsplit)
    k = _chain_shape(x, ensembles, discard, nsplit)[3]
    chain = as_chain(x, discard)
    out = _rhat_moments(_z_chain(chain), k, 0, nsplit)
    if folded:
        out = np.maximum(out, _rhat_moments(_z_chain(_folded(chain)), k, 0, nsplit))
    return out


def _check_method(method):
    if method not in ("moments", "rank"):
        raise ValueError("method must be 'moments' or 'rank', not %r" % (method,))


def _rhat_moments(x, ensembles, discard, nsplit):
    gm = group_moments(x, ensembles, discard, nsplit)
    m = gm["n"].shape[0] * gm["n"].shape[1]
    return rhat_from_moments(gm["n"].reshape(m, -1), gm["mean"].reshape(m, -1),
                             gm["var"].reshape(m, -1), gm["draws"])


def _quantiles(s, q):
    """np.percentile's (linear) quantiles of every column from exact order statistics
    (nh_column_select): [len(q)][ncol]"""
    from .plot import column_select
    pos = np.asarray(q, dtype=float) * (s.M - 1)
    lo = np.floor(pos).astype(int)
    hi = np.minimum(lo + 1, s.M - 1)
    v = column_select(s, list(lo) + list(hi))
    a, b = v[:len(lo)], v[len(lo):]
    return a + (b - a) * (pos - lo)[:, np.newaxis]


# ---------------------------------------------------------------------------------------
# rank-normalised statistics (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021)
# ---------------------------------------------------------------------------------------
def _dims(x, discard, tuple_is_chain=False):
    """the shape of ``x[discard:]``, checked without a device: (rows, nwalkers, ndim) of a chain
    -- a DeviceChain, a 3-D host array, a legacy tuple where the caller reads one as a chain
    (``dview``'s docstring) -- else (M, ncol) of a matrix"""
    if (tuple_is_chain and isinstance(x, tuple)) or isinstance(x, DeviceChain) or \
            not isinstance(x, (tuple, DeviceMatrix)) and len(np.shape(x)) == 3:
        rows, nw, ndim = chain_dims(x, discard, 1)
        return rows - int(discard), nw, ndim
    M, ncol = matrix_shape(x)
    discard = int(discard)
    if discard < 0:
        raise ValueError("discard must not be negative")
    if M - discard < 1:
        raise ValueError("no samples behind discard = %d" % discard)
    return M - discard, ncol


def _view(x, discard, shape):
    """the view of ``x`` behind ``discard`` rows, ``shape`` being what ``_dims`` made of it"""
    if len(shape) == 3:
        return as_chain(x, discard)
    return as_matrix(x).rows(discard, discard + shape[0])


def _like(v, buf):
    """the device array ``buf`` [nrows][nwalkers * ndim] as a view of ``v``'s kind and shape"""
    m = matrix_on(buf, v.nrows, v.nwalkers * v.ndim)
    return DeviceChain(m, v.nwalkers, v.ndim) if isinstance(v, DeviceChain) else m


def _ranks(v):
    """(r [S][ndim], status int32 [ndim]) on the device"""
    ctx = v.ctx
    r, status = ctx.empty((v.S, v.ndim)), ctx.empty((v.ndim,), np.int32)
    ctx.call("nh_rank_columns", *v.pooled(), r, status)
    return r, status


def _z_chain(v):
    """the normal scores of the pooled ranks in the chain's layout, as a view like ``v``"""
    from ._lib import NH_RANK_CHAIN
    ctx, ld = v.ctx, v.nwalkers * v.ndim
    r, _ = _ranks(v)
    z = ctx.empty((v.nrows, ld))
    ctx.call("nh_rank_normal_scores", r, v.nrows, v.nwalkers, v.ndim, NH_RANK_CHAIN, ld, v.ndim, z)
    return _like(v, z)


def _transformed(chain, thr, mode):
    """the chain |x - thr| or x <= thr"""
    ctx, ld = chain.ctx, chain.nwalkers * chain.ndim
    out = ctx.empty((chain.nrows, ld))
    ctx.call("nh_rank_transform", *chain.pooled(),
             ctx.array(np.ascontiguousarray(thr, dtype=float)), mode, out, ld)
    return _like(chain, out)


def _folded(chain):
    """the chain |x - median|, np.median of every parameter's pooled values"""
    from ._lib import NH_RANK_FOLD
    from .plot import column_select
    v = column_select(chain.flat(), [(chain.S - 1) // 2, chain.S // 2])  # (the two middle ones)
    return _transformed(chain, 0.5 * (v[0] + v[1]), NH_RANK_FOLD)


def rank_columns(x, discard=0, device=False):
    """``scipy.stats.rankdata(col, method="average")`` of every column of ``x``, ranked on the GPU
    (``nh_rank_columns``): 1-based ranks, equal values -- a rejected move repeats a walker's value
    -- share the mean of the positions they occupy, -0.0 equals +0.0.  ``x`` is a matrix ``(M,)``
    or ``(M, ncol)`` (host, a ``dview.DeviceMatrix`` or ``(DeviceArray, M, ncol, ld)``), or a chain
    ``(rows, nwalkers, ndim)`` (host, or a ``dview.DeviceChain``), of which every parameter is
    ranked over all walkers and rows (``chain[discard:, :, d].ravel()``); the result has the shape
    of ``x[discard:]``.  A column with a NaN or an infinite value is NaN throughout.
    ``device=True`` returns the device block ``(DeviceArray [M][ncol], M, ncol, ncol)``, a chain's
    M being rows x walkers."""
    shape = _dims(x, discard)
    v = _view(x, discard, shape)
    r, _ = _ranks(v)
    return (r, v.S, v.ndim, v.ndim) if device else r.get().reshape(shape)


def rank_normalize(x, ensembles=1, discard=0, device=False):
    """The rank-normalised scores ``z = ndtri((r - 3/8) / (S + 1/4))`` of ``x``, ``r`` being
    ``rank_columns``' ranks and ``S`` the number of values ranked together (Blom's offsets, as in
    Vehtari et al. 2021).  ``x`` is what ``rank_columns`` takes, except that a tuple is the chain
    ``(DeviceArray, rows, nwalkers, ndim)`` as ``group_moments`` takes it; a chain is ranked over
    all walkers of all ``ensembles`` (which must divide the walkers) and comes back in the chain's
    layout, ``(rows - discard, nwalkers, ndim)`` -- with ``device=True`` as the block
    ``(DeviceArray, rows - discard, nwalkers, ndim)`` that ``group_moments`` takes; a matrix as
    ``(DeviceArray, M, ncol, ncol)``."""
    if isinstance(ensembles, bool) or not isinstance(ensembles, (int, np.integer)) or ensembles < 1:
        raise ValueError("ensembles must be a positive integer")
    shape = _dims(x, discard, True)
    if len(shape) == 3 and shape[1] % int(ensembles):
        raise ValueError("%d walkers do not split into %d ensembles" % (shape[1], int(ensembles)))
    z = _z_chain(_view(x, discard, shape)).owner
    if device:
        return (z,) + tuple(shape) if len(shape) == 3 else (z, shape[0], shape[1], shape[1])
    return z.get().reshape(shape)


def _taus(chain, c):
    """emcee's integrated autocorrelation time of every parameter of a DeviceChain, the
    autocorrelation function averaged over the walkers
    (``autocorr.integrated_time(..., tol=0, quiet=True)``)"""
    from .autocorr import _dimension
    return np.array([_dimension(chain, d, c)[0] for d in range(chain.ndim)], dtype=float)


def _check_kind(kind):
    if kind not in ("bulk", "tail"):
        raise ValueError("kind must be 'bulk' or 'tail', not %r" % (kind,))


def _ess_bulk(chain, c, z=None):
    return chain.S / _taus(_z_chain(chain) if z is None else z, c)


def _ess_tail(chain, c):
    from ._lib import NH_RANK_LE
    q = _quantiles(chain.flat(), [0.05, 0.95])
    tau = [_taus(_transformed(chain, qq, NH_RANK_LE), c) for qq in q]
    return np.minimum(chain.S / tau[0], chain.S / tau[1])


def ess(x, kind="bulk", discard=0, c=5):
    """The effective sample size of each parameter of a chain ``(rows, nwalkers, ndim)`` (host, a
    ``dview.DeviceChain`` or the block ``(DeviceArray, rows, nwalkers, ndim)``): ``S / tau`` with
    ``S = (rows - discard) * nwalkers`` and ``tau`` the integrated autocorrelation time of a
    TRANSFORMED chain -- ``kind="bulk"``: the rank-normalised scores ``rank_normalize`` gives, which
    says how well the centre of the posterior is known whatever its tails; ``kind="tail"``: the
    smaller of the two for the indicator chains ``x <= q05`` and ``x <= q95`` (the quantiles over
    the pooled values), which says how well the 5 % and 95 % quantiles -- and with them credible
    bands -- are known.

    ``tau`` is emcee's estimator as this package computes it everywhere
    (``autocorr.integrated_time(..., c=c, tol=0, quiet=True)``: the autocorrelation function
    averaged over the walkers, Sokal's window), NOT Stan's Geyer-truncated estimator over
    independent chains: the walkers of one ensemble are not independent chains.  A NaN ``tau`` --
    a walker whose transformed series is constant, such as one that never went below ``q05``, a
    non-finite value, a chain of one row -- gives a NaN ESS."""
    _check_kind(kind)
    chain = as_chain(x, discard)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _ess_bulk(chain, c) if kind == "bulk" else _ess_tail(chain, c)


def summary(x, ensembles=1, discard=0, labels=None, c=5):
    """The table of a fit's parameters from GPU reductions over the chain ``x`` (as ``ess`` takes
    it), a dict of arrays [ndim]: ``mean`` and ``sd`` (ddof = 1) of the pooled values, ``median``,
    ``q16`` and ``q84`` (``np.quantile``'s linear rule on exact order statistics), ``ess_bulk``,
    ``ess_tail``, ``tau`` (emcee's, of the values themselves, in rows) and, for ``ensembles`` >= 2,
    ``rhat`` (moments) and ``rhat_rank`` (``rhat(method="rank")``), both split.  ``labels`` (one
    per parameter) are returned under ``"labels"``.  Only arrays of ndim values reach the host."""
    if isinstance(ensembles, bool) or not isinstance(ensembles, (int, np.integer)) or ensembles < 1:
        raise ValueError("ensembles must be a positive integer")
    k = int(ensembles)
    ndim = chain_dims(x, discard, 1)[2]
    if k > 1:
        _chain_shape(x, k, discard, 2)
    if labels is not None and len(labels) != ndim:
        raise ValueError("%d labels for %d parameters" % (len(labels), ndim))
    chain = as_chain(x, discard)
    flat = chain.flat()
    st = column_stats(flat)
    q = _quantiles(flat, [0.16, 0.5, 0.84])
    z = _z_chain(chain)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dict(mean=st["mean"], sd=np.sqrt(st["var"]), median=q[1], q16=q[0], q84=q[2],
                   ess_bulk=_ess_bulk(chain, c, z), ess_tail=_ess_tail(chain, c),
                   tau=_taus(chain, c))
    if k > 1:
        out["rhat"] = _rhat_moments(chain, k, 0, 2)
        out["rhat_rank"] = np.maximum(_rhat_moments(z, k, 0, 2),
                                      _rhat_moments(_z_chain(_folded(chain)), k, 0, 2))
    if labels is not None:
        out["labels"] = list(labels)
    return out


def covariance(x, discard=0):
    """(mean [d], cov [d][d]) of the rows of ``x`` behind ``discard``: ``np.mean(rows, axis=0)``
    and ``np.cov(rows, rowvar=False)`` (unbiased), in two passes on the GPU (``nh_chain_cov``).
    ``x`` is a chain -- host ``(rows, nwalkers, ndim)``, a ``dview.DeviceChain`` or ``(DeviceArray,
    rows, nwalkers, ndim)`` (a 4-tuple is read as a chain, as ``rank_normalize`` reads it) -- of
    which every walker is pooled, or a matrix ``(M,)`` / ``(M, d)`` (host, or a
    ``dview.DeviceMatrix``).  d <= 32.  A column with a NaN or an infinite value is NaN in the
    mean and in its row and column of the covariance; a single row gives a NaN covariance."""
    shape = _dims(x, discard, True)
    if shape[-1] > NH_EVID_MAX_DIM:
        raise ValueError("%d columns are more than the %d a covariance takes"
                         % (shape[-1], NH_EVID_MAX_DIM))
    v = _view(x, discard, shape)
    mean, cov = v.ctx.empty((v.ndim,)), v.ctx.empty((v.ndim, v.ndim))
    v.ctx.call("nh_chain_cov", *v.pooled(), mean, cov)
    return mean.get(), cov.get()


# ---------------------------------------------------------------------------------------
# the figure
# ---------------------------------------------------------------------------------------
def corner(samples, labels=None, truths=None, quantiles=(0.16, 0.5, 0.84), bins=20, range=None,
           levels=None, truth_color=None, fig=None):
    """A corner figure of the samples [M][ncol]: the histogram of every column on the diagonal
    with dashed lines at ``quantiles``, below it the 2-D histogram of every column pair as a
    density image with contours enclosing the fractions ``levels`` of the samples (default: 0.5,
    1, 1.5 and 2 sigma of a 2-D Gaussian).  ``truths`` are drawn as lines and a square marker in
    ``truth_color``.  One pass over the samples on the GPU gives every histogram and one
    selection the quantiles; no panel downloads samples.  Returns the matplotlib figure."""
    bins = _check_bins(bins, True)
    M, n = matrix_shape(samples)
    pairs = _check_pairs(None, n)
    quantiles = [float(v) for v in (quantiles if quantiles is not None else ())]
    if any(not 0.0 <= v <= 1.0 for v in quantiles):
        raise ValueError("quantiles must be in [0, 1]")
    if labels is not None and len(labels) != n:
        raise ValueError("%d labels for %d columns" % (len(labels), n))
    if truths is not None and len(truths) != n:
        raise ValueError("%d truths for %d columns" % (len(truths), n))
    if range is not None:
        _range(range, n)
    import matplotlib.pyplot as plt
    s = as_matrix(samples)
    h1, H, edges = _histograms(s, bins, range, pairs)
    qv = _quantiles(s, quantiles) if quantiles else np.empty((0, n))
    truth_color = "#4682b4" if truth_color is None else truth_color

    if fig is None:
        side = 1.0 + 2.0 * n
        fig = plt.figure(figsize=(side, side))
    if len(fig.axes) == n * n:  # (a figure this function made: drawn over, as corner does)
        axes = np.array(fig.axes).reshape(n, n)
    else:
        axes = fig.subplots(n, n, squeeze=False)
    fig.subplots_adjust(left=0.12, bottom=0.12, right=0.97, top=0.97, wspace=0.05, hspace=0.05)
    which = {pr: k for k, pr in enumerate(pairs)}
    for r in np.arange(n):
        for c in np.arange(n):
            ax = axes[r, c]
            if c > r:
                ax.set_visible(False)
                ax.set_frame_on(False)
                continue
            if r == c:
                ax.stairs(h1[c], edges[c], color="k")
                for v in qv[:, c]:
                    ax.axvline(v, ls="dashed", color="k")
                if truths is not None and truths[c] is not None:
                    ax.axvline(truths[c], color=truth_color)
                ax.set_xlim(edges[c][0], edges[c][-1])
                ax.set_ylim(0, 1.1 * max(h1[c].max(), 1))
                ax.set_yticks([])
            else:
                # column c along x, column r along y: H[p] is [bin of c][bin of r]
                Hp = H[which[(c, r)]]
                ax.pcolormesh(edges[c], edges[r], Hp.T, cmap="Greys", rasterized=True)
                if Hp.max() > 0:
                    lv = np.unique(contour_thresholds(Hp, levels))
                    xc = 0.5 * (edges[c][1:] + edges[c][:-1])
                    yc = 0.5 * (edges[r][1:] + edges[r][:-1])
                    if bins > 1:
                        ax.contour(xc, yc, Hp.T, levels=lv, colors="k")
                if truths is not None:
                    if truths[c] is not None:
                        ax.axvline(truths[c], color=truth_color)
                    if truths[r] is not None:
                        ax.axhline(truths[r], color=truth_color)
                    if truths[c] is not None and truths[r] is not None:
                        ax.plot(truths[c], truths[r], "s", color=truth_color)
                ax.set_xlim(edges[c][0], edges[c][-1])
                ax.set_ylim(edges[r][0], edges[r][-1])
            # labels and tick labels on the outer axes only
            if r < n - 1:
                ax.tick_params(labelbottom=False)
            else:
                ax.tick_params(axis="x", labelrotation=45)
                if labels is not None:
                    ax.set_xlabel(labels[c])
            if c > 0 or r == 0:
                ax.tick_params(labelleft=False)
            elif labels is not None:
                ax.set_ylabel(labels[r])
    return fig
