"""Many Nelder-Mead searches at once on the GPU: multi-start maximum likelihood and the profile
likelihood.

A simplex search evaluates four candidate points per iteration, and the device likelihood costs
the same for 4 walkers as for 4000.  Here S independent searches advance in lock-step: the
bookkeeping of all S simplexes lives in HBM (``nh_simplex_*``, csrc/nh_simplex.hip), their 4 S
candidate points are written straight into a ``DPars`` block, the function values are read
straight from the ``DVec`` the likelihood returns, and the host reads 8 bytes per iteration: how
many simplexes are still active and how many asked for a shrink.  One chain of model launches per
iteration serves every search -- the 252 of a profile over 3 parameters x 21 grid values x 4
starts as well as one.

The algorithm of every simplex is naima's prefit (``neldermead.minimize_batched``: relative
``xtol`` / ``ftol``, the same decisions, the same count of function evaluations, status 0
converged / 1 ``maxfev`` / 2 ``maxiter``), bit for bit, on the reduced function of its FREE
coordinates: ``frozen[s, d]`` pins coordinate d of search s at ``values[s, d]``, which is what a
profile likelihood needs.  Two rules are fixed where NumPy leaves them open: a function value
that is NaN counts as +inf, and the sort is stable.  At most ``NH_SIMPLEX_MAX_DIM`` = 64
parameters, the limit of the sampler's own step kernels.

* ``SimplexBatch``        the owner of the device state: ``propose() -> DPars``, ``update(f)``,
                          ``active``, ``result()``
* ``minimize_many``       the loop propose -> fn -> update for any ``fn(DPars) -> DVec``
* ``fit_ml``              multi-start maximum likelihood (or MAP) of a naima model; ``modes``
* ``profile_likelihood``  every grid value of every profiled parameter as ONE batch;
                          ``ProfileResult.interval(cl)`` are the Delta lnL = z^2 / 2 crossings
* ``OptimizeMixin``       ``sampler.fit_ml()`` and ``sampler.profile_likelihood()``

There is no CPU fallback.  Importing this module creates no GPU context; argument errors come
before any device work.  One rank only.
"""
import warnings
from statistics import NormalDist

import numpy as np

from ._lib import NH_SIMPLEX_MAX_DIM

__all__ = ["SimplexBatch", "minimize_many", "fit_ml", "profile_likelihood", "cluster_modes",
           "MLResult", "ProfileResult", "OptimizeMixin"]


# ---------------------------------------------------------------------------------------
# arguments (no device)
# ---------------------------------------------------------------------------------------
def _limit(name, v):
    if v is None:
        return -1
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 31:
        raise ValueError("%s must be a non-negative integer below 2^31 (or None), not %r"
                         % (name, v))
    return int(v)


def _tol(name, v):
    v = float(v)
    if not v >= 0.0:
        raise ValueError("%s must be a non-negative number, not %r" % (name, v))
    return v


def _check_starts(starts, frozen, values):
    """(x0[S, ndim] with the pinned values in place, frozen[S, ndim] bool or None, nmax)"""
    x0 = np.array(starts, dtype=float)
    if x0.ndim == 1:
        x0 = x0[np.newaxis]
    if x0.ndim != 2 or x0.shape[0] < 1 or x0.shape[1] < 1:
        raise ValueError("starts must be (S, ndim) with S, ndim >= 1, not %r" % (x0.shape,))
    S, ndim = x0.shape
    if ndim > NH_SIMPLEX_MAX_DIM:
        raise ValueError("%d parameters are more than the %d the sampler's step kernels and the "
                         "simplex kernels take" % (ndim, NH_SIMPLEX_MAX_DIM))
    if frozen is None:
        if values is not None:
            raise ValueError("values without frozen")
        nmax = ndim
    else:
        frozen = np.asarray(frozen)
        if frozen.ndim == 1:
            frozen = np.broadcast_to(frozen, x0.shape)
        if frozen.shape != x0.shape:
            raise ValueError("frozen must be (S, ndim) = %r, not %r" % (x0.shape, frozen.shape))
        frozen = np.ascontiguousarray(frozen.astype(bool))
        if values is not None:
            values = np.asarray(values, dtype=float)
            if values.ndim == 1:
                values = np.broadcast_to(values, x0.shape)
            if values.shape != x0.shape:
                raise ValueError("values must be (S, ndim) = %r, not %r"
                                 % (x0.shape, values.shape))
            x0 = np.where(frozen, values, x0)
        nfree = (~frozen).sum(axis=1)
        if nfree.min() < 1:
            raise ValueError("simplex %d has every coordinate frozen: nothing to minimise"
                             % int(np.argmin(nfree)))
        nmax = int(nfree.max())
    if not np.all(np.isfinite(x0)):
        raise ValueError("starts (and the values of frozen coordinates) must be finite")
    if S * (nmax + 1) * ndim >= 2 ** 31:
        raise ValueError("S * (n_free + 1) * ndim must stay below 2^31")
    return np.ascontiguousarray(x0), frozen, nmax


def cluster_modes(x, fun, rtol=1e-3):
    """The distinct optima among the end points ``x[S, ndim]`` with values ``fun[S]`` (larger is
    better): taken from the best down, a point joins the first mode whose representative x_m has
    ``max_d |x_d - x_m,d| / max(|x_m,d|, tiny) <= rtol``, else it founds a mode.  Points whose
    ``fun`` is not finite are left out.  Returns a list, best first, of dicts ``x``, ``fun``,
    ``count`` (how many starts reached it) and ``members`` (their indices).  Pure host code."""
    x, fun = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_1d(np.asarray(fun, dtype=float))
    if x.shape[0] != fun.shape[0] or fun.ndim != 1:
        raise ValueError("x must be (S, ndim) and fun (S,), not %r and %r" % (x.shape, fun.shape))
    if not float(rtol) >= 0.0:
        raise ValueError("rtol must be non-negative")
    modes = []
    for i in np.argsort(-fun, kind="stable"):
        if not np.isfinite(fun[i]):
            continue
        for m in modes:
            scale = np.maximum(np.abs(m["x"]), np.finfo(float).tiny)
            if np.max(np.abs(x[i] - m["x"]) / scale) <= rtol:
                m["count"] += 1
                m["members"].append(int(i))
                break
        else:
            modes.append(dict(x=x[i].copy(), fun=float(fun[i]), count=1, members=[int(i)]))
    return modes


def _parabola(xs, ys):
    """coefficients (a, b, c) of a u^2 + b u + c through three points, u = x - xs[1]"""
    u0, u2 = xs[0] - xs[1], xs[2] - xs[1]
    d0, d2 = (ys[0] - ys[1]) / u0, (ys[2] - ys[1]) / u2
    a = (d2 - d0) / (u2 - u0)
    return a, d0 - a * u0, ys[1]


def _crossing(grid, lnl, i, level):
    """where the profile crosses ``level`` between grid[i] and grid[i + 1] (one of the two values
    is below it, the other is not): the root in that cell of the parabola through the three grid
    points nearest to the crossing; the chord where those are not all finite or have no such root"""
    x0, x1, y0, y1 = grid[i], grid[i + 1], lnl[i], lnl[i + 1]
    if not (np.isfinite(y0) and np.isfinite(y1)):
        return float(x0 if np.isfinite(y0) else x1)  # the last grid point the prior allows
    lin = x0 + (level - y0) * (x1 - x0) / (y1 - y0)
    left, right = i - 1, i + 2
    trips = []
    if left >= 0:
        trips.append((abs(lin - grid[left]), left))
    if right < len(grid):
        trips.append((abs(lin - grid[right]), i))
    for _, j in sorted(trips):
        xs, ys = grid[j:j + 3], lnl[j:j + 3]
        if not np.all(np.isfinite(ys)):
            continue
        a, b, c = _parabola(xs, ys)
        if a == 0.0:
            break
        disc = b * b - 4.0 * a * (c - level)
        if disc < 0.0:
            continue
        q = -0.5 * (b + np.copysign(np.sqrt(disc), b))  # (the stable form of the two roots)
        roots = [q / a + xs[1]] + ([(c - level) / q + xs[1]] if q != 0.0 else [])
        pad = 1e-9 * (x1 - x0)
        ok = [r for r in roots if x0 - pad <= r <= x1 + pad]
        if ok:
            return float(min(ok, key=lambda r: abs(r - lin)))
    return float(lin)


class MLResult:
    """``fit_ml``'s result.  ``x`` the best point and ``fun`` its log-probability (the MAXIMISED
    function: the log-likelihood under the flat prior, the log-posterior with a prior);
    ``success`` whether that search converged; ``ends[S, ndim]``, ``ends_fun[S]``, ``status[S]``,
    ``nfev[S]``, ``nit[S]`` every search's end point; ``starts[S, ndim]``; ``modes``
    (``cluster_modes`` of the end points: one entry per distinct optimum, best first)."""

    def __init__(self, starts, res, mode_rtol):
        self.starts = starts
        self.ends, self.ends_fun = res["x"], -res["fun"]
        self.status, self.nfev, self.nit = res["status"], res["nfev"], res["nit"]
        self.iterations = res.get("iterations")
        fun = np.where(np.isnan(self.ends_fun), -np.inf, self.ends_fun)
        best = int(np.argmax(fun))
        self.x, self.fun = self.ends[best].copy(), float(self.ends_fun[best])
        self.success = bool(self.status[best] == 0)
        self.modes = cluster_modes(self.ends, self.ends_fun, mode_rtol)

    def __repr__(self):
        return "MLResult(fun=%r, x=%r, modes=%d, starts=%d)" % (self.fun, self.x, len(self.modes),
                                                                 len(self.ends))


class ProfileResult:
    """The profile likelihood of one parameter.  ``par`` its index and ``label``; ``grid[G]`` the
    pinned values, ascending, the ML value among them; ``lnl[G]`` the log-probability maximised
    over the other parameters (the best over the starts of a grid point); ``pars[G, ndim]`` where
    that maximum lies; ``status[G]`` of the winning search (0 converged, 1 maxfev, 2 maxiter);
    ``ml`` the point the profile is taken round (``x``, ``fun``)."""

    def __init__(self, par, label, grid, lnl, pars, status, ml):
        self.par, self.label, self.grid, self.lnl = par, label, grid, lnl
        self.pars, self.status, self.ml = pars, status, ml

    @property
    def lnl_max(self):
        """the top of the profile: the vertex of the parabola through the best grid point and its
        two neighbours (exact for a quadratic profile; the grid value itself at an end of the grid
        or beside a non-finite value), or ``ml.fun`` where that is larger"""
        lnl = np.where(np.isnan(self.lnl), -np.inf, self.lnl)
        k = int(np.argmax(lnl))
        top = float(lnl[k])
        if 0 < k < len(lnl) - 1 and np.all(np.isfinite(lnl[k - 1:k + 2])):
            a, b, c = _parabola(self.grid[k - 1:k + 2], lnl[k - 1:k + 2])
            if a < 0.0:
                top = max(top, float(c - b * b / (4.0 * a)))
        return max(top, float(self.ml.fun)) if np.isfinite(self.ml.fun) else top

    @property
    def delta_chi2(self):
        """``2 (lnl_max - lnl)`` on the grid: the likelihood-ratio statistic, which Wilks' theorem
        gives a chi-squared distribution with one degree of freedom -- 1 and 4 are the 1 sigma
        and 2 sigma levels"""
        return 2.0 * (self.lnl_max - self.lnl)

    def interval(self, cl=0.683):
        """(lo, hi): the two crossings of ``lnl = lnl_max - z^2 / 2`` nearest to the top of the
        profile, ``z = Phi^-1((1 + cl) / 2)``, each located by the parabola through the three grid
        points nearest to it (exact for a quadratic profile).  A side the grid does not bracket is
        ``nan``, with a warning."""
        cl = float(cl)
        if not 0.0 < cl < 1.0:
            raise ValueError("cl must lie in (0, 1), not %r" % cl)
        z = NormalDist().inv_cdf(0.5 * (1.0 + cl))
        level = self.lnl_max - 0.5 * z * z
        lnl = np.where(np.isnan(self.lnl), -np.inf, self.lnl)
        k = int(np.argmax(lnl))
        lo = hi = float("nan")
        for i in range(k - 1, -1, -1):
            if lnl[i] < level:
                lo = _crossing(self.grid, lnl, i, level)
                break
        for i in range(k, len(lnl) - 1):
            if lnl[i + 1] < level:
                hi = _crossing(self.grid, lnl, i, level)
                break
        for side, v in (("lower", lo), ("upper", hi)):
            if np.isnan(v):
                warnings.warn("the grid of %s does not bracket the %s %g%% crossing: widen span "
                              "or pass a grid" % (self.label, side, 100 * cl))
        return lo, hi

    def __repr__(self):
        return "ProfileResult(%s, G=%d, lnl_max=%r)" % (self.label, len(self.grid), self.lnl_max)


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
class SimplexBatch:
    """S simplexes in HBM (module docstring).  ``starts[S, ndim]``; ``frozen[S, ndim]`` marks the
    coordinates of each search that stay at ``values[S, ndim]`` (at their start where ``values``
    is None); ``maxiter`` / ``maxfev`` default to 200 n_free of each search.  ``logp=True``: the
    function handed to ``update`` is a log-probability to MAXIMISE (the kernels negate it).

    ``propose()`` returns the ``DPars`` block that wants evaluating next -- the initial points
    first, then the 4 S candidates of an iteration (kind c of simplex s in column c S + s), or the
    points of a shrink in the iterations where a simplex asked for one -- and ``update(f)`` takes
    the values of exactly that block, a ``DVec`` or a ``DeviceArray`` of one value per column.
    ``active`` is the number of searches still running; ``result()`` may be called at any time."""

    def __init__(self, ctx, starts, frozen=None, values=None, xtol=1e-4, ftol=1e-4, maxiter=None,
                 maxfev=None, logp=False):
        x0, frozen, nmax = _check_starts(starts, frozen, values)
        self.xtol, self.ftol = _tol("xtol", xtol), _tol("ftol", ftol)
        maxiter, maxfev = _limit("maxiter", maxiter), _limit("maxfev", maxfev)
        from . import _lib
        _lib.load()
        self.ctx, self.logp = ctx, int(bool(logp))
        self.S, self.ndim, self.nmax = x0.shape[0], x0.shape[1], nmax
        self.dims = (self.S, self.ndim, self.nmax)
        nbytes = int(_lib._lib.nh_simplex_bytes(*self.dims))
        if nbytes <= 0:
            raise ValueError("sizes out of range for the simplex kernels: %r" % (self.dims,))
        self.state = ctx.empty((nbytes // 8,))
        self._x0 = ctx.array(x0)
        self._frozen = None if frozen is None else ctx.array(frozen.astype(np.int32), dtype=np.int32)
        self._limits = (maxiter, maxfev)
        self._phase, self._q, self._cols = "init", None, 0
        self.active, self.nshrink, self.iterations = self.S, 0, 0

    def propose(self):
        from .darray import DPars
        ctx, S = self.ctx, self.S
        if self._q is not None:
            raise RuntimeError("propose() twice without update()")
        if self._phase == "init":
            n = (self.nmax + 1) * S
            q = ctx.empty((self.ndim, n))
            ctx.call("nh_simplex_init_points", self.state, *self.dims, self._x0, self._frozen,
                     self._x0 if self._frozen is not None else None, *self._limits, q)
        elif self._phase == "shrink":
            n = self.nmax * self.nshrink
            q = ctx.empty((self.ndim, n))
            ctx.call("nh_simplex_shrink_points", self.state, *self.dims, self.nshrink, q)
        else:
            n = 4 * S
            q = ctx.empty((self.ndim, n))
            ctx.call("nh_simplex_propose", self.state, *self.dims, q)
        self._q, self._cols = q, n
        return DPars(ctx, q, self.ndim, n)

    def _column(self, f):
        """(owner, pointer, stride) of the function values, one per proposed column"""
        from .darray import DVec
        if isinstance(f, DVec):
            if not (f.tf == 0 and f.a == 1.0 and f.b == 1.0 and f.c == 0.0):
                f = f.dense()
            n, own, ptr, stride = f.n, f, f.ptr, f.stride
        elif hasattr(f, "ptr") and getattr(f, "dtype", None) in (np.float64, float):
            n, own, ptr, stride = f.size, f, f.ptr, 1
        else:
            raise TypeError("update() takes a DVec or a float64 DeviceArray, not %s"
                            % type(f).__name__)
        if n != self._cols:
            raise ValueError("%d function values for %d proposed columns" % (n, self._cols))
        return own, ptr, stride

    def update(self, f):
        import ctypes as C

        from . import _lib
        if self._q is None:
            raise RuntimeError("update() without propose()")
        own, ptr, stride = self._column(f)
        ctx, tail = self.ctx, (ptr, stride, self.logp, self.xtol, self.ftol)
        if self._phase == "init":
            ctx.call("nh_simplex_adopt", self.state, *self.dims, *tail)
        elif self._phase == "shrink":
            ctx.call("nh_simplex_shrink_adopt", self.state, *self.dims, self.nshrink, *tail)
        else:
            ctx.call("nh_simplex_update", self.state, *self.dims, self._q, *tail)
        counts = (C.c_int * 2)()
        _lib._chk(_lib._lib.nh_simplex_counts(ctx.h, self.state.ptr, *self.dims, counts))
        del own
        self.iterations += self._phase == "iter"
        self.active, self.nshrink = int(counts[0]), int(counts[1])
        self._phase = "shrink" if self.nshrink else "iter"
        self._q = None

    def result(self):
        """dict of ``x[S, ndim]``, ``fun[S]`` (of the MINIMISED function: minus the
        log-probability under ``logp=True``), ``nfev``, ``nit``, ``status`` (-1: still running)
        and ``success``"""
        ctx, S = self.ctx, self.S
        x, fun = ctx.empty((S, self.ndim)), ctx.empty((S,))
        ints = ctx.empty((4, S), dtype=np.int32)
        ctx.call("nh_simplex_result", self.state, *self.dims, x, fun, ints)
        iv = ints.get()
        return dict(x=x.get(), fun=fun.get(), nfev=iv[0].astype(np.int64),
                    nit=iv[1].astype(np.int64), status=iv[2].astype(np.int64),
                    success=iv[2] == 0)


def minimize_many(fn, starts, frozen=None, values=None, xtol=1e-4, ftol=1e-4, maxiter=None,
                  maxfev=None, batch=4096, logp=True, ctx=None):
    """S Nelder-Mead searches in lock-step.  ``fn(DPars) -> DVec`` (or a float64 DeviceArray) maps
    a block of n parameter columns to n values: a log-probability to maximise (``logp=True``), or
    a function to minimise.  The loop is propose -> fn -> update -> an 8-byte download; a shrink
    launch pair runs only in iterations where a simplex asked for one.  More than ``batch // 4``
    searches run as consecutive groups of that many; every search's result is independent of the
    grouping and of the searches beside it, bit for bit, when ``fn``'s value of a column does not
    depend on the other columns.  Returns ``SimplexBatch.result()``'s dict for all S, plus
    ``iterations``, the loop iterations of each group."""
    x0, frozen, _ = _check_starts(starts, frozen, values)
    if isinstance(batch, bool) or int(batch) != batch or int(batch) < 4:
        raise ValueError("batch must be an integer >= 4, not %r" % (batch,))
    if not callable(fn):
        raise ValueError("fn must be callable")
    if ctx is None:
        from ._lib import get_context
        ctx = get_context()
    per = int(batch) // 4
    parts, its = [], []
    for a in range(0, len(x0), per):
        sb = SimplexBatch(ctx, x0[a:a + per], None if frozen is None else frozen[a:a + per],
                          None, xtol, ftol, maxiter, maxfev, logp=logp)
        sb.update(fn(sb.propose()))
        while sb.active:
            sb.update(fn(sb.propose()))
        parts.append(sb.result())
        its.append(sb.iterations)
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["iterations"] = its
    return out


def _device_lnprob(data, model, prior):
    """``fn(DPars) -> DVec`` of core.lnprob"""
    from .core import lnprob
    from .darray import DVec

    def fn(P):
        out = lnprob(P, data, model, prior)[0]
        if not isinstance(out, DVec):
            raise TypeError("the model's log-probability did not stay on the device")
        return out

    return fn


def _probe(fn, ctx, x):
    """one evaluation of at most two columns: a model that cannot run on device parameters
    raises its reason here, before any simplex exists"""
    from .darray import DPars
    c = np.ascontiguousarray(np.atleast_2d(x)[:2].T, dtype=float)
    try:
        fn(DPars(ctx, ctx.array(c), c.shape[0], c.shape[1]))
    finally:
        ctx.flush()


def _one_rank(what):
    import os
    if os.environ.get("NAIMA_AMD_FORCE_SHARDED", "0") == "1":
        raise NotImplementedError("%s with walkers sharded over several ranks" % what)


def fit_ml(data, model, prior=None, starts=None, xtol=1e-4, ftol=1e-4, maxiter=None, maxfev=None,
           batch=4096, mode_rtol=1e-3):
    """Multi-start maximum likelihood of ``model`` on the (validated) data table: one Nelder-Mead
    search from every row of ``starts[S, ndim]``, all in lock-step through ``core.lnprob`` on
    device parameters.  ``prior=None`` is the flat prior of naima's prefit; a prior function gives
    the MAP instead, and a region it forbids counts as +inf.  Returns an ``MLResult``.  A model
    that cannot run on device parameters raises what it raises there (``NotImplementedError``
    for a grid or table shaped per walker, ``TypeError`` / ``ValueError`` for plain numpy
    arithmetic on the parameters)."""
    if starts is None:
        raise ValueError("fit_ml needs starts[S, ndim]")
    x0, _, _ = _check_starts(starts, None, None)
    _one_rank("fit_ml")
    from ._lib import get_context
    ctx = get_context()
    fn = _device_lnprob(data, model, prior)
    _probe(fn, ctx, x0)
    res = minimize_many(fn, x0, None, None, xtol, ftol, maxiter, maxfev, batch, True, ctx)
    return MLResult(x0, res, mode_rtol)


def _par_indices(par, ndim, labels):
    pars = list(par) if isinstance(par, (list, tuple)) else [par]
    if not pars:
        raise ValueError("no parameter to profile")
    out = []
    for p in pars:
        if isinstance(p, str):
            if labels is None or p not in list(labels):
                raise ValueError("no parameter is labelled %r" % p)
            p = list(labels).index(p)
        if isinstance(p, bool) or int(p) != p or not -ndim <= int(p) < ndim:
            raise ValueError("parameter %r is outside the %d parameters" % (p, ndim))
        out.append(int(p) % ndim)
    return out, isinstance(par, (list, tuple))


def profile_likelihood(data, model, par, grid=None, n=21, span=4.0, ml=None, starts_per_point=1,
                       freeze_others=False, prior=None, p0=None, sd=None, labels=None,
                       spread=0.05, seed=0, xtol=1e-4, ftol=1e-4, maxiter=None, maxfev=None,
                       batch=4096):
    """The profile likelihood of parameter ``par`` (an index, a label of ``labels``, or a list of
    those: all of them in the same batch): at every grid value the log-probability maximised over
    the other parameters -- one simplex with ``par`` frozen there, ``starts_per_point`` of them
    where asked (the first from the ML point's other coordinates, the rest from a Gaussian ball of
    relative width ``spread`` round them, ``np.random.default_rng(seed)``) -- all run as ONE
    ``minimize_many``.  ``ml`` is an ``MLResult`` or a parameter vector (default: ``fit_ml`` from
    ``p0``).  ``grid`` defaults to ``n`` values over ``ml[par] +- span * sd``, ``sd`` (a number,
    or one per parameter) defaulting to a tenth of ``|ml[par]|``; a list of parameters takes a
    list of grids.  The ML value itself is always made a grid point.  ``freeze_others=True`` pins
    every other parameter at its ML value: the grid is then only evaluated, in one launch chain.
    ``prior`` as in ``fit_ml``.  Returns a ``ProfileResult`` (a list of them for a list)."""
    _one_rank("profile_likelihood")
    if ml is None and p0 is None:
        raise ValueError("profile_likelihood needs ml (a fit_ml result or a point) or p0")
    k = int(starts_per_point)
    if k != starts_per_point or k < 1:
        raise ValueError("starts_per_point must be a positive integer")
    n, span = int(n), float(span)
    if n < 3 or not span > 0.0:
        raise ValueError("n must be at least 3 and span positive")
    from ._lib import get_context
    ctx = get_context()
    if ml is None:
        ml = fit_ml(data, model, prior, np.atleast_2d(np.asarray(p0, dtype=float)), xtol, ftol,
                    maxiter, maxfev, batch)
    mlx = np.asarray(ml.x if hasattr(ml, "x") else ml, dtype=float).ravel()
    ndim = mlx.size
    idx, many = _par_indices(par, ndim, labels)
    if ndim < 2 and not freeze_others:
        raise ValueError("a one-parameter model has nothing to maximise over: freeze_others=True")
    fn = _device_lnprob(data, model, prior)
    _probe(fn, ctx, mlx)
    if not hasattr(ml, "fun"):
        from .darray import DPars
        v = fn(DPars(ctx, ctx.array(mlx[:, None]), ndim, 1)).get()
        ml = _Point(mlx, float(v[0]))
    sds = np.broadcast_to(0.1 * np.abs(mlx) if sd is None else np.asarray(sd, dtype=float), (ndim,))
    grids = grid if many else [grid]
    if grid is None:
        grids = [None] * len(idx)
    if len(grids) != len(idx):
        raise ValueError("%d grids for %d parameters" % (len(grids), len(idx)))
    built = []
    for p, g in zip(idx, grids):
        if g is None:
            w = sds[p] if sds[p] > 0 and np.isfinite(sds[p]) else 0.1
            g = mlx[p] + span * w * np.linspace(-1.0, 1.0, n)
        g = np.asarray(g, dtype=float).ravel()
        if not np.all(np.isfinite(g)) or g.size < 2:
            raise ValueError("a grid needs two finite values at least")
        built.append(np.unique(np.append(g, mlx[p])))
    # every (parameter, grid value, start) is one column
    rng = np.random.default_rng(seed)
    starts, frozen = [], []
    for p, g in zip(idx, built):
        for v in g:
            for j in range(k):
                x = mlx.copy() if j == 0 else mlx + spread * mlx * rng.normal(size=ndim)
                x[p] = v
                f = np.ones(ndim, dtype=bool) if freeze_others else np.zeros(ndim, dtype=bool)
                f[p] = True
                starts.append(x)
                frozen.append(f)
    starts, frozen = np.array(starts), np.array(frozen)
    if freeze_others:
        from .darray import DPars
        ends, fun = starts[::k], np.empty(len(starts) // k)
        per = int(batch)
        for a in range(0, len(ends), per):
            c = np.ascontiguousarray(ends[a:a + per].T)
            fun[a:a + per] = fn(DPars(ctx, ctx.array(c), ndim, c.shape[1])).get()
        status = np.zeros(len(ends), dtype=np.int64)
    else:
        res = minimize_many(fn, starts, frozen, None, xtol, ftol, maxiter, maxfev, batch, True, ctx)
        lnl = np.where(np.isnan(res["fun"]), -np.inf, -res["fun"]).reshape(-1, k)
        best = np.argmax(lnl, axis=1)
        rows = np.arange(len(best)) * k + best
        ends, fun, status = res["x"][rows], -res["fun"][rows], res["status"][rows]
    out, a = [], 0
    for p, g in zip(idx, built):
        sl = slice(a, a + len(g))
        a += len(g)
        out.append(ProfileResult(p, labels[p] if labels is not None else "par%d" % p, g, fun[sl],
                                 ends[sl], status[sl], ml))
    return out if many else out[0]


class _Point:
    def __init__(self, x, fun):
        self.x, self.fun = x, fun


# ---------------------------------------------------------------------------------------
# a sampler
# ---------------------------------------------------------------------------------------
class OptimizeMixin:
    """``fit_ml`` and ``profile_likelihood`` of an EnsembleSampler made by ``get_sampler``"""

    def _optimize_args(self, what, prior):
        if self.comm.size > 1:
            raise NotImplementedError("%s with walkers sharded over several ranks" % what)
        _one_rank(what)
        if not self.naima_style or len(self.args) != 3:
            raise ValueError("%s needs a sampler of naima's lnprob(pars, data, model, prior)" % what)
        data, model, pr = self.args
        return data, model, (pr if prior else None)

    def fit_ml(self, n_starts=16, spread=0.1, seed=None, from_chain=True, prior=False, **kw):
        """Multi-start maximum likelihood (``optimize.fit_ml``) of the sampler's model and data.
        The starts are the ``n_starts`` most probable DISTINCT samples of the stored chain
        (``from_chain=True`` and a chain to take them from), else a Gaussian ball of relative
        width ``spread`` round the sampler's ``p0`` -- its first point p0 itself -- drawn from
        ``np.random.default_rng(seed)``.  ``prior=False`` fits under the flat prior (maximum
        likelihood, as naima's prefit); ``prior=True`` under the sampler's prior (the MAP).
        ``kw``: ``xtol``, ``ftol``, ``maxiter``, ``maxfev``, ``batch``, ``mode_rtol``."""
        data, model, pr = self._optimize_args("fit_ml", prior)
        n_starts = int(n_starts)
        if n_starts < 1:
            raise ValueError("n_starts must be positive")
        starts = None
        if from_chain:
            try:
                chain = np.asarray(self.get_chain())
                lp = np.asarray(self.get_log_prob())
            except Exception:
                chain = None
            if chain is not None and chain.size:
                flat, lpf = chain.reshape(-1, chain.shape[-1]), lp.reshape(-1)
                order = np.argsort(-np.where(np.isnan(lpf), -np.inf, lpf), kind="stable")
                _, first = np.unique(flat[order], axis=0, return_index=True)
                starts = flat[order][np.sort(first)[:n_starts]]
        if starts is None:
            p0 = np.asarray(getattr(self, "run_info", {}).get("p0"), dtype=float)
            if p0.ndim == 0:
                raise ValueError("no chain and no p0 to start from")
            p0 = np.atleast_2d(p0)[0]
            rng = np.random.default_rng(seed)
            starts = p0 + spread * p0 * rng.normal(size=(n_starts, p0.size))
            starts[0] = p0
        return fit_ml(data, model, pr, starts, **kw)

    def profile_likelihood(self, par, ml=None, prior=False, **kw):
        """``optimize.profile_likelihood`` of the sampler's model and data round ``ml`` (default:
        ``self.fit_ml(prior=prior)``); ``par`` may be a label of the sampler.  The default grid's
        ``sd`` is the standard deviation of the stored chain where there is one."""
        data, model, pr = self._optimize_args("profile_likelihood", prior)
        if ml is None:
            ml = self.fit_ml(prior=prior)
        if "sd" not in kw:
            try:
                chain = np.asarray(self.get_chain())
                if chain.size and chain.shape[0] * chain.shape[1] > 1:
                    kw["sd"] = chain.reshape(-1, chain.shape[-1]).std(axis=0)
            except Exception:
                pass
        kw.setdefault("labels", getattr(self, "labels", None))
        return profile_likelihood(data, model, par, ml=ml, prior=pr, **kw)
