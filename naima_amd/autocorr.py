"""emcee's ``emcee.autocorr`` surface: the integrated autocorrelation time of a chain, with the
autocorrelation function computed on the GPU.

Per dimension the device returns the walker-averaged normalised autocorrelation function
(``nh_autocorr_prep`` / ``nh_autocorr_lags``: emcee's ``function_1d`` of every walker's series,
averaged over the walkers; direct lag sums, which equal the zero-padded FFT's linear correlation).
The host takes emcee's cumulative sum and window search on it.  Lags are computed in blocks, 256
and then doubling, only until a dimension's window is certain; a dimension with a constant walker
or a non-finite value is NaN (emcee's 0/0) without any lag work.

``RunningAutocorr`` is the same estimate for a chain that is still growing in HBM (a history block
of the device loop): lag sums that grow with the chain (``nh_acf_accumulate`` /
``nh_acf_finalize``), so that a check every few steps of a run costs the new rows only and moves
``n_dim x max_lag`` numbers to the host.  ``converged`` is emcee's stopping rule on two such checks.

Importing this module creates no GPU context; argument errors come before any device work.
"""
import logging

import numpy as np

from .dview import as_chain

__all__ = ["function_1d", "integrated_time", "AutocorrError", "auto_window", "RunningAutocorr",
           "converged"]

logger = logging.getLogger("naima_amd.autocorr")

_FIRST_BLOCK = 256


class AutocorrError(Exception):
    """Raised when the chain is too short to give a reliable autocorrelation time; ``.tau``
    holds the estimate anyway."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super(AutocorrError, self).__init__(*args, **kwargs)


def auto_window(taus, c):
    """emcee's window: the first lag ``m`` with ``m >= c * taus[m]`` (Sokal 1989)"""
    m = np.arange(len(taus)) < c * taus
    if np.any(m):
        return np.argmin(m)
    return len(taus) - 1


def _prep(chain, d):
    """centre dimension d's series of a DeviceChain on the device: (z, s2, ok); ok is False when a
    walker's series is constant or holds a non-finite value (the dimension is NaN then)"""
    ctx, (n_t, n_w, n_d) = chain.ctx, chain.shape
    z, s2 = ctx.empty((n_w, n_t)), ctx.empty((n_w,))
    ctx.call("nh_autocorr_prep", chain.ptr, n_t, n_w, n_d, d, z, s2)
    v = s2.get()
    return z, s2, bool(np.all(np.isfinite(v) & (v > 0)))


def _lags(ctx, z, s2, n_t, n_w, lag0, nlags):
    f = ctx.empty((nlags,))
    ctx.call("nh_autocorr_lags", z, s2, n_t, n_w, lag0, nlags, f)
    return f.get()


def _window_done(taus, c):
    """the window is certain from the lags so far: some lag m > 0 has m >= c * taus[m] while
    lag 0 has 0 < c * taus[0] (then auto_window returns the first such m whatever comes later)"""
    m = np.arange(len(taus)) < c * taus
    return bool(m[0]) and not bool(np.all(m))


def _dimension(chain, d, c):
    """(tau, window, f) of a DeviceChain's dimension d; f holds the lags computed, NaN-filled for
    a NaN dimension"""
    ctx, (n_t, n_w, _) = chain.ctx, chain.shape
    z, s2, ok = _prep(chain, d)
    if not ok:
        return np.nan, n_t - 1, np.full(1, np.nan)
    f = np.empty(0)
    block = _FIRST_BLOCK
    while True:
        nl = min(block, n_t - f.size)
        f = np.concatenate([f, _lags(ctx, z, s2, n_t, n_w, f.size, nl)])
        taus = 2.0 * np.cumsum(f) - 1.0
        if f.size == n_t or _window_done(taus, c):
            w = auto_window(taus, c)
            return taus[w], w, f
        block *= 2


def _as3d(x, has_walkers):
    x = np.atleast_1d(x)
    if len(x.shape) == 1:
        x = x[:, np.newaxis, np.newaxis]
    if len(x.shape) == 2:
        if not has_walkers:
            x = x[:, np.newaxis, :]
        else:
            x = x[:, :, np.newaxis]
    if len(x.shape) != 3:
        raise ValueError("invalid dimensions")
    if x.shape[0] == 0:
        raise ValueError("the chain has no steps")
    if x.shape[1] == 0 or x.shape[2] == 0:
        raise ValueError("the chain has no walkers or no parameters")
    return x


def _integrated(x, c=5, has_walkers=True):
    """(tau [n_d], windows [n_d], [f of each dimension], n_t) without the tolerance check"""
    x = _as3d(x, has_walkers)
    chain = as_chain(x)
    out = [_dimension(chain, d, c) for d in range(x.shape[2])]
    tau = np.array([o[0] for o in out], dtype=float)
    windows = np.array([o[1] for o in out], dtype=int)
    return tau, windows, [o[2] for o in out], x.shape[0]


def function_1d(x):
    """The normalised autocorrelation function of one series, every lag (emcee's
    ``function_1d``); NaN throughout for a constant or non-finite series."""
    x = np.atleast_1d(x)
    if len(x.shape) != 1:
        raise ValueError("invalid dimensions for 1D autocorrelation function")
    n_t = x.shape[0]
    if n_t == 0:
        raise ValueError("the series is empty")
    chain = as_chain(x[:, np.newaxis, np.newaxis])
    z, s2, ok = _prep(chain, 0)
    if not ok:
        return np.full(n_t, np.nan)
    return _lags(chain.ctx, z, s2, n_t, 1, 0, n_t)


def integrated_time(x, c=5, tol=50, quiet=False, has_walkers=True):
    """Estimate the integrated autocorrelation time of a time series (emcee 3's
    ``emcee.autocorr.integrated_time``).

    Args:
        x: the series, ``(n_t, n_walkers, n_dim)`` (``get_chain()``); a 1-D array is one series,
            a 2-D one ``(n_t, n_walkers)``, or ``(n_t, n_dim)`` with ``has_walkers=False``.
        c (float): the step size for the window search (default 5).
        tol (float): the minimum number of autocorrelation times needed to trust the estimate
            (default 50).
        quiet (bool): log a warning instead of raising ``AutocorrError`` when the chain is too
            short.
        has_walkers (bool): whether the second axis of a 2-D ``x`` is the walkers.

    Returns:
        float array ``[n_dim]``: the autocorrelation time of each parameter; NaN for a parameter
        with a constant walker or a non-finite value.

    Raises:
        AutocorrError: if the chain is shorter than ``tol`` times the autocorrelation time of a
            parameter (and ``quiet`` is False).
    """
    tau_est, _, _, n_t = _integrated(x, c, has_walkers)
    flag = tol * tau_est > n_t
    if np.any(flag):
        msg = (
            "The chain is shorter than {0} times the integrated "
            "autocorrelation time for {1} parameter(s). Use this estimate "
            "with caution and run a longer chain!\n"
        ).format(tol, np.sum(flag))
        msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, n_t / tol, tau_est)
        if not quiet:
            raise AutocorrError(tau_est, msg)
        logger.warning(msg)
    return tau_est


def converged(tau, tau_old, n, tol=50, rtol=0.01):
    """The stopping rule of emcee's tutorial ("Autocorrelation analysis & convergence"): the chain
    of ``n`` rows is longer than ``tol`` times every autocorrelation time, and no time has changed
    by more than ``rtol`` since the check before (``tau_old``; ``np.inf`` before the first check,
    which therefore never converges: the relative change is 1 or more).  A NaN time never converges."""
    tau = np.atleast_1d(np.asarray(tau, dtype=float))
    tau_old = np.broadcast_to(np.asarray(tau_old, dtype=float), tau.shape)
    if np.any(np.isnan(tau)) or np.any(np.isnan(tau_old)):
        return False
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.all(tau * tol < n)
        ok &= np.all(np.abs(tau_old - tau) / tau < rtol)
    return bool(ok)


class RunningAutocorr:
    """The integrated autocorrelation time of a chain block that grows in HBM.

    ``update(buffer, n_rows, row_start)`` adds the block's new rows to lag sums kept on the device
    (lags below ``max_lag``); ``tau()`` turns them into the walker-averaged autocorrelation function
    and takes emcee's window search on the host.  What ``update`` is given in several calls or in
    one gives bit-identical results.  If a dimension's window is not certain within the lags kept
    while the chain is longer than that, the number of lags is doubled and the sums are rebuilt
    in one pass over the block (``rebuilds`` counts these); the state takes
    ``8 * n_w * n_d * max_lag`` bytes of HBM, and ``tau`` as much scratch."""

    def __init__(self, n_w, n_d, max_lag=1024, c=5):
        n_w, n_d, max_lag = int(n_w), int(n_d), int(max_lag)
        if n_w < 1 or n_d < 1:
            raise ValueError("the chain has no walkers or no parameters")
        if max_lag < 2:
            raise ValueError("max_lag must be at least 2")
        self.n_w, self.n_d, self.max_lag, self.c = n_w, n_d, max_lag, c
        self.rebuilds = 0
        self._buf = None
        self._state = None   # (pivot, S, stats) on the device
        self.n = self.row_start = 0   # the state holds rows [row_start, n) of _buf

    def _accumulate(self, n0, n1):
        from . import _lib
        ctx = _lib.get_context()
        if self._state is None:
            ld = self.n_w * self.n_d
            self._state = (ctx.empty((ld,)), ctx.empty((ld, self.max_lag)), ctx.empty((3, ld)))
        ctx.call("nh_acf_accumulate", self._buf, self._buf.shape[0], self.n_w, self.n_d,
                 self.row_start, n0, n1, self.max_lag, *self._state)
        self.n = n1

    def update(self, device_buffer, n_rows, row_start=0):
        """the block ``device_buffer`` (a device array ``[rows][n_w * n_d]``) now holds ``n_rows``
        rows, of which those from ``row_start`` on are the chain.  Another block, another
        ``row_start`` or fewer rows than before start the sums again."""
        n_rows, row_start = int(n_rows), int(row_start)
        shape = tuple(device_buffer.shape)
        if len(shape) != 2 or shape[1] != self.n_w * self.n_d:
            raise ValueError("the block is not [rows][n_w * n_d]")
        if not 0 <= row_start <= n_rows <= shape[0]:
            raise ValueError("need 0 <= row_start <= n_rows <= the block's rows")
        same = (self._buf is not None and self._buf.ptr == device_buffer.ptr and
                self._buf.shape == shape and self.row_start == row_start and n_rows >= self.n)
        if not same:
            self._buf, self.row_start, self.n = device_buffer, row_start, row_start
        if n_rows > self.n:
            self._accumulate(self.n, n_rows)

    def _f(self):
        """the walker-averaged normalised autocorrelation function, [n_d][lags kept]"""
        from . import _lib
        ctx = _lib.get_context()
        f = ctx.empty((self.n_d, self.max_lag))
        ctx.call("nh_acf_finalize", self._buf, self._buf.shape[0], self.n_w, self.n_d,
                 self.row_start, self.n, self.max_lag, *self._state, f)
        return f.get()[:, :min(self.max_lag, self.n - self.row_start)]

    def tau(self):
        """(tau [n_d], window [n_d]) of the rows given so far, as ``integrated_time(x, c, tol=0)``
        gives them; NaN for a parameter with a constant walker or a non-finite value"""
        n = self.n - self.row_start
        if self._buf is None or n < 1:
            raise ValueError("the chain has no steps")
        while True:
            f = self._f()
            taus = 2.0 * np.cumsum(f, axis=1) - 1.0
            tau, window = np.full(self.n_d, np.nan), np.full(self.n_d, n - 1, dtype=int)
            more = False
            for d in range(self.n_d):
                if np.isnan(f[d, 0]):
                    continue
                if f.shape[1] < n and not _window_done(taus[d], self.c):
                    more = True
                    break
                window[d] = auto_window(taus[d], self.c)
                tau[d] = taus[d, window[d]]
            if not more:
                self.f = f
                return tau, window
            # the window lies behind the lags kept: twice as many, from the block that is still there
            self.max_lag *= 2
            self.rebuilds += 1
            self._state = None
            self._accumulate(self.row_start, self.n)
