"""Typed views of samples that lie in HBM, and the one place where their shapes are checked.

``DeviceMatrix`` is a row-major matrix [M][ncol] with row stride ``ld``; ``DeviceChain`` is a chain
[rows][nwalkers * ndim], with its log-probabilities [rows][nwalkers] where they travel with it.
Both are views: ``owner`` keeps the buffer alive, ``row0`` is the view's first row in it, and
``rows(a, b)`` / ``behind(discard)`` give sub-views or raise ``ValueError``.  The analysis modules
reach their data through ``as_matrix`` and ``as_chain``, which take a typed view, a host array
(uploaded once) or a legacy tuple; ``matrix_shape`` and ``chain_dims`` are the same checks without
a device, so that argument errors come before any device work.

A typed view is never reinterpreted: ``posterior.rank_columns`` ranks a ``DeviceChain`` as it
ranks the host chain (rows, nwalkers, ndim); to ``rank_normalize`` and ``covariance`` a
``DeviceMatrix`` is a matrix.  For compatibility two 4-tuples remain accepted, and each function
reads one the way it always has:

* ``(DeviceArray, M, ncol, ld)``, a matrix: ``posterior.column_stats``, ``histogram``,
  ``histogram_pairs``, ``gaussian_kde``, ``rank_columns`` and ``corner``, and every function of
  ``infocrit`` and ``predictive``;
* ``(DeviceArray, rows, nwalkers, ndim)``, a chain laid out [rows][nwalkers * ndim]:
  ``posterior.group_moments``, ``rhat``, ``ess``, ``summary``, ``rank_normalize`` and
  ``covariance``, and ``evidence.bridge_sampling``.  (Importing this module creates no GPU context.)
"""
import numpy as np

__all__ = ["DeviceMatrix", "DeviceChain", "matrix_on", "matrix_shape", "chain_dims", "as_matrix",
           "as_chain"]


class DeviceMatrix:
    """rows [row0, row0 + M) of the row-major float64 matrix at ``base``: ``ncol`` columns, row
    stride ``ld``; ``ptr`` is the view's first row, ``nbytes`` the size of the buffer at ``base``
    where it is known, ``owner`` what keeps that buffer alive"""
    nwalkers = 1  # (its pooled columns are those of a chain of one walker: nrows, nwalkers, ndim)
    nrows = S = property(lambda self: self.M)
    ndim = property(lambda self: self.ncol)

    def __init__(self, ctx, base, M, ncol, ld, owner, row0=0, nbytes=None):
        self.ctx, self.base, self.owner, self.nbytes = ctx, base, owner, nbytes
        self.M, self.ncol, self.ld, self.row0 = int(M), int(ncol), int(ld), int(row0)
        if self.M < 1 or self.ncol < 1 or self.ld < self.ncol or self.row0 < 0 or \
                (nbytes is not None and (self.row0 + self.M) * self.ld * 8 > nbytes):
            raise ValueError("a device matrix of %d x %d (ld %d) does not fit its buffer"
                             % (self.M, self.ncol, self.ld))
        self.ptr = base + 8 * self.row0 * self.ld  # (the one place a row offset becomes bytes)

    def rows(self, a, b):
        """the view of rows [a, b) of this one"""
        if not 0 <= a < b <= self.M:
            raise ValueError("rows [%d, %d) are not rows of a view of %d" % (a, b, self.M))
        return DeviceMatrix(self.ctx, self.base, b - a, self.ncol, self.ld, self.owner,
                            self.row0 + a, self.nbytes)

    def pooled(self):
        """(ptr, row0, nrows, ld, cstride, npool, ncolp) as nh_rank_columns, nh_rank_transform and
        nh_chain_cov take pooled columns: element t * npool + j of column p is
        x[(row0 + t) * ld + j * cstride + p]; a matrix pools nothing"""
        return (self.base, self.row0, self.M, self.ld, 0, 1, self.ncol)

    def get(self):
        """the host copy [M][ncol]; nothing behind the last row's last column is read"""
        from . import _lib
        host = np.empty((self.M, self.ld))
        _lib._chk(_lib._lib.nh_download(self.ctx.h, host.ctypes.data, self.ptr,
                                        8 * ((self.M - 1) * self.ld + self.ncol)))
        return host[:, :self.ncol]


class DeviceChain:
    """a chain [rows][nwalkers * ndim] in HBM: the DeviceMatrix ``m`` of its rows, and ``logp``,
    the DeviceMatrix [rows][nwalkers] of their log-probabilities, or None"""
    ctx = property(lambda self: self.m.ctx)
    ptr = property(lambda self: self.m.ptr)
    owner = property(lambda self: self.m.owner)
    nrows = property(lambda self: self.m.M)
    shape = property(lambda self: (self.m.M, self.nwalkers, self.ndim))
    S = property(lambda self: self.m.M * self.nwalkers, doc="values pooled per parameter")

    def __init__(self, m, nwalkers, ndim, logp=None):
        self.m, self.nwalkers, self.ndim, self.logp = m, int(nwalkers), int(ndim), logp
        if self.nwalkers < 1 or self.ndim < 1 or not m.ncol == m.ld == self.nwalkers * self.ndim:
            raise ValueError("a device chain of %d x %d x %d does not fit its buffer" % self.shape)
        if logp is not None and (logp.M, logp.ncol) != (m.M, self.nwalkers):
            raise ValueError("the device log-probabilities are not (%d, %d)" % self.shape[:2])

    def rows(self, a, b):
        """the view of rows [a, b) of this one, ``logp`` in step"""
        return DeviceChain(self.m.rows(a, b), self.nwalkers, self.ndim,
                           None if self.logp is None else self.logp.rows(a, b))

    def behind(self, discard):
        return self.rows(discard, self.nrows)

    def pooled(self):
        """``DeviceMatrix.pooled`` of every parameter, all walkers pooled"""
        return self.m.pooled()[:4] + (self.ndim, self.nwalkers, self.ndim)

    def flat(self):
        """the DeviceMatrix [rows * nwalkers][ndim] of the same values"""
        m = self.m
        return DeviceMatrix(m.ctx, m.base, self.S, self.ndim, self.ndim, m.owner,
                            m.row0 * self.nwalkers, m.nbytes)


def matrix_on(buf, M, ncol, ld=None):
    """the DeviceMatrix [M][ncol] that starts the device array ``buf``"""
    return DeviceMatrix(buf.ctx, buf.ptr, M, ncol, ncol if ld is None else ld, buf, 0,
                        getattr(buf, "nbytes", None))


def _is_block(x):  # (a legacy tuple: a device array and three integers)
    return isinstance(x, tuple) and len(x) == 4 and not np.isscalar(x[0]) and hasattr(x[0], "ptr")


def _chain_block(x):
    if not _is_block(x):
        raise ValueError("a device chain is (DeviceArray, rows, nwalkers, ndim)")
    rows, nw, ndim = (int(v) for v in x[1:])
    if rows < 1 or nw < 1 or ndim < 1 or rows * nw * ndim * 8 > x[0].nbytes:
        raise ValueError("a device chain of %d x %d x %d does not fit its buffer"
                         % (rows, nw, ndim))
    return DeviceChain(matrix_on(x[0], rows, nw * ndim), nw, ndim)


def matrix_shape(x, pointwise=False):
    """(M, ncol) of what ``as_matrix`` makes of ``x``, checked without a device; ``pointwise``: a
    host array must be 2-D (samples, data points), else (M,) is one column"""
    if isinstance(x, DeviceMatrix) or _is_block(x):
        x = as_matrix(x)
        return x.M, x.ncol
    s = np.shape(x)
    if len(s) == 1 and not pointwise:
        s = (s[0], 1)
    if len(s) != 2:
        raise ValueError("a pointwise matrix must be 2-D (samples, data points); got shape %s"
                         % (tuple(s),) if pointwise else "samples must be (M,) or (M, ncol)")
    if s[0] == 0 or s[1] == 0:
        raise ValueError("no samples")
    return int(s[0]), int(s[1])


def as_matrix(x):
    """``x`` as a DeviceMatrix: one as it is, ``(DeviceArray, M, ncol, ld)``, or a host array
    ``(M,)`` / ``(M, ncol)``, which is uploaded"""
    if isinstance(x, DeviceMatrix):
        return x
    if _is_block(x):
        return matrix_on(*x)
    from . import _lib
    M, ncol = matrix_shape(x)
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(M, ncol))
    return matrix_on(_lib.get_context().array(a), M, ncol)


def chain_dims(x, discard=0, least=0):
    """(rows, nwalkers, ndim) of what ``as_chain`` takes -- a DeviceChain, ``(DeviceArray, rows,
    nwalkers, ndim)`` or a host array (rows, nwalkers, ndim) -- with at least ``least`` rows
    behind ``discard``; checked without a device"""
    if isinstance(x, (tuple, DeviceChain)):
        rows, nw, ndim = (_chain_block(x) if isinstance(x, tuple) else x).shape
    else:
        shape = np.shape(x)
        if len(shape) != 3:
            raise ValueError("a chain must be (rows, nwalkers, ndim)")
        rows, nw, ndim = shape
        if nw < 1 or ndim < 1:
            raise ValueError("the chain has no walkers or no parameters")
    discard = int(discard)
    if discard < 0:
        raise ValueError("discard must not be negative")
    if rows - discard < least:
        raise ValueError("%d rows behind discard = %d: %d needed at least"
                         % (max(0, rows - discard), discard, least))
    return rows, nw, ndim


def as_chain(x, discard=0, least=1, logp=None):
    """the DeviceChain of the rows of ``x`` (as ``chain_dims`` takes it) behind ``discard``; a host
    array is uploaded whole.  ``logp`` (rows, nwalkers), as ``as_matrix`` takes it, travels with
    the chain in place of what ``x`` carried."""
    rows, nw, ndim = chain_dims(x, discard, least)
    if isinstance(x, tuple):
        x = _chain_block(x)
    elif not isinstance(x, DeviceChain):
        from . import _lib
        a = np.ascontiguousarray(x, dtype=np.float64).reshape(rows, nw * ndim)
        x = DeviceChain(matrix_on(_lib.get_context().array(a), rows, nw * ndim), nw, ndim)
    if logp is not None:
        x = DeviceChain(x.m, nw, ndim, as_matrix(logp))
    return x.behind(discard)
