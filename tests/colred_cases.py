"""The six entry points that reduce the columns of a device matrix in the tiling of
csrc/nh_colred.h, each as one function from a shape (M, ncol) to its inputs and its device
outputs: what tests/test_gpu_colred.py checks against the NumPy restatements, and what a script
that compares two builds of the library dumps.  Every matrix lies inside one of row stride
ld = ncol + pad whose padding is NaN."""
import ctypes as C

import numpy as np

import infocrit_np as RI
from test_infocrit_host import spectra, table

NCOLS = [1, 3, 65]       # cw = 1 (256 row lanes) | cw = 4, one idle column lane | two tiles, 64 + 1
MS = [1, 255, 2049]      # one row | fewer rows than the row lanes of cw = 1 | three chunks, a short one
PAD = 2
POISON = -7.25e33
ENTRIES = ("column_moments", "lnl_column_stats", "psis_columns", "pit_columns", "psis_weights",
           "weighted_moments")


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def padded(x, pad, fill=np.nan):
    host = np.full((x.shape[0], x.shape[1] + pad), fill)
    host[:, :x.shape[1]] = x
    return host


def rng_of(M, ncol, salt):
    return np.random.default_rng(100003 * salt + 31 * M + ncol)


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def moments_input(M, ncol):
    """columns of different scale; from five rows on a NaN, a +inf and a -inf"""
    rng = rng_of(M, ncol, 1)
    x = rng.normal(0.0, 1.0, (M, ncol)) * np.exp(rng.normal(0.0, 2.0, ncol)) + rng.normal(0, 5, ncol)
    if M >= 5:
        x[M - 1, 0] = np.nan
        x[M - 2, ncol - 1] = np.inf
        x[3, ncol // 2] = -np.inf
    return x


def lnl_input(M, ncol):
    """log-likelihood terms by column: light-tailed, heavy-tailed, far down (exp() of them is
    subnormal or zero unless the maximum is subtracted first); column 1 is constant"""
    rng = rng_of(M, ncol, 2)
    L = np.empty((M, ncol))
    for c in range(ncol):
        z = rng.standard_normal(M)
        L[:, c] = (-0.5 * (0.3 * z - 0.5) ** 2, -0.5 * (8.0 * z) ** 2,
                   -700.0 - 60.0 * rng.random(M) ** 2)[c % 3]
    if ncol > 1:
        L[:, 1] = -3.25
    return L


def pit_input(M, ncol):
    t = table("some-mixed" if ncol > 1 else "none-uniform", nE=ncol, seed=ncol)
    return spectra(t, M, seed=M), t


def bad_ratio_column(M, ncol):
    """the column of ratio_input that gets no weights, or None"""
    return ncol - 1 if ncol > 1 or M == 255 else None


def ratio_input(M, ncol):
    """log-ratios by column: lognormal, heavy ties, all equal, every third row -inf; the last
    column (the only one at M = 255, none at the other M) holds a NaN and, from two rows on, a +inf"""
    rng = rng_of(M, ncol, 3)
    lr = np.empty((M, ncol))
    for c in range(ncol):
        z = rng.normal(0.0, 1.0, M)
        if c % 4 == 3:
            z[::3] = -np.inf
            z[M // 2] = 0.25
        lr[:, c] = (1.5 * z, np.round(2 * z) / 2, np.full(M, -2.5), z)[c % 4]
    bad = bad_ratio_column(M, ncol)
    if bad is not None:
        lr[M // 2, bad] = np.nan
        if M > 1:
            lr[0, bad] = np.inf
    return lr


def weighted_input(M, ncol):
    """(x, lw): every fourth row (not the first) has weight zero and holds NaN; column 2 is
    constant under positive weight"""
    rng = rng_of(M, ncol, 4)
    x = rng.normal(3.0, 2.0, (M, ncol)) * np.exp(rng.normal(0, 1, ncol))
    lw = rng.normal(0.0, 1.0, M)
    lw[4::4] = -np.inf
    lw = lw - RI.logsumexp(lw)
    dead = np.isneginf(lw)
    x[dead] = np.nan
    if ncol > 2:
        x[~dead, 2] = 1.25
    return x, lw


# ---------------------------------------------------------------------------------------
# the entry points through the C ABI: dicts of host arrays
# ---------------------------------------------------------------------------------------
def column_moments(x, pad=PAD):
    c = ctx()
    M, ncol = x.shape
    dx, counts, stats = c.array(padded(x, pad)), c.empty((2, ncol), np.int64), c.empty((4, ncol))
    c.call("nh_column_moments", dx, M, ncol, ncol + pad, counts, stats)
    return dict(counts=counts.get(), stats=stats.get())


def _lnl_stats(c, dL, M, ncol, ld):
    st = c.empty((5, ncol))
    c.call("nh_lnl_column_stats", dL, M, ncol, ld, st)
    return st


def lnl_column_stats(L, pad=PAD):
    c = ctx()
    M, ncol = L.shape
    dL = c.array(padded(L, pad))
    return dict(stats=_lnl_stats(c, dL, M, ncol, ncol + pad).get())


def psis_columns(L, pad=PAD):
    c = ctx()
    M, ncol = L.shape
    ld, Mt = ncol + pad, RI.tail_length(M)
    dL = c.array(padded(L, pad))
    st = _lnl_stats(c, dL, M, ncol, ld)
    lsel = c.empty((1, ncol))
    c.call("nh_column_select", dL, M, ncol, ld, (C.c_int * 1)(Mt), 1, lsel)
    k, n, elpd = c.empty((ncol,)), c.empty((ncol,), np.int64), c.empty((ncol,))
    c.call("nh_psis_columns", dL, M, ncol, ld, Mt, st, lsel, k, n, elpd)
    return dict(pareto_k=k.get(), n_tail=n.get(), elpd=elpd.get())


def pit_columns(xt, pad=PAD):
    x, t = xt
    c = ctx()
    M, nE = x.shape
    dx, out = c.array(padded(x, pad)), c.array(np.full((2, nE), POISON))
    cols = (c.array(t["conv"]), c.array(t["flux"]), c.array(t["flux_error_lo"]),
            c.array(t["flux_error_hi"]), c.array(t["ul"].astype(np.int32), dtype=np.int32))
    c.call("nh_pit_columns", dx, M, nE, nE + pad, *cols, out)
    return dict(out=out.get())


def psis_weights(lr, pad=PAD):
    """lw lies in a block of row stride ncol + 1 whose last column must stay what it was"""
    c = ctx()
    M, K = lr.shape
    ld, ldw, Mt = K + pad, K + 1, RI.tail_length(M)
    dx = c.array(padded(lr, pad))
    lsel = c.empty((1, K))
    c.call("nh_column_select", dx, M, K, ld, (C.c_int * 1)(M - Mt - 1), 1, lsel)
    lw = c.array(np.full((M, ldw), POISON))
    k, n, ess, lm = c.empty((K,)), c.empty((K,), np.int64), c.empty((K,)), c.empty((K,))
    st = c.empty((K,), np.int32)
    c.call("nh_psis_weights", dx, M, K, ld, Mt, lsel, lw, ldw, k, n, ess, lm, st)
    return dict(lw=lw.get(), pareto_k=k.get(), n_tail=n.get(), ess=ess.get(), lmean=lm.get(),
                status=st.get())


def weighted_moments(xlw, pad=PAD):
    """the weights are column 1 of a block [M][3]"""
    x, lw = xlw
    c = ctx()
    M, ncol = x.shape
    block = np.full((M, 3), POISON)
    block[:, 1] = lw
    dx, dw, out = c.array(padded(x, pad)), c.array(block), c.empty((3, ncol))
    c.call("nh_weighted_moments", dx, M, ncol, ncol + pad, dw.ptr + 8, 3, out)
    return dict(out=out.get())


INPUTS = dict(column_moments=moments_input, lnl_column_stats=lnl_input, psis_columns=lnl_input,
              pit_columns=pit_input, psis_weights=ratio_input, weighted_moments=weighted_input)
CALLS = dict(column_moments=column_moments, lnl_column_stats=lnl_column_stats,
             psis_columns=psis_columns, pit_columns=pit_columns, psis_weights=psis_weights,
             weighted_moments=weighted_moments)


def run(entry, M, ncol, pad=PAD):
    """the device outputs of `entry` at (M, ncol), as a dict of host arrays"""
    return CALLS[entry](INPUTS[entry](M, ncol), pad)
