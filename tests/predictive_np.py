"""A float64 NumPy restatement of what naima_amd.predictive's kernels compute (nh_ppc_rows,
nh_ppc_counts, nh_pit_columns), written from the definitions: Philox4x32-10 (Salmon, Moraes, Dror
& Shaw 2011) with uint64 products, the split-normal draw the likelihood implies, the six
discrepancy statistics of a row, the comparison counts and the probability integral transform
(math.erfc; no scipy).  The tests hold the device to it; tests/test_predictive_host.py holds IT to
Random123's known answers and to the moments of the distribution it draws from.  No GPU, no
naima_amd import."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32(ctr, key, rounds=10):
    """ctr = (c0, c1, c2, c3), key = (k0, k1): arrays (or scalars) of 32-bit words that broadcast
    against each other -> the four output words as uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK for k in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2  # (32 x 32 bits: no overflow of 64)
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def draw(M, nE, elo, ehi, seed=0, row0=0):
    """(a [M][nE], below [M][nE]): the half-normal and the side of the replicate of every
    (row0 + s, k)"""
    seed = int(seed) & (2 ** 64 - 1)
    row = (np.arange(M, dtype=np.uint64) + np.uint64(row0))[:, None]
    k = np.arange(nE, dtype=np.uint64)[None, :]
    r0, r1, r2, r3 = philox4x32((row & MASK, row >> S32, k, 0), (seed & 0xFFFFFFFF, seed >> 32))
    r0, r1, r2, r3 = np.broadcast_arrays(r0, r1, r2, r3)
    U = (((r0 << np.uint64(20)) | (r1 >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
    V = (r2.astype(np.float64) + 0.5) * 2.0 ** -32
    W = r3.astype(np.float64) * 2.0 ** -32
    a = np.sqrt(-2.0 * np.log(U)) * np.abs(np.cos(2 * np.pi * V))
    elo, ehi = np.asarray(elo, dtype=float), np.asarray(ehi, dtype=float)
    below = W * (elo + ehi) < ehi
    return a, below


def runs(pos):
    """1 + the number of sign changes along the last axis of a boolean matrix; 0 without a
    column"""
    if pos.shape[-1] == 0:
        return np.zeros(pos.shape[:-1])
    return 1.0 + (pos[..., 1:] != pos[..., :-1]).sum(axis=-1)


def ppc_rows(x, conv, flux, elo, ehi, ul, seed=0, row0=0):
    """(Y [M][nE], T [M][6], below [M][nE]) of spectra x [M][nE] in the model's unit: y_rep (mc
    at an upper limit) and chi2_obs, chi2_rep, maxabs_obs, maxabs_rep, runs_obs, runs_rep over
    the points that are not upper limits, in column order"""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    M, nE = x.shape
    ul = np.asarray(ul, dtype=bool)
    elo, ehi = np.asarray(elo, dtype=float), np.asarray(ehi, dtype=float)
    mc = x * conv
    a, below = draw(M, nE, elo, ehi, seed, row0)
    Y = np.where(ul, mc, np.where(below, mc - ehi * a, mc + elo * a))
    d = mc - flux
    with np.errstate(divide="ignore", invalid="ignore"):
        r_obs = (-d / np.where(d > 0, ehi, elo))[:, ~ul]
    r_rep = np.where(below, -a, a)[:, ~ul]
    T = np.zeros((M, 6))
    if r_obs.shape[1]:
        T[:, 0], T[:, 1] = (r_obs ** 2).sum(axis=1), (r_rep ** 2).sum(axis=1)
        T[:, 2], T[:, 3] = np.abs(r_obs).max(axis=1), np.abs(r_rep).max(axis=1)
        T[:, 4], T[:, 5] = runs(r_obs >= 0), runs(r_rep >= 0)
    return Y, T, below


def ppc_counts(T):
    """[#(chi2_rep >= chi2_obs), #(maxabs_rep >= maxabs_obs), #(runs_rep <= runs_obs), #rows with
    a non-finite entry], the first three over the other rows"""
    T = np.asarray(T, dtype=float)
    ok = np.isfinite(T).all(axis=1)
    t = T[ok]
    return np.array([(t[:, 1] >= t[:, 0]).sum(), (t[:, 3] >= t[:, 2]).sum(),
                     (t[:, 5] <= t[:, 4]).sum(), (~ok).sum()], dtype=np.int64)


def p_values(T):
    """(p_chi2, p_max, p_runs, n_bad)"""
    c = ppc_counts(T)
    good = len(T) - c[3]
    return c[0] / good, c[1] / good, c[2] / good, int(c[3])


_erfc = np.vectorize(math.erfc, otypes=[float])
_erf = np.vectorize(math.erf, otypes=[float])


def split_normal_cdf(y, m, elo, ehi):
    """F(y | m): scale ehi on the side y < m, elo on the side y > m; the lower tail through
    erfc"""
    y, m, elo, ehi = np.broadcast_arrays(*(np.asarray(v, dtype=float) for v in (y, m, elo, ehi)))
    z, w = y - m, elo + ehi
    low = z <= 0
    out = np.empty(z.shape)
    up = ~low
    out[low] = 2.0 * ehi[low] / w[low] * (0.5 * _erfc(-(z[low] / ehi[low]) / math.sqrt(2.0)))
    out[up] = ehi[up] / w[up] + 2.0 * elo[up] / w[up] * (0.5 * _erf((z[up] / elo[up])
                                                                    / math.sqrt(2.0)))
    return out


def pit_columns(x, conv, flux, elo, ehi, ul):
    """[2][nE]: pit (NaN at an upper limit) and ul_violation (NaN elsewhere)"""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    ul = np.asarray(ul, dtype=bool)
    mc = x * conv
    out = np.full((2, x.shape[1]), np.nan)
    p = ~ul
    if p.any():
        out[0, p] = split_normal_cdf(np.asarray(flux)[p], mc[:, p], np.asarray(elo)[p],
                                     np.asarray(ehi)[p]).mean(axis=0)
    if ul.any():
        out[1, ul] = (mc[:, ul] > np.asarray(flux)[ul]).mean(axis=0)
    return out
