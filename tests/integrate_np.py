"""A long double NumPy restatement of nh_integrate_tables (include/naima_hip.h), written from the
entry point's contract and from trapz_loglog's segment rules (utils.py:336-351), and a generator of
inputs whose nodes and log-ratios agree to 2 ulp.  The tests hold the device to it;
tests/test_integrate_host.py holds IT to oracle.naima_np.trapz_loglog and to mpmath.  No GPU, no
naima_amd import.

With u = w_i * Kt[i][k] and dl = dlw[i] + dlnKt[i][k] = ln(u2/u1) a segment's term is
    0                       where u1 or u2 is zero                  (utils.py:347-348)
    u1 * lx                 where u1, u2 differ in sign or dl is NaN (the log branch a NaN b takes)
    lx * u1 * expm1(dl)/dl  elsewhere (u1 * lx at dl = 0)
which is y1 (x2 (x2/x1)^b - x1)/(b + 1) for y = u/x, b + 1 = dl/lx: the continuous form, whose
dl -> 0 limit is the log branch the reference switches to at |b + 1| <= 1e-10."""
import numpy as np

LD = np.longdouble
DL_ZERO = 1e300  # dlnKt where a table node of the segment is zero (what the nh_table_* builders write)
# planted log-ratios around the series thresholds (2^-10 non-negative form, 2^-7 signed form)
PEAK_DL = (0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -11, -2.0 ** -11, 2.0 ** -10, -2.0 ** -10, 2.0 ** -9)
PEAK_LARGE = (2.0 ** -10, -2.0 ** -10, 2.0 ** -9)  # none of them below 2^-10


def terms(w, dlw, lx, Kt, dlnKt):
    """term[r][i][k] of walker rows w [R][nG], dlw [R][nG], lx [nG-1], Kt, dlnKt [nG][nK]"""
    w, dlw, lx = np.asarray(w, dtype=LD), np.asarray(dlw, dtype=LD), np.asarray(lx, dtype=LD)
    Kt, dlnKt = np.asarray(Kt, dtype=LD), np.asarray(dlnKt, dtype=LD)
    u = w[:, :, None] * Kt[None, :, :]
    u1, u2 = u[:, :-1], u[:, 1:]
    with np.errstate(all="ignore"):
        dl = dlw[:, :-1, None] + dlnKt[None, :-1, :]
        ul = u1 * lx[None, :, None]
        safe = np.where((dl == 0) | np.isnan(dl), LD(1), dl)
        t = np.where(dl == 0, ul, ul * (np.expm1(safe) / safe))
        t = np.where((np.signbit(u1) != np.signbit(u2)) | np.isnan(dl), ul, t)
        t = np.where(np.isnan(u1) | np.isnan(u2), LD(np.nan), t)  # (a NaN node is not a zero node)
    return np.where((u1 == 0) | (u2 == 0), LD(0), t)


def integrate(w, dlw, lx, Kt, dlnKt, scale=None, nsplit=1):
    """(planes [nsplit][R][nK], S [nsplit][R][nK]): plane h = scale[k] * the sum of the terms of
    segments [h*hper, (h+1)*hper), hper = ceil(nseg/nsplit), and S the same sum of |term|"""
    t = terms(w, dlw, lx, Kt, dlnKt)
    R, nseg, nK = t.shape
    sc = np.ones(nK, dtype=LD) if scale is None else np.asarray(scale, dtype=LD)
    hper = -(-nseg // nsplit)
    planes, S = np.zeros((nsplit, R, nK), dtype=LD), np.zeros((nsplit, R, nK), dtype=LD)
    for h in range(nsplit):
        seg = t[:, h * hper:min(nseg, (h + 1) * hper)]
        planes[h] = sc * seg.sum(axis=1)
        S[h] = np.abs(sc) * np.abs(seg).sum(axis=1)
    return planes, S


def make_inputs(seed, R, nG, nK):
    """dict(w, dlw [R][nG], lx [nG-1], Kt, dlnKt [nG][nK], peaks): positive nodes built from
    log-ratios that are multiples of 2^-20 in [-1, 1] -- drawn first, summed and exponentiated
    in long double, then rounded to double.  Two segments (`peaks`) have the SAME dl for every
    walker: PEAK_DL[k % 8] in the first (every wave has lanes on both sides of the series
    threshold), PEAK_LARGE[k % 3] in the second (no lane below it)."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -20
    dlw = np.zeros((R, nG))
    dK = np.zeros((nG, nK))
    dlw[:, :-1] = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(R, nG - 1)) * q
    dK[:-1] = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(nG - 1, nK)) * q
    nseg = nG - 1
    peaks = sorted({nseg // 3, (2 * nseg) // 3}) if nseg >= 3 else []
    k = np.arange(nK)
    for n, i in enumerate(peaks):
        a = rng.integers(-2 ** 18, 2 ** 18 + 1) * q
        dlw[:, i] = a
        dK[i] = (np.take(PEAK_DL, k % 8) if n == 0 else np.take(PEAK_LARGE, k % 3)) - a
    lnw = np.zeros((R, nG), dtype=LD)
    lnK = np.zeros((nG, nK), dtype=LD)
    lnw[:, 1:] = np.cumsum(dlw[:, :-1].astype(LD), axis=1)
    lnK[1:] = np.cumsum(dK[:-1].astype(LD), axis=0)
    lnw += LD(rng.uniform(-2, 2, size=(R, 1)))
    lnK += LD(rng.uniform(-2, 2, size=(1, nK)))
    lx = rng.uniform(0.01, 0.1, size=nG - 1)
    return dict(w=np.exp(lnw).astype(np.float64), dlw=dlw, lx=lx,
                Kt=np.exp(lnK).astype(np.float64), dlnKt=dK, peaks=peaks)


def plant_zeros(d, seed):
    """zero table entries inside the non-negative contract (dlnKt = 1e300 on both adjacent
    segments): isolated zeros, a run across the middle of the abscissa, column 1 whole, and the
    second 64-column tile whole where the table has one.  In place; returns d."""
    rng = np.random.default_rng(seed)
    Kt, dK = d["Kt"], d["dlnKt"]
    nG, nK = Kt.shape
    zero = np.zeros((nG, nK), dtype=bool)
    for _ in range(max(2, nG * nK // 50)):
        zero[rng.integers(nG), rng.integers(nK)] = True
    zero[0, nK // 2] = zero[nG - 1, nK // 2] = True  # (both ends of the abscissa)
    zero[nG // 2 - min(3, nG // 4):nG // 2 + 2, 0] = True
    if nK > 1:
        zero[:, 1] = True
    if nK >= 128:
        zero[:, 64:128] = True
    Kt[zero] = 0.0
    dK[:-1][zero[:-1] | zero[1:]] = DL_ZERO
    return d


def plant_signed(d, seed):
    """what only the signed form accepts, on rows w [R >= 3][nG]: sign changes in Kt (dl left
    finite at some, NaN at others), a NaN dl without a sign change, an all-negative walker, exact
    zeros and -0.0 in w and Kt with an ordinary finite dl.  In place; returns d."""
    rng = np.random.default_rng(seed)
    w, Kt, dK = d["w"], d["Kt"], d["dlnKt"]
    nG, nK = Kt.shape
    for n in range(max(2, nK // 3)):
        i, k = rng.integers(1, nG), rng.integers(nK)
        Kt[i:, k] = -Kt[i:, k]
        if n % 2:
            dK[i - 1, k] = np.nan
    for _ in range(max(1, nK // 8)):
        dK[rng.integers(nG - 1), rng.integers(nK)] = np.nan
    w[1] = -w[1]
    for n in range(max(4, nG * nK // 100)):
        Kt[rng.integers(nG), rng.integers(nK)] = (0.0, -0.0)[n % 2]
    for n in range(max(2, nG // 20)):
        w[rng.integers(w.shape[0]), rng.integers(nG)] = (0.0, -0.0)[n % 2]
    return d
