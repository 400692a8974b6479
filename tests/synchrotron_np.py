"""A long double NumPy restatement of nh_synchrotron (include/naima_hip.h), written from the entry
point's contract -- Synchrotron._spectrum (radiative.py:282-342) through trapz_loglog's segment
rules (utils.py:336-351) -- from the same float64 inputs the device gets, and a generator of such
inputs.  The tests hold the device to it; tests/test_synchrotron_host.py holds IT to
oracle.naima_np.synchrotron_spectrum and to mpmath.  No GPU, no naima_amd import.

With x_i = E/Ec(gamma_i, B), P of AKP10 Eq. D7 and the node u_i = w_i P(x_i) exp(-x_i), a
segment's log-ratio is
    dl = dlw[i] + ln(P_{i+1}/P_i) - (x_{i+1} - x_i)
(analytic: nothing in it cancels) and its term, as integrate_np.terms states trapz_loglog's rules,
    0                       where u_i or u_{i+1} is zero
    NaN                     where one of them is NaN (and neither is zero)
    u_i lx expm1(dl)/dl     elsewhere (u_i lx at dl = 0).
spec = CS1 erg/eV * the sum of the terms.

Rules of this reference:
  * a node with x > 746 is DEAD: float64's exp(-x) is exactly 0 there (from x = 745.14 on), so the
    oracle's node is an exact zero and the zero-node rule kills both its segments.  A NaN or
    infinite weight at a dead node is killed with it: only a bad weight inside an energy's live
    range [i0, nG) makes that energy NaN.  (nh_synchrotron never reads the dead nodes and agrees;
    the resident loops make the whole row NaN on purpose -- syn_nan -- which is their contract, not
    this entry point's.)
  * between 745.14 and 746 float64 has flushed the node to zero and this reference has not: what
    that leaves is below 2^-1070 of a weight of 1 and falls under the tests' underflow cap.
  * B <= 0, NaN or +inf: the whole row is NaN.
  * one deviation from the oracle, recorded and not tested: a NaN weight at the LAST node reaches
    the oracle through b = NaN alone, i.e. through its log branch x1 y1 ln(x2/x1), which is
    finite.  Here it is NaN.  The tests plant NaNs at interior nodes only."""
import numpy as np

from oracle import naima_np as O

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended long double"

X_DEAD = 746.0
DL_ZERO = 1e300  # |dlw| next to a zero weight (nh_pdist.h clamps ln(0/w) to it)
# the planted total log-ratios of make_inputs, around NH_SEG_SMALL_POS = 2^-10 (nh_common.h)
PLANT_DL = (0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -11, -2.0 ** -11, 2.0 ** -10 * (1 + 2.0 ** -8),
            2.0 ** -10 * (1 - 2.0 ** -8), 2.0 ** -9)

_E, _C, _HBAR, _ME, _ERG = (LD(O.E_GAUSS), LD(O.C_CGS), LD(O.HBAR_CGS), LD(O.M_E_G),
                            LD(O.ERG_PER_EV))


def P_of(x):
    """AKP10 Eq. D7 without its exponential (oracle.naima_np.gtilde), in the precision of x"""
    cb = np.cbrt(x)
    cb2 = cb * cb
    cb4 = cb2 * cb2
    g1 = LD(1.808) * cb / np.sqrt(1 + LD(3.4) * cb2)
    g2 = 1 + LD(2.210) * cb2 + LD(0.347) * cb4
    g3 = 1 + LD(1.353) * cb2 + LD(0.217) * cb4
    return g1 * (g2 / g3)


def x_of(B, gam, E_eV):
    """x[k][i] = E_k / Ec(gamma_i, B), Ec = 3 e hbar B gamma^2 / (2 m_e c), in long double"""
    g = np.asarray(gam, dtype=LD)
    q = (np.asarray(E_eV, dtype=LD) * _ERG) * (2 * (_ME * _C)) / (3 * _E * _HBAR * LD(B))
    return q[:, None] / (g * g)[None, :]


def cs1_of(B, E_eV):
    """CS1 erg/eV = sqrt(3) e^3 B / (2 pi m_e c^2 hbar E) * erg/eV  [nE]: radiative.py:319-328,
    340"""
    E_erg = np.asarray(E_eV, dtype=LD) * _ERG
    pi = LD(4) * np.arctan(LD(1))
    return (np.sqrt(LD(3)) * _E ** 3 * LD(B)) / (2 * pi * _ME * _C ** 2 * _HBAR * E_erg) * _ERG


def first_live(x):
    """i0[k]: the first node with x <= 746, nG if none (x decreases along the grid)"""
    live = x <= X_DEAD
    return np.where(live.any(axis=1), live.argmax(axis=1), x.shape[1])


def row_terms(w, dlw, B, gam, lx, E_eV, with_s2=False):
    """(term [nE][nG-1] before CS1, x [nE][nG], dl [nE][nG-1]) of one walker with a good field;
    with_s2: and s^2 = ((P2 - P1)/(P2 + P1))^2 [nE][nG-1], what syn_dlnP1 picks its form by"""
    w, dlw, lx = np.asarray(w, dtype=LD), np.asarray(dlw, dtype=LD), np.asarray(lx, dtype=LD)
    x = x_of(B, gam, E_eV)
    with np.errstate(all="ignore"):
        P = P_of(x)
        u = np.where(x <= X_DEAD, w[None, :] * (P * np.exp(-x)), LD(0))
        u1, u2 = u[:, :-1], u[:, 1:]
        P1, P2 = P[:, :-1], P[:, 1:]
        dl = dlw[None, :-1] + np.log1p((P2 - P1) / P1) - (x[:, 1:] - x[:, :-1])
        ul = u1 * lx[None, :]
        safe = np.where((dl == 0) | np.isnan(dl), LD(1), dl)
        t = np.where(dl == 0, ul, ul * (np.expm1(safe) / safe))
        t = np.where(np.isnan(u1) | np.isnan(u2), LD(np.nan), t)
    t = np.where((u1 == 0) | (u2 == 0), LD(0), t)
    if with_s2:
        return t, x, dl, ((P2 - P1) / (P2 + P1)) ** 2
    return t, x, dl


def spectrum(w, dlw, B, gam, lx, E_eV):
    """dict of [N][nE] arrays for walker rows w, dlw [N][nG] and fields B [N]:
    spec  the spectrum, 1/(s eV);   S = CS1 sum |term|;   SX = CS1 sum |term| max(x_i, x_{i+1}),
    the share of the sum that sits far down the exponential, where a rounding of x counts x-fold;
    S_raw = sum |term| before CS1;  cs1;  i0 (int) the liveness map;
    and s2 [3]: the largest s^2 among the segments with a non-zero term in each range of
    syn_dlnP1's forms, s^2 <= 1e-4, <= 9e-4 and above (0 where a range is empty)"""
    w, dlw = np.atleast_2d(w), np.atleast_2d(dlw)
    N, nG = w.shape
    nE = len(E_eV)
    out = {k: np.full((N, nE), LD(np.nan)) for k in ("spec", "S", "SX", "S_raw", "cs1")}
    out["i0"] = np.full((N, nE), nG, dtype=np.int64)
    out["s2"] = np.zeros(3)
    for r in range(N):
        if not (B[r] > 0 and np.isfinite(B[r])):
            continue
        t, x, _, s2 = row_terms(w[r], dlw[r], B[r], gam, lx, E_eV, with_s2=True)
        cs1 = cs1_of(B[r], E_eV)
        a = np.abs(t)
        s2 = s2[a > 0].astype(np.float64)
        for j, (lo, hi) in enumerate(((-1, 1e-4), (1e-4, 9e-4), (9e-4, np.inf))):
            m = s2[(s2 > lo) & (s2 <= hi)]
            out["s2"][j] = max(out["s2"][j], m.max() if m.size else 0.0)
        out["spec"][r] = cs1 * t.sum(axis=1)
        out["S_raw"][r] = a.sum(axis=1)
        out["S"][r] = cs1 * out["S_raw"][r]
        out["SX"][r] = cs1 * (a * np.maximum(x[:, :-1], x[:, 1:])).sum(axis=1)
        out["cs1"][r] = cs1
        out["i0"][r] = first_live(x)
    return out


def make_inputs(seed, R, B, gam, lx, E_eV, ln_top=None):
    """dict(w, dlw [R][nG], planted): positive weights built from their log-ratios.  dlw are
    multiples of 2^-20 around a power law -- slope per walker in [-3, 0.5], jitter of 0.3 of a
    segment's width -- summed and exponentiated in long double, rounded once.  Every walker r with a
    good field has one planted (energy k, segment i) -- a live segment with 0.05 <= x_i <= 20, where
    the integrand peaks -- whose dlw[i] is set, in long double, so that the total dl of (k, i) is
    PLANT_DL[r % 8]: `planted` lists (r, k, i, target).  The largest weight of a walker is 1, or
    with `ln_top` its last one is e^ln_top (weights of 1 put every energy whose live nodes all have
    x > 665 under the tests' underflow cap; a heavier top of the grid brings those with
    x < 708, where float64's exp(-x) is still a normal number, back above it).  Zero weights:
    the top min(nG // 8, 40) nodes of every walker with r % 4 == 1 (dlw = -1e300 from the last
    positive node on) and one interior node of every walker with r % 4 == 2 (dlw = -1e300 into it,
    +1e300 out of it).
    On a grid of more than twelve decades "the largest weight" is the largest of the top twelve
    (no energy of the cases is live below them); further down a weight stops growing at e^400 =
    5e173 (dlw = 0 between two such nodes; w / gamma stays a float64 for the oracle) and one below 1e-250 is an exact zero, marked
    -+1e300 like the planted ones -- as nh_pdist.h ends a distribution whose cutoff underflows."""
    rng = np.random.default_rng(seed)
    nG = len(gam)
    q20 = 2.0 ** -20
    lxd = np.asarray(lx, dtype=np.float64)
    slope = rng.uniform(-3.0, 0.5, size=(R, 1))
    jit = rng.uniform(-0.3, 0.3, size=(R, nG - 1))
    dlw = np.zeros((R, nG))
    dlw[:, :-1] = np.rint((slope + jit) * lxd[None, :] / q20) * q20
    planted = []
    for r in range(R):
        if not (B[r] > 0 and np.isfinite(B[r])) or nG < 3:
            continue
        x = x_of(B[r], gam, E_eV)
        ok = np.argwhere((x[:, :-1] <= 20) & (x[:, :-1] >= 0.05))
        # (not next to the zeros planted below)
        ok = [(k, i) for k, i in ok if i + 2 < nG - min(nG // 8, 40) and abs(i - nG // 3) > 1]
        if not ok:
            continue
        k, i = ok[(7 * r + 3) % len(ok)]
        P = P_of(x[k, i:i + 2])
        rest = np.log1p((P[1] - P[0]) / P[0]) - (x[k, i + 1] - x[k, i])
        dlw[r, i] = np.float64(LD(PLANT_DL[r % 8]) - rest)
        planted.append((r, int(k), int(i), PLANT_DL[r % 8]))
    lnw = np.zeros((R, nG), dtype=LD)
    lnw[:, 1:] = np.cumsum(dlw[:, :-1].astype(LD), axis=1)
    if ln_top is None:
        top = np.asarray(gam) >= gam[-1] * 1e-12
        lnw -= lnw[:, top].max(axis=1, keepdims=True)  # the largest weight is 1
    else:
        lnw += ln_top - lnw[:, [-1]]                   # the LAST weight is e^ln_top
    capped = lnw > 400
    if capped.any():
        lnw = np.minimum(lnw, LD(400))
        seg = capped[:, :-1] | capped[:, 1:]
        dlw[:, :-1][seg] = (lnw[:, 1:] - lnw[:, :-1])[seg].astype(np.float64)
    w = np.exp(lnw).astype(np.float64)
    w[w < 1e-250] = 0.0
    for r in range(R):
        if r % 4 == 1 and nG >= 16:
            z = nG - min(nG // 8, 40)
            w[r, z:] = 0.0
            dlw[r, z - 1:-1] = -DL_ZERO
        if r % 4 == 2 and nG >= 16:
            z = nG // 3
            w[r, z] = 0.0
            dlw[r, z - 1], dlw[r, z] = -DL_ZERO, DL_ZERO
    z1, z2 = w[:, :-1] == 0, w[:, 1:] == 0
    dlw[:, :-1] = np.where(z2, -DL_ZERO, np.where(z1, DL_ZERO, dlw[:, :-1]))
    return dict(w=w, dlw=dlw, planted=planted)
