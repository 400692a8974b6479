"""A long double NumPy restatement of nh_syn_absorption and an mpmath restatement (50 digits) of
nh_ssa_apply (include/naima_hip.h), written from the entry points' contracts.  The per-electron
emissivity -- x = E/Ec, CS1, P of AKP10 Eq. D7 -- and the input generator are
tests/synchrotron_np.py's.  No GPU, no naima_amd import.

For N(gamma) particles per unit Lorentz factor in a volume V, w = gamma N:
    kappa(E) = alpha V = pi^2 hbar^3 CS1(E) / (m_e E) * trapz_loglog((N/gamma) H(x), gamma)
    H = 2 Gtilde (1 - D),  Gtilde = P(x) exp(-x),  D = dln Gtilde / dln x = Dp(cbrt x) - x.
With Q = P (1 - D) the node is u_i = (w_i / gamma_i) Q(x_i) exp(-x_i) (the factor 2 of H goes into
the prefactor), the segment's log-ratio dl = dlw[i] - lx[i] + ln(Q_{i+1}/Q_i) - (x_{i+1} - x_i), and
the term follows trapz_loglog's rules as synchrotron_np.row_terms states them: 0 where a node is 0,
NaN where one is NaN and neither is 0, u_i lx expm1(dl)/dl elsewhere.  A node with x > 746 is
dead; B <= 0, NaN or +-inf makes the row NaN.

The escape fraction of a homogeneous source of radius R (the contract of nh_ssa_apply):
    sphere  tau = 3 kappa / (2 pi R^2),  f = 3 u / tau,
            u = 1/2 + exp(-tau)/tau - (1 - exp(-tau))/tau^2          (Gould 1979)
            = sum_{n>=2} (-1)^n 3 n tau^(n-2) / (n+1)!
    slab    tau = kappa / (pi R^2),      f = (1 - exp(-tau)) / tau
f(0) = 1; a walker with R <= 0, NaN or +-inf has a NaN row; a NaN kappa gives NaN."""
import mpmath
import numpy as np

from synchrotron_np import (LD, X_DEAD, P_of, _C, _E, _ERG, _HBAR, _ME, cs1_of, first_live,
                            make_inputs, x_of)

__all__ = ["make_inputs", "D_of", "Q_of", "pref_of", "row_terms", "kappa", "tau_of", "escape",
           "escape_series", "apply"]

GEOMETRIES = ("sphere", "slab")


def D_of(x):
    """dln Gtilde / dln x of AKP10 Eq. D7, in the precision of x"""
    c2 = np.cbrt(x) ** 2
    c4 = c2 * c2
    rat = (1 - LD(3.4) * c2 / (1 + LD(3.4) * c2)
           + (LD(4.42) * c2 + LD(1.388) * c4) / (1 + LD(2.21) * c2 + LD(0.347) * c4)
           - (LD(2.706) * c2 + LD(0.868) * c4) / (1 + LD(1.353) * c2 + LD(0.217) * c4))
    return rat / 3 - x


def Q_of(x):
    """P (1 - D): H(x) = 2 Q(x) exp(-x)"""
    return P_of(x) * (1 - D_of(x))


def pref_of(B, E_eV):
    """2 pi^2 hbar^3 CS1 / (m_e E) [nE], cm^2 per unit of the sum (CS1 in 1/(s erg))"""
    E_erg = np.asarray(E_eV, dtype=LD) * _ERG
    pi = LD(4) * np.arctan(LD(1))
    cs1 = cs1_of(B, E_eV) / _ERG
    return 2 * pi ** 2 * _HBAR ** 3 * cs1 / (_ME * E_erg)


def row_terms(w, dlw, B, gam, lx, E_eV):
    """(term [nE][nG-1] before the prefactor, x [nE][nG], s^2 [nE][nG-1] of neighbouring Q) of
    one walker with a good field"""
    w, dlw, lx = np.asarray(w, dtype=LD), np.asarray(dlw, dtype=LD), np.asarray(lx, dtype=LD)
    g = np.asarray(gam, dtype=LD)
    x = x_of(B, gam, E_eV)
    with np.errstate(all="ignore"):
        Q = Q_of(x)
        u = np.where(x <= X_DEAD, (w / g)[None, :] * (Q * np.exp(-x)), LD(0))
        u1, u2 = u[:, :-1], u[:, 1:]
        Q1, Q2 = Q[:, :-1], Q[:, 1:]
        dl = (dlw[None, :-1] - lx[None, :]) + np.log1p((Q2 - Q1) / Q1) - (x[:, 1:] - x[:, :-1])
        ul = u1 * lx[None, :]
        safe = np.where((dl == 0) | np.isnan(dl), LD(1), dl)
        t = np.where(dl == 0, ul, ul * (np.expm1(safe) / safe))
        t = np.where(np.isnan(u1) | np.isnan(u2), LD(np.nan), t)
    t = np.where((u1 == 0) | (u2 == 0), LD(0), t)
    return t, x, ((Q2 - Q1) / (Q2 + Q1)) ** 2


def kappa(w, dlw, B, gam, lx, E_eV):
    """dict of [N][nE] arrays for walker rows w, dlw [N][nG] and fields B [N], as
    synchrotron_np.spectrum: kappa (cm^2), S = pref sum |term|, SX = pref sum |term| max(x_i,
    x_{i+1}), S_raw = sum |term|, pref, i0 (int), and s2 [3], the largest s^2 among the segments
    with a non-zero term in each range of syn_dlnP1's forms"""
    w, dlw = np.atleast_2d(w), np.atleast_2d(dlw)
    N, nG = w.shape
    nE = len(E_eV)
    out = {k: np.full((N, nE), LD(np.nan)) for k in ("kappa", "S", "SX", "S_raw", "pref")}
    out["i0"] = np.full((N, nE), nG, dtype=np.int64)
    out["s2"] = np.zeros(3)
    for r in range(N):
        if not (B[r] > 0 and np.isfinite(B[r])):
            continue
        t, x, s2 = row_terms(w[r], dlw[r], B[r], gam, lx, E_eV)
        pref = pref_of(B[r], E_eV)
        a = np.abs(t)
        s2 = s2[a > 0].astype(np.float64)
        for j, (lo, hi) in enumerate(((-1, 1e-4), (1e-4, 9e-4), (9e-4, np.inf))):
            m = s2[(s2 > lo) & (s2 <= hi)]
            out["s2"][j] = max(out["s2"][j], m.max() if m.size else 0.0)
        out["kappa"][r] = pref * t.sum(axis=1)
        out["S_raw"][r] = a.sum(axis=1)
        out["S"][r] = pref * out["S_raw"][r]
        out["SX"][r] = pref * (a * np.maximum(x[:, :-1], x[:, 1:])).sum(axis=1)
        out["pref"][r] = pref
        out["i0"][r] = first_live(x)
    return out


# ---- the escape fraction, mpmath at 50 digits ---------------------------------------------------
def _mp():
    mpmath.mp.dps = 50
    return mpmath.mp


def tau_of(kap, R, geometry):
    """tau (mpf) of float64 kappa [cm^2] and R [cm]"""
    mp = _mp()
    k, R = mp.mpf(float(kap)), mp.mpf(float(R))
    return 3 * k / (2 * mp.pi * R * R) if geometry == "sphere" else k / (mp.pi * R * R)


def escape(tau, geometry):
    """f(tau) (mpf) from the closed forms, evaluated with enough digits for tau >= 1e-15"""
    mp = _mp()
    tau = mp.mpf(tau)
    if tau == 0:
        return mp.mpf(1)
    with mp.workdps(120):
        e = mp.exp(-tau)
        if geometry == "sphere":
            f = 3 * (mp.mpf(1) / 2 + e / tau - (1 - e) / tau ** 2) / tau
        else:
            f = (1 - e) / tau
    return +f


def escape_series(tau, nterms):
    """the sphere's series, n = 2 .. nterms + 1"""
    mp = _mp()
    tau = mp.mpf(tau)
    return mp.fsum((-1) ** n * 3 * n * tau ** (n - 2) / mp.factorial(n + 1)
                   for n in range(2, nterms + 2))


def apply(kap, R, geometry, terms=None, colfac=None, write_tau=False):
    """the contract of nh_ssa_apply on float64 inputs, as an object array of mpf (NaN: float nan):
    kap [N][m] or [m] (a shared row), R [N], terms = [(scale, buf [N][m])], colfac [m]"""
    mp = _mp()
    R = np.asarray(R, dtype=float)
    kap = np.asarray(kap, dtype=float)
    N = R.size
    kap = np.broadcast_to(kap, (N, kap.shape[-1]))
    m = kap.shape[1]
    out = np.empty((N, m), dtype=object)
    for w in range(N):
        good = R[w] > 0 and np.isfinite(R[w])
        for k in range(m):
            if not good or np.isnan(kap[w, k]):
                out[w, k] = float("nan")
                continue
            tau = tau_of(kap[w, k], R[w], geometry)
            if write_tau:
                out[w, k] = tau
                continue
            s = mp.mpf(1)
            if terms:
                s = mp.fsum(mp.mpf(float(sc)) * mp.mpf(float(buf[w, k])) for sc, buf in terms)
            if colfac is not None:
                s *= mp.mpf(float(colfac[k]))
            out[w, k] = escape(tau, geometry) * s
    return out
