"""Shared by test_oracle.py (host) and test_gpu_kelner.py: the particle distributions, photon
energies and transition energies at which PionDecayKelner06 is compared with the converged
reference, and that reference itself -- oracle.k06_spectrum / k06_Wp with every integral split
at the integrand's kinks (tests/test_oracle.py certifies it against mpmath)."""
import functools

import numpy as np

from oracle import naima_np as O

AMP, E0 = 4e35, 1e12  # 1/eV, eV
M_PI_EV = O.K06_MPI_TEV * 1e12
# a break that fell on a panel edge of the fixed-grid rule for E_gamma = 1 TeV (h = 0.5)
E_EDGE = 1e12 * np.exp(0.5 * 3)
_BREAKS = (("above", 3.7e12, 1.8, 2.9), ("below", 2e10, 2.0, 2.6), ("edge", E_EDGE, 1.8, 2.9))

# kind -> [(tag, oracle parameters)]; one launch per kind, one walker per entry
SETS = {
    "PowerLaw": [("pl", dict(alpha=2.2))],
    "ExponentialCutoffPowerLaw": [
        ("ecpl_b0.5", dict(alpha=2.0, e_cutoff=1e14, beta=0.5)),
        ("ecpl_b2.5", dict(alpha=2.0, e_cutoff=1e14, beta=2.5))],
    "LogParabola": [("lp", dict(alpha=2.1, beta=0.25))],
    "BrokenPowerLaw": [("bpl_" + t, dict(e_break=eb, alpha_1=a1, alpha_2=a2))
                       for t, eb, a1, a2 in _BREAKS],
    "ExponentialCutoffBrokenPowerLaw": [
        ("ecbpl_" + t, dict(e_break=eb, alpha_1=a1, alpha_2=a2, e_cutoff=1e14, beta=1.0))
        for t, eb, a1, a2 in _BREAKS],
}
ETRANS_EV = (1e10, 1e11, 1e12)


def energies(Etrans_eV):
    """1 MeV, m_pi/2 exactly, 1 and 50 GeV, the two sides of Etrans, 1, 30 and 300 TeV"""
    below = np.nextafter(Etrans_eV, 0)
    assert below * 1e-12 < Etrans_eV * 1e-12  # still apart in TeV, where the branch is chosen
    return np.unique([1e6, M_PI_EV / 2, 1e9, 5e10, below, Etrans_eV, 1e12, 3e13, 3e14])


def oracle_pd(kind, par):
    return O.ParticleDist(kind, amplitude=AMP, e_0=E0, **par)


def amd_pd(na, kind, pars, amplitude=AMP):
    """the naima_amd distribution whose walkers are the parameter sets ``pars`` of one kind"""
    u = na.u

    def col(name, unit=None):
        v = np.array([p[name] for p in pars])
        v = v[0] if v.size == 1 else v
        return v * unit if unit is not None else v
    A, e0 = amplitude / u.eV, E0 * u.eV
    if kind == "PowerLaw":
        return na.PowerLaw(A, e0, col("alpha"))
    if kind == "ExponentialCutoffPowerLaw":
        return na.ExponentialCutoffPowerLaw(A, e0, col("alpha"), col("e_cutoff", u.eV), col("beta"))
    if kind == "LogParabola":
        return na.LogParabola(A, e0, col("alpha"), col("beta"))
    if kind == "BrokenPowerLaw":
        return na.BrokenPowerLaw(A, e0, col("e_break", u.eV), col("alpha_1"), col("alpha_2"))
    return na.ExponentialCutoffBrokenPowerLaw(A, e0, col("e_break", u.eV), col("alpha_1"),
                                              col("alpha_2"), col("e_cutoff", u.eV), col("beta"))


def breaks_TeV(par):
    """a smooth distribution's integrals are still split at the cross section's own kinks"""
    return (par["e_break"] * 1e-12,) if "e_break" in par else (O.K06_SIGMA_SWITCH_TEV,)


def _find(tag):
    for kind, sets in SETS.items():
        for t, par in sets:
            if t == tag:
                return kind, par
    raise KeyError(tag)


def J_per_TeV(tag):
    pd = oracle_pd(*_find(tag))
    return lambda Et: float(pd(Et * 1e12)) * 1e12


@functools.lru_cache(maxsize=None)
def branch(tag, E_eV, full, epsrel=1e-11):
    """one converged integral, 1/(s eV) for nh = 1: the full calculation (``full``) or the
    delta-functional approximation with nhat = 1, whatever side of Etrans E_eV lies on.
    (k06_spectrum with a single energy never mixes branches; Etrans chooses the one.)"""
    Etr = E_eV * 1e-12 if full else np.inf
    spec, nhat = O.k06_spectrum([E_eV], J_per_TeV(tag), Etrans_TeV=Etr, epsrel=epsrel,
                                breaks_TeV=breaks_TeV(_find(tag)[1]))
    assert nhat == 1.0
    return float(spec[0])


def spectrum(tag, E_eV, Etrans_eV):
    """what k06_spectrum(E_eV, ..., Etrans) returns, put together from cached integrals
    (test_oracle.py checks that it is the same): (spec [1/(s eV)] for nh = 1, nhat)"""
    E_eV = np.atleast_1d(np.asarray(E_eV, dtype=float))
    hi = E_eV * 1e-12 >= Etrans_eV * 1e-12
    nhat = 1.0
    if hi.any() and not hi.all():
        nhat = branch(tag, Etrans_eV, True) / branch(tag, Etrans_eV, False)
    return np.array([branch(tag, e, True) if h else branch(tag, e, False) * nhat
                     for e, h in zip(E_eV, hi)]), nhat


@functools.lru_cache(maxsize=None)
def Wp_TeV(tag, epsrel=1e-11):
    return O.k06_Wp(J_per_TeV(tag), breaks_TeV(_find(tag)[1]), epsrel=epsrel)
