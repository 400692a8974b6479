"""Shared by test_kelner_leptons_host.py and test_gpu_kelner_leptons.py (not a test): a NumPy /
SciPy restatement of the secondary-lepton spectra of Kelner, Aharonian & Bugayov 2006 (KAB06) --
the electrons and neutrinos of pp -> pi+- -> mu nu -> e nu nu -- as SecondaryLeptonsKelner06
computes them, with adaptive ``quad`` (epsrel 1e-11) split at every kink of the integrand.

The cross section, the particle distributions and the constants are the oracle's
(oracle.naima_np); the parameter sets are those of kelner_cases.  The reference project has no
counterpart of these spectra, so the formulas are pinned to KAB06 by the host tests instead
(normalisation and energy conservation of the decay distributions, integrals of F at 1 TeV,
lepton-to-gamma ratios of pure power laws) and this module's integrals by mpmath.

Components: "e" (e+ + e-; also the muon neutrino of the muon decay), "nue", "numu1" (the muon
neutrino of the pion decay).  Above Etrans "nue" is "e" (KAB06: F_nue ~= F_e).
"""
import functools
import math

import numpy as np

import kelner_cases as KC
from oracle import naima_np as O

R = 0.573    # 1 - lambda = (m_mu / m_pi)^2
LAM = 0.427  # the largest share of the pion's energy the direct neutrino can take
T_R, T_LAM = -math.log(R), -math.log(LAM)
T_MAX = 600.0  # quad's map of an infinite range reaches t where exp(t) overflows: nothing is left
COMPONENTS = ("e", "nue", "numu1")
# product -> the components it sums
PRODUCTS = {"electron": ("e",), "nu_e": ("nue",), "nu_mu": ("e", "numu1"),
            "nu_all": ("e", "nue", "numu1")}


# ---------------------------------------------------------------------------------------
# full calculation: F(x, Ep), per unit x, Ep in TeV
# ---------------------------------------------------------------------------------------
def _beta_e_base(L):
    return 0.201 + 0.062 * L + 0.00042 * L ** 2


# below this proton energy [TeV] (36 GeV) Eq. 64's beta_e does not exist: its base is negative.
# beta_e -> inf as the base -> 0+, and F_e -> 0 with it, so F_e = 0 below is the continuation
L_E_ZERO = (-0.062 + math.sqrt(0.062 ** 2 - 4 * 0.00042 * 0.201)) / (2 * 0.00042)
EP_E_ZERO_TEV = math.exp(L_E_ZERO)


def F_e(x, Ep):
    """KAB06 Eq. 62-65: electrons, nu_mu of the muon decay, and (approximately) nu_e"""
    L = math.log(Ep)
    base = _beta_e_base(L)
    if not base > 0.0:
        return 0.0
    B = 1.0 / (69.5 + 2.65 * L + 0.3 * L ** 2)
    beta = base ** -0.25
    k = (0.279 + 0.141 * L + 0.0172 * L ** 2) / (0.3 + (2.3 + L) ** 2)
    lx = math.log(x)
    return B * (1 + k * lx ** 2) ** 3 / (x * (1 + 0.3 / x ** beta)) * (-lx) ** 5


def F_numu1(x, Ep):
    """KAB06 Eq. 66-69: the muon neutrino of pi -> mu nu"""
    y = x / LAM
    if y >= 1.0:
        return 0.0
    L = math.log(Ep)
    B = 1.75 + 0.204 * L + 0.010 * L ** 2
    beta = 1.0 / (1.67 + 0.111 * L + 0.0038 * L ** 2)
    k = 1.07 - 0.086 * L + 0.002 * L ** 2
    yb = y ** beta
    ly = math.log(y)
    return (B * ly / y * ((1 - yb) / (1 + k * yb * (1 - yb))) ** 4
            * (1 / ly - 4 * beta * yb / (1 - yb)
               - 4 * k * beta * yb * (1 - 2 * yb) / (1 + k * yb * (1 - yb))))


def F_gamma(x, Ep):
    return float(O.k06_Fgamma(x, Ep))


F_OF = {"e": F_e, "nue": F_e, "numu1": F_numu1}


# ---------------------------------------------------------------------------------------
# delta-functional branch: the decay distributions f(x), x = E / E_pi, relativistic pion
# ---------------------------------------------------------------------------------------
def f_numu1(x):
    return 1.0 / LAM if x < LAM else 0.0


def f_e(x, r=R):
    """electrons and the muon neutrino of mu -> e nu nu (KAB06 section IV)"""
    c = (3 - 2 * r) / (9 * (1 - r) ** 2)
    if x >= r:
        return c * (9 * x ** 2 - 6 * math.log(x) - 4 * x ** 3 - 5)
    h1 = c * (9 * r ** 2 - 6 * math.log(r) - 4 * r ** 3 - 5)
    h2 = (1 + 2 * r) * (r - x) / (9 * r ** 2) * (9 * (r + x) - 4 * (r ** 2 + r * x + x ** 2))
    return h1 + h2


def f_nue(x, r=R):
    """the electron neutrino of mu -> e nu nu (KAB06 section IV)"""
    c = 2 / (3 * (1 - r) ** 2)
    if x >= r:
        return c * ((1 - x) * (6 * (1 - x) ** 2 + r * (5 + 5 * x - 4 * x ** 2))
                    + 6 * r * math.log(x))
    he1 = c * ((1 - r) * (6 - 7 * r + 11 * r ** 2 - 4 * r ** 3) + 6 * r * math.log(r))
    he2 = (2 * (r - x) / (3 * r ** 2)
           * (7 * r ** 2 - 4 * r ** 3 + 7 * x * r - 4 * x * r ** 2 - 2 * x ** 2 - 4 * x ** 2 * r))
    return he1 + he2


f_OF = {"e": f_e, "nue": f_nue, "numu1": f_numu1}


# ---------------------------------------------------------------------------------------
# the integrals, in t = -ln x (dx / x = dt), one quad per stretch between two kinks
# ---------------------------------------------------------------------------------------
def _kinks_TeV(tag):
    return O.k06_kinks(KC.breaks_TeV(KC._find(tag)[1]))


def _pieces(f, t0, mids, epsrel):
    ends = [t0] + sorted(t for t in set(mids) if t > t0 + 1e-12) + [np.inf]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return O._k06_quad_pieces(f, ends, epsrel)


def full_ends(kinks_TeV, E_TeV, comp):
    """(start, kinks) in t of the full branch: Ep = E exp(t)"""
    mids = [math.log(b / E_TeV) for b in kinks_TeV if b > E_TeV]
    if comp == "numu1":
        return T_LAM, mids
    if EP_E_ZERO_TEV > E_TeV:
        mids.append(math.log(EP_E_ZERO_TEV / E_TeV))
    return 0.0, mids


def delta_ends(kinks_TeV, E_TeV, comp):
    """(start, kinks) in t of the delta-functional branch: E_pi = E exp(t) >= m_pi"""
    t0 = max(0.0, math.log(O.K06_MPI_TEV / E_TeV))
    mids = [math.log(epi / E_TeV) for epi in ((b - O.K06_MP_TEV) * O.K06_KPI for b in kinks_TeV)
            if epi > E_TeV]
    if comp == "numu1":
        return max(t0, T_LAM), mids
    return t0, mids + [T_R]


def integral(J, kinks_TeV, E_TeV, full, comp, epsrel=1e-11):
    """component ``comp`` at E_TeV, 1/(s TeV) for nh = 1, of protons ``J(Ep_TeV)`` [1/TeV] whose
    kinks (with the cross section's) are ``kinks_TeV``: the full calculation (``full``) or the
    delta-functional approximation with nhat = 1"""
    E = E_TeV
    if full:
        F = F_OF[comp]

        def f(t):
            if t > T_MAX:
                return 0.0
            Ep = E * math.exp(t)
            return O.k06_sigma_inel(Ep) * J(Ep) * F(math.exp(-t), Ep)
        t0, mids = full_ends(kinks_TeV, E, comp)
        return O.C_CGS * _pieces(f, t0, mids, epsrel)
    fx = f_OF[comp]

    def f(t):
        if t > T_MAX:
            return 0.0
        Ep0 = O.K06_MP_TEV + E * math.exp(t) / O.K06_KPI
        return fx(math.exp(-t)) * O.k06_sigma_inel(Ep0) * J(Ep0)
    t0, mids = delta_ends(kinks_TeV, E, comp)
    return 2 * O.C_CGS / O.K06_KPI * _pieces(f, t0, mids, epsrel)


@functools.lru_cache(maxsize=None)
def branch(tag, E_eV, full, comp, epsrel=1e-11):
    """one converged integral of a kelner_cases parameter set, 1/(s eV) for nh = 1, whatever
    side of Etrans E_eV lies on"""
    return integral(KC.J_per_TeV(tag), _kinks_TeV(tag), E_eV * 1e-12, full, comp, epsrel) * 1e-12


def nhat(tag, Etrans_eV):
    """the three matching factors (e, nue, numu1): full / delta at Etrans; nue meets F_e"""
    return np.array([branch(tag, Etrans_eV, True, c) / branch(tag, Etrans_eV, False, c)
                     for c in COMPONENTS])


def spectrum(tag, E_eV, Etrans_eV, product):
    """(spec [1/(s eV)] for nh = 1, nhat[3]).  The delta branch is matched whenever an energy
    lies below Etrans, also when none lies above it (unlike PionDecayKelner06)."""
    E_eV = np.atleast_1d(np.asarray(E_eV, dtype=float))
    hi = E_eV * 1e-12 >= Etrans_eV * 1e-12
    nh = np.ones(3) if hi.all() else nhat(tag, Etrans_eV)
    spec = np.zeros(E_eV.size)
    for c in PRODUCTS[product]:
        n = nh[COMPONENTS.index(c)]
        spec += [branch(tag, e, True, c) if h else branch(tag, e, False, c) * n
                 for e, h in zip(E_eV, hi)]
    return spec, nh
