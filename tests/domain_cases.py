"""Shared by test_domain_host.py (host) and test_gpu_domain.py: scalars OUTSIDE their physical
domain -- the synchrotron field B, a thermal seed's T, u and theta, the target densities n0 / nh
and the grid limits Eemin / Eemax / nEed (Epmin / Epmax / nEpd) -- each as a batch of 8 walkers
that holds legal values beside the illegal ones (walker 0 and the last walker are always legal),
and what oracle/naima_np.py, which follows the reference's arithmetic line by line, gives for
every walker: a finite row, a row with non-finite elements, or the exception the reference's
int() of the node count raises (radiative.py:152-154, 1002-1009).

A case is (id, class, the scalar, its 8 values, everything else).  Everything else is fixed and
small: ECPL particles (index 2.3, cut-off 30 TeV, beta 1), a particle grid of 1 GeV .. 100 TeV
at 20 nodes per decade (100 nodes), 7 photon energies from 1 GeV to 10 TeV (energies(): off the
grid's nodes for bremsstrahlung; 6 from 1 meV to 100 keV for synchrotron), and 70 energies over the same ranges -- one full tile of 64 and a
ragged one -- for the kernels that tile energies.  Units: energies of electrons and photons in
eV, of protons in GeV, B in G, T in K, u in eV/cm3, theta in rad, densities in 1/cm3."""
import functools
import warnings

import numpy as np

from oracle import naima_np as O

AMP, E0, ALPHA, ECUT, BETA = 1e36, 1e12, 2.3, 3e13, 1.0  # 1/eV, eV, -, eV, -
NW = 8
SIZES = ("small", "tiles")


def energies(cls, size):
    # Bremsstrahlung: 1 GeV .. 10 TeV drawn in by 2 %.  A photon energy equal to a grid node's
    # (1 GeV is the first node's, 10**(20/6) GeV the 67th's) sits on the step of the
    # bremsstrahlung cross sections (g < eps, radiative.py:838-871), and the last bit of 10**x
    # decides the comparison: the general kernel, whose nodes are the device's exp10, and
    # np.logspace fell on different sides of it, 1.1 % of the spectrum at that energy
    lo, hi, n = {"Synchrotron": (1e-3, 1e5, 6), "Bremsstrahlung": (1.02e9, 0.98e13, 7)}.get(
        cls, (1e9, 1e13, 7))
    return np.geomspace(lo, hi, n if size == "small" else 70)


# every scalar of a class at its legal value
DEFAULTS = {
    "Synchrotron": dict(B=1e-5, Eemin=1e9, Eemax=1e14, nEed=20),
    "InverseCompton": dict(T=30.0, u=0.5, theta=0.7, Eemin=1e9, Eemax=1e14, nEed=20),
    "Bremsstrahlung": dict(n0=1.0, Eemin=1e9, Eemax=1e14, nEed=20),
    "PionDecay": dict(nh=1.0, Epmin=2.0, Epmax=1e5, nEpd=20),
}
# the scalars that shape a grid or a kernel: given per walker they go through the general kernels
STRUCTURAL = ("Eemin", "Eemax", "nEed", "Epmin", "Epmax", "nEpd", "T", "theta")
# the reference's constructor refuses these as a plain scalar below 0 (validate_scalar with
# domain="positive", radiative.py:486-501 and validator.py:33-35): ValueError, where a value per
# walker only meets the arithmetic
REFUSED_NEGATIVE = ("T", "u")

TWO_PI = 2 * np.pi
_LIMITS_LO = [1e9, 2e14, 1e14, -1e9, 0.0, 3e10, 5e14, 3e9]    # inverted, equal, negative, 0, ...
_LIMITS_HI = [1e14, 1e8, 1e9, -1e13, 0.0, 1e13, 1e6, 3e14]
_DENS = [20, -5, 0.3, 0, 7.5, 33, -0.0, 12]
_TARGET = [1.0, -1.0, 0.0, 3.0, -2.5e-3, 1e3, -0.0, 0.3]
# (1 - cos(1e-8) is 0 in double: a legal angle whose row is NaN, as theta = 0's)
_THETA = [0.7, -0.7, 0.0, 1e-8, np.pi, -3.0, 4.0, TWO_PI - 0.7]
_LEGAL_THETA = [True, False, False, False, True, False, True, True]
_LEGAL_LIMITS = [True, False, False, False, False, True, False, True]
_LEGAL_DENS = [True, False, False, False, True, True, False, True]
_LEGAL_TARGET = [True, False, False, True, False, True, False, True]

# (id, class, scalar, values, legal walkers, everything else: scalars ALSO given per walker (at
#  their legal value) so that the case takes the general kernel)
CASES = [
    ("syn-B", "Synchrotron", "B", [1e-5, -1e-5, 0.0, 1e-30, 3e-6, -3e-4, 1e-3, 2e-5],
     [True, False, False, True, True, False, True, True], ()),
    ("syn-B-general", "Synchrotron", "B", [1e-5, -1e-5, 0.0, 1e-30, 3e-6, -3e-4, 1e-3, 2e-5],
     [True, False, False, True, True, False, True, True], ("Eemin",)),
    ("syn-Eemin", "Synchrotron", "Eemin", _LIMITS_LO, _LEGAL_LIMITS, ()),
    ("syn-Eemax", "Synchrotron", "Eemax", _LIMITS_HI, _LEGAL_LIMITS, ()),
    ("syn-nEed", "Synchrotron", "nEed", _DENS, _LEGAL_DENS, ()),
    ("ic-theta", "InverseCompton", "theta", _THETA, _LEGAL_THETA, ()),
    ("ic-theta-general", "InverseCompton", "theta", _THETA, _LEGAL_THETA, ("Eemin",)),
    ("ic-T", "InverseCompton", "T", [30.0, -30.0, 1e-30, 3e4, 0.0, 3e3, -1e-30, 2.7],
     [True, False, True, True, False, True, False, True], ()),
    ("ic-u", "InverseCompton", "u", [0.5, -0.5, 0.0, 2.0, -1e-3, 1e3, -0.0, 1.0],
     [True, False, False, True, False, True, False, True], ()),
    ("ic-Eemin", "InverseCompton", "Eemin", _LIMITS_LO, _LEGAL_LIMITS, ()),
    ("ic-Eemax", "InverseCompton", "Eemax", _LIMITS_HI, _LEGAL_LIMITS, ()),
    ("ic-nEed", "InverseCompton", "nEed", _DENS, _LEGAL_DENS, ()),
    ("br-n0", "Bremsstrahlung", "n0", _TARGET, _LEGAL_TARGET, ()),
    ("br-n0-general", "Bremsstrahlung", "n0", _TARGET, _LEGAL_TARGET, ("Eemin",)),
    ("br-Eemin", "Bremsstrahlung", "Eemin", _LIMITS_LO, _LEGAL_LIMITS, ()),
    ("br-Eemax", "Bremsstrahlung", "Eemax", _LIMITS_HI, _LEGAL_LIMITS, ()),
    ("br-nEed", "Bremsstrahlung", "nEed", _DENS, _LEGAL_DENS, ()),
    ("pp-nh", "PionDecay", "nh", _TARGET, _LEGAL_TARGET, ()),
    ("pp-nh-general", "PionDecay", "nh", _TARGET, _LEGAL_TARGET, ("Epmin",)),
    # (0.5 GeV: below the pion threshold m_p + T_th = 1.218 GeV, and below the proton's rest mass)
    ("pp-Epmin", "PionDecay", "Epmin", [2.0, 2e5, 1e5, -2.0, 0.0, 0.5, 1.0, 30.0],
     [True, False, False, False, False, False, False, True], ()),
    ("pp-Epmax", "PionDecay", "Epmax", [1e5, 1.0, 2.0, -1e5, 0.0, 1e4, 0.5, 3e5],
     [True, False, False, False, False, True, False, True], ()),
    ("pp-nEpd", "PionDecay", "nEpd", _DENS, _LEGAL_DENS, ()),
]
IDS = [c[0] for c in CASES]

# a span whose node count exceeds Context.general_nmax = 2048: the status path's own case, the
# whole batch is refused (20 nodes per decade over 3e-120 eV .. 100 TeV: int(2670.46) nodes)
TOO_LONG = ("syn-too-long", "Synchrotron", "Eemin", [1e9, 3e-120, 3e9, 1e10, 1e9, 3e10, 1e11, 3e9])

# what the oracle's rows have to be, per scalar (test_domain_host.py holds the table to it):
#   "unphysical"  a value outside the domain whose row is entirely finite
#   "nonfinite"   a row that is entirely non-finite ("mixed": only some of its elements)
#   "raises"      the reference's int() of the node count raises
# The reference raises only there, so only a grid limit can; a negative B or T has no entirely
# finite row at these energies (B = -0.3 mG keeps its lowest energies finite: exp(|x|) has not
# overflowed there), and no target density or seed energy density makes a non-finite one.  A
# proton grid that starts below the pion threshold is NaN: the kinetic energy goes negative.
OUTCOMES = {
    "B": {"nonfinite", "mixed"}, "T": {"nonfinite"}, "theta": {"unphysical", "nonfinite"},
    "u": {"unphysical"}, "n0": {"unphysical"}, "nh": {"unphysical"},
    "Eemin": {"unphysical", "raises"}, "Eemax": {"unphysical", "raises"},
    "Epmin": {"unphysical", "nonfinite", "raises"}, "Epmax": {"unphysical", "nonfinite", "raises"},
    "nEed": {"unphysical"}, "nEpd": {"unphysical"},
}


def particle_distribution():
    return O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=AMP, e_0=E0, alpha=ALPHA,
                          e_cutoff=ECUT, beta=BETA)


def seeds(par):
    """the CMB and one anisotropic star-like field: the scalars under test are the second seed's"""
    return [O.thermal_seed("CMB"),
            dict(type="thermal", T=par["T"], u=par["u"] * O.ERG_PER_EV, theta=par["theta"])]


def walker(cls, par, E):
    """the oracle for one walker with the scalars ``par``: dict(flux [1/(s eV)], W [erg], Wc [erg]:
    compute_We / compute_Wp between the limits, and for InverseCompton seed: the second seed's flux) -- or the exception of the reference's int()"""
    pd = particle_distribution()
    par = {k: np.float64(v) for k, v in par.items()}  # (the reference's scalars are arrays)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if cls == "PionDecay":
            Ep = O.proton_grid(par["Epmin"], par["Epmax"], par["nEpd"])
            J = O.J_on(pd, Ep)
            # (compute_Wp counts its nodes from the difference of the logarithms, Wp and the
            # spectrum from the logarithm of the ratio: radiative.py:1047-1053, 1002-1009)
            Ec = O.log_grid(par["Epmin"], par["Epmax"], par["nEpd"])
            return dict(flux=O.pion_spectrum(E, Ep, J, par["nh"]),
                        W=O.proton_energy_content(pd, Ep), Wc=O.proton_energy_content(pd, Ec))
        g = O.electron_grid(par["Eemin"], par["Eemax"], par["nEed"])
        ne = O.nelec_on(pd, g)
        out = dict(W=O.electron_energy_content(pd, g))
        out["Wc"] = out["W"]  # (compute_We with the limits as the call's arguments: the same grid)
        if cls == "Synchrotron":
            out["flux"] = O.synchrotron_spectrum(E, g, ne, par["B"])
        elif cls == "Bremsstrahlung":
            out["flux"] = O.brems_spectrum(E, g, ne, n0=par["n0"])
        else:
            tot, per = O.ic_spectrum(E, g, ne, seeds(par))
            out["flux"], out["seed"] = tot, per[1]
        return out


@functools.lru_cache(maxsize=None)
def expected(cid, size):
    """the oracle on every walker of case ``cid``: a list of dicts (walker) or exception types,
    computed once and shared; the arrays are read-only"""
    _, cls, name, values, _, _ = CASES[IDS.index(cid)]
    E = energies(cls, size)
    rows = []
    for v in values:
        par = dict(DEFAULTS[cls])
        par[name] = v
        try:
            r = walker(cls, par, E)
        except (ValueError, OverflowError) as exc:
            rows.append(type(exc))
            continue
        for a in r.values():
            np.asarray(a).setflags(write=False)
        rows.append(r)
    return rows


def outcome(row, legal):
    """"raises" | "nonfinite" | "mixed" | "unphysical" | "legal" for one walker's oracle row"""
    if isinstance(row, type):
        return "raises"
    fin = np.isfinite(row["flux"])
    if not fin.any():
        return "nonfinite"
    if not fin.all():
        return "mixed"
    return "legal" if legal else "unphysical"
