"""Host tests of tests/kelner_leptons_np.py, the reference the GPU tests hold
nh_pp_leptons_kelner06 to.  The reference project has no neutrino code, so the formulas are
pinned to the paper (Kelner, Aharonian & Bugayov 2006) by properties it states -- the decay
distributions are normalised and conserve energy, one electron and one direct muon neutrino per
charged pion, the lepton-to-gamma ratios of power laws -- and the quadrature by mpmath."""
import math

import numpy as np
import pytest
from numpy.testing import assert_allclose
from scipy.integrate import quad

import kelner_cases as KC
import kelner_leptons_np as KL
from oracle import naima_np as O


def _q(f, *ends):
    return math.fsum(quad(f, a, b, epsrel=1e-13, epsabs=0, limit=400)[0]
                     for a, b in zip(ends[:-1], ends[1:]))


# ---------------------------------------------------------------------------------------
# the decay distributions of the delta-functional branch
# ---------------------------------------------------------------------------------------
def test_decay_distributions_normalised_continuous_energy_conserving():
    """pi -> mu nu -> e nu nu for a relativistic pion: each lepton's f(x) integrates to 1, is
    continuous at r, and the four leptons carry the pion's energy between them: lambda/2
    (direct nu_mu) + <x>_e (electron) + <x>_e (nu_mu of the muon) + <x>_nue = 1"""
    r, lam = KL.R, KL.LAM
    mean = {}
    for name, f in (("e", KL.f_e), ("nue", KL.f_nue)):
        assert abs(_q(f, 0.0, r, 1.0) - 1.0) < 1e-13
        assert abs(f(r) - f(np.nextafter(r, 0))) < 1e-13
        assert abs(f(1.0)) < 1e-13 and f(0.5) > 0 and f(0.9) > 0
        mean[name] = _q(lambda x: x * f(x), 0.0, r, 1.0)
    assert abs(_q(KL.f_numu1, 0.0, lam) - 1.0) < 1e-13 and KL.f_numu1(lam) == 0.0
    assert abs(lam / 2 + 2 * mean["e"] + mean["nue"] - 1.0) < 1e-13
    assert_allclose(mean["e"], 0.2646, atol=5e-5)
    assert_allclose(mean["nue"], 0.2573, atol=5e-5)


# ---------------------------------------------------------------------------------------
# transcription pins of the F's (computed from KAB06 Eq. 58-69; 1e-5 is the printed precision)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, F, top, number, energy", [
    ("F_e", KL.F_e, 1.0, 3.64743, 0.0609425),
    ("F_numu1", KL.F_numu1, KL.LAM, 3.64248, 0.0497339),
    ("F_gamma", KL.F_gamma, 1.0, 7.44825, 0.166031)])
def test_F_pins_at_1TeV(name, F, top, number, energy):
    """int_{1e-3}^{1} F dx and int_0^1 x F dx at Ep = 1 TeV.  One electron and one direct muon
    neutrino per charged pion: the first two numbers are nearly equal"""
    assert_allclose(_q(lambda x: F(x, 1.0), 1e-3, 0.1, top), number, rtol=1e-5)
    assert_allclose(_q(lambda x: x * F(x, 1.0), 0.0, 1e-3, 0.1, top), energy, rtol=1e-5)


def test_F_e_regular_form_and_onset():
    """the form the kernel evaluates, B (1 + k t^2)^3 t^5 exp((1 - b) t) / (exp(-b t) + 0.3) at
    x = exp(-t), is Eq. 62; and F_e vanishes continuously towards Ep = 36.3 GeV, below which
    Eq. 64 has no value"""
    for Ep in (0.05, 1.0, 1e3):
        L = math.log(Ep)
        b = KL._beta_e_base(L) ** -0.25
        B = 1 / (69.5 + 2.65 * L + 0.3 * L * L)
        k = (0.279 + 0.141 * L + 0.0172 * L * L) / (0.3 + (2.3 + L) ** 2)
        for t in (1e-3, 0.3, 2.0, 9.0):
            v = B * (1 + k * t * t) ** 3 * t ** 5 * math.exp((1 - b) * t) / (math.exp(-b * t) + 0.3)
            assert_allclose(KL.F_e(math.exp(-t), Ep), v, rtol=1e-12)
    assert abs(KL._beta_e_base(KL.L_E_ZERO)) < 1e-15
    assert KL.F_e(0.3, KL.EP_E_ZERO_TEV * (1 - 1e-9)) == 0.0
    assert 0.0 <= KL.F_e(0.3, KL.EP_E_ZERO_TEV * (1 + 1e-9)) < 1e-100
    assert KL.F_e(0.3, 0.01) == 0.0


# ---------------------------------------------------------------------------------------
# pure power laws at 1 TeV, full branch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha, e_g, numu_g", [(2.0, 0.42443, 0.74802), (2.5, 0.33315, 0.55332),
                                                (3.0, 0.26487, 0.41219)])
def test_power_law_ratios_to_gamma(alpha, e_g, numu_g):
    def J(Ep):
        return Ep ** -alpha
    kinks = O.k06_kinks((0.1,))
    gam, nhat = O.k06_spectrum([1e12], J, Etrans_TeV=0.1, epsrel=1e-11, breaks_TeV=(0.1,))
    gam = gam[0] * 1e12
    e = KL.integral(J, kinks, 1.0, True, "e")
    m = KL.integral(J, kinks, 1.0, True, "numu1")
    assert_allclose(e / gam, e_g, rtol=1e-4)
    assert_allclose((e + m) / gam, numu_g, rtol=1e-4)


# ---------------------------------------------------------------------------------------
# the reference's integrals against mpmath (30 digits, tanh-sinh, in x, untransformed formulas)
# ---------------------------------------------------------------------------------------
def _mp_leptons(tag):
    import mpmath as mp
    kind, par = KC._find(tag)
    p = {k: mp.mpf(float(v)) for k, v in dict(par, amplitude=KC.AMP, e_0=KC.E0).items()}
    KPI, MP_, MPI, ETH = (mp.mpf(v) for v in (O.K06_KPI, O.K06_MP_TEV, O.K06_MPI_TEV,
                                              O.K06_ETH_TEV))
    R, LAM = mp.mpf(KL.R), mp.mpf(KL.LAM)
    kinks = [mp.mpf(b) for b in KL._kinks_TeV(tag)]
    m = mp.mpf

    def J(Et):
        E = Et * m(1e12)
        x = E / p["e_0"]
        if "e_break" not in p:
            v = x ** -p["alpha"]
        elif E < p["e_break"]:
            v = x ** -p["alpha_1"]
        else:
            v = (p["e_break"] / p["e_0"]) ** (p["alpha_2"] - p["alpha_1"]) * x ** -p["alpha_2"]
        return p["amplitude"] * v * m(1e12)

    def sigma(Ep):
        L = mp.log(Ep)
        s = m("34.3") + m("1.88") * L + m("0.25") * L ** 2
        if Ep <= m(0.1):
            s *= (1 - (ETH / Ep) ** 4) ** 2 * (0 if Ep < ETH else 1)
        return s * m("1e-27")

    def base_e(L):
        return m("0.201") + m("0.062") * L + m("0.00042") * L ** 2

    def Fe(x, Ep):
        L = mp.log(Ep)
        if base_e(L) <= 0:
            return m(0)
        B = 1 / (m("69.5") + m("2.65") * L + m("0.3") * L ** 2)
        beta = base_e(L) ** m("-0.25")
        k = (m("0.279") + m("0.141") * L + m("0.0172") * L ** 2) / (m("0.3") + (m("2.3") + L) ** 2)
        return (B * (1 + k * mp.log(x) ** 2) ** 3 / (x * (1 + m("0.3") / x ** beta))
                * (-mp.log(x)) ** 5)

    def Fmu(x, Ep):
        y = x / LAM
        if y >= 1:
            return m(0)
        L = mp.log(Ep)
        B = m("1.75") + m("0.204") * L + m("0.010") * L ** 2
        beta = 1 / (m("1.67") + m("0.111") * L + m("0.0038") * L ** 2)
        k = m("1.07") - m("0.086") * L + m("0.002") * L ** 2
        yb = y ** beta
        return (B * mp.log(y) / y * ((1 - yb) / (1 + k * yb * (1 - yb))) ** 4
                * (1 / mp.log(y) - 4 * beta * yb / (1 - yb)
                   - 4 * k * beta * yb * (1 - 2 * yb) / (1 + k * yb * (1 - yb))))

    def fe(x):
        c = (3 - 2 * R) / (9 * (1 - R) ** 2)

        def g(z):
            return c * (9 * z ** 2 - 6 * mp.log(z) - 4 * z ** 3 - 5)
        if x >= R:
            return g(x)
        return g(R) + (1 + 2 * R) * (R - x) / (9 * R ** 2) * (9 * (R + x)
                                                              - 4 * (R ** 2 + R * x + x ** 2))

    def fnue(x):
        c = 2 / (3 * (1 - R) ** 2)
        if x >= R:
            return c * ((1 - x) * (6 * (1 - x) ** 2 + R * (5 + 5 * x - 4 * x ** 2))
                        + 6 * R * mp.log(x))
        he1 = c * ((1 - R) * (6 - 7 * R + 11 * R ** 2 - 4 * R ** 3) + 6 * R * mp.log(R))
        return he1 + 2 * (R - x) / (3 * R ** 2) * (7 * R ** 2 - 4 * R ** 3 + 7 * x * R
                                                   - 4 * x * R ** 2 - 2 * x ** 2 - 4 * x ** 2 * R)

    def fmu(x):
        return 1 / LAM if x < LAM else m(0)

    def done(v, err, scale):
        return float(scale * v), float(err / abs(v))

    def full(E, comp):
        E = m(E)
        F, top = (Fmu, LAM) if comp == "numu1" else (Fe, m(1))
        onset = [] if comp == "numu1" else [m(KL.EP_E_ZERO_TEV)]

        def f(x):
            if x == top:
                return m(0)
            with mp.workdps(2 * mp.mp.dps + 10):  # F_numu1 cancels towards y = 1
                v = sigma(E / x) * J(E / x) * F(x, E / x) / x
            return +v
        ends = sorted(set([m(0), top] + [E / b for b in kinks + onset if E / b < top]))
        return done(*mp.quad(f, ends, error=True), O.C_CGS * 1e-12)

    def delta(E, comp):
        E = m(E)
        fx = {"e": fe, "nue": fnue, "numu1": fmu}[comp]
        top = min(m(1), E / MPI)  # E_pi = E / x >= m_pi
        if comp == "numu1":
            top = min(top, LAM)

        def f(x):
            Ep0 = MP_ + E / x / KPI
            return fx(x) * sigma(Ep0) * J(Ep0) / x
        mids = [R] + [E / ((b - MP_) * KPI) for b in kinks if b > MP_]
        ends = sorted(set([m(0), top] + [x for x in mids if x < top]))
        return done(*mp.quad(f, ends, error=True), 2 * O.C_CGS / O.K06_KPI * 1e-12)

    return mp, full, delta


@pytest.mark.parametrize("tag, Etrans, below, above", [("pl", 1e11, 5e7, 1e12),
                                                       ("bpl_below", 1e10, 1e9, 3e13)])
def test_reference_is_converged(tag, Etrans, below, above):
    """a power law and a broken one, an energy on each side of Etrans and Etrans itself (both
    branches: what nhat is made of), all three components: quad at 1e-11, at 1e-13 and mpmath
    agree to 1e-10.  5e7 eV lies below m_pi (the clamp), and the full branch at 1e10 eV crosses
    F_e's onset at Ep = 36.3 GeV"""
    mp, full, delta = _mp_leptons(tag)
    with mp.workdps(30):
        for is_full, E in ((False, below), (False, Etrans), (True, Etrans), (True, above)):
            for comp in (("e", "numu1") if is_full else KL.COMPONENTS):
                q11 = KL.branch(tag, E, is_full, comp)
                q13 = KL.branch(tag, E, is_full, comp, epsrel=1e-13)
                v, verr = (full if is_full else delta)(E * 1e-12, comp)
                print("%s %s %-5s %.0e eV: quad 1e-11 / 1e-13 - 1 = %.1e, / mpmath - 1 = %.1e "
                      "(mpmath's error estimate %.1e)"
                      % (tag, "full" if is_full else "delta", comp, E, q11 / q13 - 1, q11 / v - 1,
                         verr))
                assert verr < 1e-12
                assert_allclose(q11, q13, rtol=1e-10)
                assert_allclose(q11, v, rtol=1e-10)


def test_spectrum_composition():
    """spectrum() puts the products together from the components: matched on the low side
    whenever an energy lies there, nu_e = e on the high side, nhat = 1 with none below"""
    E = np.array([1e9, 1e12])
    n = KL.nhat("pl", 1e11)
    for prod, comps in KL.PRODUCTS.items():
        spec, nh = KL.spectrum("pl", E, 1e11, prod)
        assert_allclose(nh, n, rtol=0)
        lo = sum(KL.branch("pl", 1e9, False, c) * n[KL.COMPONENTS.index(c)] for c in comps)
        hi = sum(KL.branch("pl", 1e12, True, c) for c in comps)
        assert_allclose(spec, [lo, hi], rtol=1e-15)
        assert_allclose(KL.spectrum("pl", E[:1], 1e11, prod)[0], spec[:1], rtol=0)  # one-sided
        assert_allclose(KL.spectrum("pl", E[1:], 1e11, prod)[1], 1.0, rtol=0)
    assert KL.branch("pl", 1e12, True, "nue") == KL.branch("pl", 1e12, True, "e")
