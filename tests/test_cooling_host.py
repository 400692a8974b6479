"""Host tests of tests/cooling_np.py, the NumPy restatement that the GPU tests hold
nh_cooled_electrons to: against the closed form of a power law cooled by synchrotron losses,
against a converged quad / brentq solution with Klein-Nishina losses, and of the loss table
itself.  Every bound is the figure measured here (profiles/NOTES_cooling.md) with the margin the
test's docstring states."""
import numpy as np
import pytest

import cooling_cases as CC
import cooling_np as CN
from naima_amd.constants import AR_CGS, ERG_PER_EV

T_CMB, T_FIR = 2.72548, 30.0
U_CMB, U_FIR = AR_CGS * T_CMB ** 4, 0.5 * ERG_PER_EV


# ------------------------------------------------------------------------- 1. the closed form
def test_synchrotron_loss_constant_against_literals():
    """(4/3) sigma_T c (B^2 / 8 pi) gamma^2 from CODATA-2018 literals, independent of the model's
    constant: 25.3 eV/s at 1 TeV in 100 uG, a cooling time of 1253 yr"""
    sigma_t, c, mec2_eV, erg_eV = 6.6524587321e-25, 2.99792458e10, 510998.95, 6.241509074e11
    B, E = 1e-4, 1e12
    b = 4.0 / 3.0 * sigma_t * c * (B * B / (8.0 * np.pi)) * (E / mec2_eV) ** 2 * erg_eV
    assert abs(b / 25.30 - 1.0) < 1e-3 and abs(E / b / CC.YR / 1253.0 - 1.0) < 1e-3
    assert abs(CN.syn_coefficient(B) * E * E / b - 1.0) < 1e-9


@pytest.mark.parametrize("age,bound", list(zip(CC.CF_AGES, (3.4e-13, 3.4e-13, 3.2e-15))))
def test_restatement_is_the_closed_form(age, bound):
    """Q and 1/b are power laws, so the scheme is exact up to rounding.  Measured: 8.3e-14 at
    age = inf and with the break mid-grid (the worst node is the fourth from the top, where
    S -> 0), 7.8e-16 at the tiny age; bounds: 4 x.  The last node (n = 0 = 0) is left out.  At the
    tiny age E* lies in E_i's own segment at every node and n / (Q age) - 1 was 4.4e-16
    (bound 4 x = 1.8e-15)."""
    c = CC.CF
    e = CN._log_grid(c["Emin"], c["Emax"], c["npd"])
    a = CN.syn_coefficient(c["B_G"])
    Q = c["Q0"] * (e / c["e0"]) ** -c["alpha"]
    n = CN.solve(e, Q, c["B_G"], age)
    exact = CN.closed_form_powerlaw(e, c["Q0"], c["e0"], c["alpha"], a, age, e[-1])
    rel = np.abs(n[:-1] / exact[:-1] - 1.0)
    print("closed form: age %g s, max rel %.3g at node %d" % (age, rel.max(), rel.argmax()))
    assert n[-1] == 0.0 and rel.max() < bound
    if age == CC.CF_AGES[2]:
        lim = np.abs(n[:-1] / (Q[:-1] * age) - 1.0).max()
        print("n / (Q age) - 1: %.3g" % lim)
        assert a * age * e[-1] < 2e-15 and lim < 1.8e-15
    if age == CC.CF_AGES[1]:  # the break is inside the grid: both regimes are present
        x = a * age * e
        assert (x < 1).sum() > 100 and (x > 1).sum() > 100


# ---------------------------------------------------- 2. against the converged solution
AGES2 = {"3e5yr": 3e5 * CC.YR, "steady": np.inf}
# measured maximum relative error over EVERY node with n > 1e-30 max, at 20 | 100 nodes per decade
MEASURED2 = {("ECPL", "3e5yr"): (1.048e-2, 3.90e-4), ("ECPL", "steady"): (1.048e-2, 3.90e-4),
             ("BPL", "3e5yr"): (3.84e-3, 8.97e-5), ("BPL", "steady"): (1.08e-3, 8.97e-5)}


@pytest.mark.parametrize("name,agename", list(MEASURED2))
def test_restatement_against_converged_solution(name, agename):
    """CMB + FIR losses (Klein-Nishina included), no magnetic field, 3e5 yr (the break near
    1 TeV) and the steady state; every node where n > 1e-30 max (all but the last, where n = 0).
    The bounds are 2 x the figures of MEASURED2, measured here; the error has to fall from 20 to
    100 nodes per decade.  The worst node: ECPL the last but one (112 of 114, 568 of 570: S -> 0
    there); BPL node 49 at 20 per decade (0.28 TeV, beside the kink of Q at 0.33 TeV) and node
    522 at 100 per decade (166 TeV, the Klein-Nishina part of the FIR loss)."""
    kind, p = CC.INJECTIONS[name]
    age = AGES2[agename]
    spl = [CN.loss_spline(T) for T in (T_CMB, T_FIR)]
    us = (U_CMB, U_FIR)

    def bfun(E):
        return sum(uu * np.exp(s(np.log(E))) for uu, s in zip(us, spl))

    def Qfun(E):
        return float(CC.injection_np(kind, p, np.array([E]))[0])

    kinks = [np.log(p[5])] if kind in (2, 3) else []
    errs, where = [], []
    for npd in (20, 100):
        e = CN._log_grid(1e9, 510.998e12, npd)
        loss = np.stack([CN.loss_table(T, e) for T in (T_CMB, T_FIR)])
        n = CN.solve(e, CC.injection_np(kind, p, e), 0.0, age, loss, us)
        ref = CN.converged(e, Qfun, bfun, age, e[-1], kinks)
        m = n > 1e-30 * n.max()
        assert m.sum() == e.size - 1 and n[-1] == 0.0 and ref[-1] == 0.0
        rel = np.abs(n[m] / ref[m] - 1.0)
        errs.append(rel.max())
        where.append(int(np.nonzero(m)[0][rel.argmax()]))
    print("%s %s: max rel error %.4g at 20/decade (node %d), %.4g at 100/decade (node %d)"
          % (name, agename, errs[0], where[0], errs[1], where[1]))
    b20, b100 = (2 * v for v in MEASURED2[(name, agename)])
    assert errs[0] < b20 and errs[1] < b100 and errs[1] < errs[0]


# --------------------------------------------------------------------- 3. the IC loss table
@pytest.mark.parametrize("T", [T_CMB, T_FIR])
def test_loss_table_thomson_limit_klein_nishina_and_photon_grid(T):
    """l(E) through the oracle's Khangulyan kernel: (4/3) sigma_T c gamma^2 per unit energy
    density where gamma kT << m_e c^2, below it and falling monotonically against it in the
    Klein-Nishina regime.  The deviation in the Thomson limit is the accuracy of Khangulyan's
    fits (quoted at ~1 %); measured at 1 GeV: 1.98e-4 (CMB), 1.9e-5 (FIR); bounds: 1.5 x.  The photon
    grid (200 per decade in z = E_ph / E_e up to 1/2, 100 per decade in 1 - z down to 1e-7):
    halving the spacing changes l by 7.6e-5 and l is within 6.4e-5 of the adaptive quadrature,
    both below 1.8e-4, the tightest bound of test 2 (BPL at 100 per decade)."""
    e = CN._log_grid(1e9, 510.998e12, 100)
    l1 = CN.loss_table(T, e)
    ratio = l1 / CN.thomson_loss(e)
    dev = abs(ratio[0] - 1.0)
    print("T = %g K: Thomson-limit deviation at 1 GeV %.3g; l / Thomson at the top %.3g"
          % (T, dev, ratio[-1]))
    assert 4.0 * (e[0] / 510998.95) * T * 1.6863699549e-10 < 1e-3  # (gamma kT << m_e c^2 there)
    assert dev < THOMSON_BOUND[T]
    kn = 4.0 * (e / 510998.95) * T * 1.6863699549e-10 > 0.1  # the Klein-Nishina regime
    assert np.all(np.diff(ratio) < 0) and ratio[-1] < 0.2 and kn.sum() > 50
    assert np.all(ratio[kn] < 1.0)
    l2 = CN.loss_table(T, e, 400, 200)
    conv = np.abs(l1 / l2 - 1.0).max()
    quad = max(abs(l1[i] / CN.loss_quad(T, e[i]) - 1.0) for i in (0, 300, e.size - 1))
    print("photon grid: halving the spacing changes l by %.3g; against quad %.3g" % (conv, quad))
    assert conv < 1.8e-4 and quad < 1.8e-4


THOMSON_BOUND = {T_CMB: 3.0e-4, T_FIR: 2.9e-5}
