"""Synchrotron self-absorption on the host: the restatement (tests/ssa_np.py) against the
physics -- the derivative D against a central difference of ln Gtilde, kappa against the closed
form of Rybicki & Lightman (6.53) for a power law, the slopes 5/2 and -(p-1)/2 of an absorbed
sphere, the escape fractions' limits --, the test cases (tests/ssa_cases.py) against the planner and
against what they are there for, and SynchrotronSelfAbsorption's grammar and errors.  No GPU."""
from math import gamma as G
from math import pi, sqrt

import mpmath
import numpy as np
import pytest

import ssa_cases as AC
import ssa_np as ANP
import synchrotron_np as SNP

LD = SNP.LD
UNDER = 2.0 ** -960  # the sum before the prefactor below this: an underflow element
ALL = [(c[0], g) for c in AC.CASES for g in AC.grids_of(c[2])]
ALL_IDS = ["%s-%s" % cg for cg in ALL]

E_, C_, HBAR, ME, ERG = (float(v) for v in (SNP._E, SNP._C, SNP._HBAR, SNP._ME, SNP._ERG))
H_PLANCK = 2 * pi * HBAR


def _power_law(K, p, lg_lo, lg_hi, per_decade=100):
    """(w, dlw [1][nG], gam, lx) of N(gamma) = K gamma^-p on a log-uniform grid"""
    n = int(round((lg_hi - lg_lo) * per_decade)) + 1
    gam = 10.0 ** np.linspace(lg_lo, lg_hi, n)
    g = gam.astype(LD)
    lx = np.log(g[1:] / g[:-1]).astype(np.float64)
    w = (K * g ** (1 - LD(p))).astype(np.float64)[None, :]
    dlw = np.zeros_like(w)
    dlw[0, :-1] = np.log(w[0, 1:].astype(LD) / w[0, :-1].astype(LD))
    return w, dlw, gam, lx


# ------------------------------------------------------------------------------ 1. the physics
def test_D_is_the_logarithmic_derivative_of_Gtilde():
    """D against the central difference of ln Gtilde in ln x, step 1e-6, in mpmath: what is left
    is the rule's h^2/6 |d^3 ln Gtilde / d(ln x)^3| <= 1e-12 (1 + x) / 6 = 2e-11 at x = 100.
    D <= 1/3 and H > 0 everywhere"""
    mpmath.mp.dps = 40

    def lnG(lx):
        x = mpmath.exp(lx)
        c = mpmath.cbrt(x)
        g1 = mpmath.mpf("1.808") * c / mpmath.sqrt(1 + mpmath.mpf("3.4") * c ** 2)
        g2 = 1 + mpmath.mpf("2.210") * c ** 2 + mpmath.mpf("0.347") * c ** 4
        g3 = 1 + mpmath.mpf("1.353") * c ** 2 + mpmath.mpf("0.217") * c ** 4
        return mpmath.log(g1 * g2 / g3) - x

    h = mpmath.mpf("1e-6")
    xs = np.geomspace(1e-6, 100.0, 81)
    worst = 0.0
    for x in xs:
        lx = mpmath.log(mpmath.mpf(float(x)))
        cd = (lnG(lx + h) - lnG(lx - h)) / (2 * h)
        worst = max(worst, abs(float(cd - mpmath.mpf(float(ANP.D_of(LD(x)))))))
    print("max |D - central difference| = %.3g" % worst)
    assert worst <= 1e-10
    x = np.geomspace(1e-30, 746.0, 4001).astype(LD)
    D = ANP.D_of(x)
    assert np.all(D <= LD(1) / 3) and np.all(ANP.Q_of(x) > 0)
    assert abs(float(D[0]) - 1 / 3) < 1e-9


@pytest.mark.parametrize("p", [2.0, 2.5, 3.2])
def test_kappa_is_rybicki_lightman_6_53(p):
    """B = 1 mG, gamma from 10^0.5 to 10^9 at 100 nodes per decade, nu = 1e8 and 1e12 Hz, against
    the pitch-angle average of R&L 6.53: within 3e-3, AKP10's 0.2 % for Gtilde plus the grid's
    share (measured: -0.9e-3 .. -1.2e-3)"""
    B = 1e-3
    w, dlw, gam, lx = _power_law(1.0, p, 0.5, 9.0)
    a = (p + 2) / 2
    sin_avg = sqrt(pi) / 2 * G((a + 2) / 2) / G((a + 3) / 2)
    for nu in (1e8, 1e12):
        E_eV = np.array([H_PLANCK * nu / ERG])
        k = float(ANP.kappa(w, dlw, np.array([B]), gam, lx, E_eV)["kappa"][0, 0])
        rl = (sqrt(3) * E_ ** 3 / (8 * pi * ME) * (3 * E_ / (2 * pi * ME ** 3 * C_ ** 5)) ** (p / 2)
              * (ME * C_ * C_) ** (p - 1) * B ** a * sin_avg * G((3 * p + 2) / 12)
              * G((3 * p + 22) / 12) * nu ** (-(p + 4) / 2))
        print("p = %.1f, nu = %.0e: kappa / R&L - 1 = %.3g" % (p, nu, k / rl - 1))
        assert abs(k / rl - 1) <= 3e-3


def test_slopes_of_an_absorbed_sphere():
    """B = 1 G, R = 1e15 cm, N = 1e52 gamma^-2.5 on 10 .. 1e6: L_nu rises as nu^(5/2) between
    5.62e9 and 1e10 Hz (tau = 443 and 68) and falls as nu^-(p-1)/2 between 3.16e11 and 5.62e11"""
    w, dlw, gam, lx = _power_law(1e52, 2.5, 1.0, 6.0)
    nu = np.array([10 ** 9.75, 1e10, 10 ** 11.5, 10 ** 11.75])
    E = H_PLANCK * nu / ERG
    B = np.array([1.0])
    kap = ANP.kappa(w, dlw, B, gam, lx, E)["kappa"][0]
    spec = SNP.spectrum(w, dlw, B, gam, lx, E)["spec"][0]
    tau = [ANP.tau_of(float(k), 1e15, "sphere") for k in kap]
    f = np.array([float(ANP.escape(t, "sphere")) for t in tau])
    L = E * spec.astype(np.float64) * f
    thick = np.log(L[1] / L[0]) / np.log(nu[1] / nu[0])
    thin = np.log(L[3] / L[2]) / np.log(nu[3] / nu[2])
    print("tau = %.4g, %.4g; slopes %.4f, %.4f" % (tau[0], tau[1], thick, thin))
    assert abs(thick - 2.5) <= 0.01 and abs(thin + 0.75) <= 0.01
    assert abs(float(tau[0]) / 443 - 1) < 0.01 and abs(float(tau[1]) / 68 - 1) < 0.01


def test_escape_fraction_limits_and_monotonicity():
    """f(0) = 1, f -> 1 - 3 tau/8 (sphere), 1 - tau/2 (slab), f -> 3/(2 tau), 1/tau; strictly
    decreasing; the sphere's series of 20 terms is the closed form to 1e-20 up to tau = 1 (the
    first term left out is 66/23! = 2.6e-21)"""
    mp = mpmath.mp
    taus = np.geomspace(1e-12, 1e4, 129)
    for geo, slope, tail in (("sphere", mp.mpf(3) / 8, mp.mpf(3) / 2), ("slab", mp.mpf(1) / 2, 1)):
        assert ANP.escape(0, geo) == 1
        f = [ANP.escape(float(t), geo) for t in taus]
        assert all(b < a for a, b in zip(f, f[1:])) and f[0] < 1
        t = mp.mpf("1e-8")
        assert abs((1 - ANP.escape(t, geo)) / t - slope) < 1e-7
        t = mp.mpf("1e4")
        assert abs(ANP.escape(t, geo) * t / tail - 1) < 1e-3
    for t in (1e-12, 1e-3, 0.5, 1 - 2.0 ** -53, 1.0):
        assert abs(ANP.escape_series(t, 20) - ANP.escape(t, "sphere")) < 1e-20
    assert abs(ANP.escape_series(1.0, 2) - (1 - mp.mpf(3) / 8)) < 1e-40


def test_apply_restatement_rules():
    kap = np.array([[0.0, 1.0, np.nan], [2.0, 3.0, 4.0]])
    buf = np.array([[2.0, 2.0, 2.0], [1.0, 1.0, 1.0]])
    out = ANP.apply(kap, [1.0, -1.0], "sphere", terms=[(0.5, buf), (0.25, buf)], colfac=[1, 2, 3])
    assert out[0, 0] == 1.5 and np.isnan(float(out[0, 2])) and all(np.isnan(float(v)) for v in out[1])
    assert abs(out[0, 1] / (3 * ANP.escape(mpmath.mpf(3) / (2 * mpmath.pi), "sphere")) - 1) < 1e-40
    tau = ANP.apply(kap[1], [1.0, 2.0], "slab", write_tau=True)
    assert abs(tau[1, 2] * mpmath.pi - 1) < 1e-40 and abs(tau[0, 0] * mpmath.pi - 2) < 1e-40
    for bad in (0.0, np.nan, np.inf, -np.inf):
        assert np.isnan(float(ANP.apply(kap[1], [bad], "slab")[0, 0]))


# ---------------------------------------------------------------------------------- 2. the cases
@pytest.mark.parametrize("case", AC.CASES, ids=AC.CASE_IDS)
def test_case_labels_are_the_planners(case):
    cid, N, nG, nE, label, _ = case
    rc, p = AC.plan(N, nG, nE)
    assert rc == 0 and p[:3] == label
    assert p[3] == 24 * nG + 32768 and p[2] == -(-nE // p[1])
    assert N >= 9


def test_cases_reach_every_instance():
    """C = 4, 8, 16 on one tile, 4 and 8 on several (nE > 64 caps C at 8), both halvings, dynamic
    LDS on both sides of 64 KB and the most the launcher takes; nE = 1, 12, 64 and multi-tile;
    the planner refuses what the emission's refuses"""
    plans = {c[0]: AC.plan(c[1], c[2], c[3])[1] for c in AC.CASES}
    assert {(p[0], p[2] > 1) for p in plans.values()} == {(4, False), (8, False), (16, False),
                                                          (4, True), (8, True)}
    assert plans["halve-16"][0] == 8 and AC.plan(1024, 257, 1)[1][0] == 16
    assert plans["halve-8"][0] == 4 and AC.plan(2048, 65, 1)[1][0] == 8
    assert plans["lds-over"][3] > 64 * 1024 > plans["c16-64"][3]
    assert plans["lds-max"][3] == 153584 and AC.plan(9, 5035, 12)[0] != 0
    assert {c[3] for c in AC.CASES} >= {1, 12, 64, 67, 130}
    assert min(c[2] for c in AC.CASES) == 40
    for N, nG, nE in ((-1, 40, 12), (9, 1, 12), (9, 40, 0)):
        assert AC.plan(N, nG, nE)[0] != 0
    assert AC.plan(0, 40, 12) == (0, (0, 0, 0, 0))


@pytest.mark.parametrize("cid,gname", ALL, ids=ALL_IDS)
def test_case_inputs(cid, gname):
    """per case and grid, from the reference alone: at most 5 % of the live elements are underflow
    elements; the planted segments' total log-ratio is the target to an ulp of dlw and the
    weights follow their log-ratios to 4 eps; the bad-field rows and the NaN-weight row are NaN
    where the contract says; zero nodes and dead energies exist across the cases"""
    d = AC.make_case(cid, gname)
    ref = AC.case_reference(cid, gname)
    kap = ref["kappa"]
    live = ~np.isnan(kap) & (ref["S"] > 0)
    under = live & (ref["S_raw"] < UNDER)
    assert under.sum() <= 0.05 * live.sum(), (under.sum(), live.sum())
    assert np.all(kap[live] > 0)
    nan = np.isnan(kap)
    for r in AC.BAD_B:
        assert nan[r].all()
    assert np.array_equal(nan[AC.NAN_ROW], ref["i0"][AC.NAN_ROW] <= d["nan_node"])
    assert not nan[[0, 1, 2, 8]].any()
    wd, dlwd, Bd = d["dist"]
    for r, k, i, target in d["planted"]:
        x = SNP.x_of(Bd[r], d["gam"], d["E"])[k, i:i + 2]
        Q = ANP.Q_of(x)
        dl = (LD(dlwd[r, i]) - LD(d["lx"][i])) + np.log1p((Q[1] - Q[0]) / Q[0]) - (x[1] - x[0])
        assert abs(float(dl - LD(target))) <= 2.0 ** -52 * max(1.0, abs(dlwd[r, i]))
    pos = (wd[:, :-1] > 0) & (wd[:, 1:] > 0)
    with np.errstate(all="ignore"):
        ratio = np.log(wd[:, 1:].astype(LD) / wd[:, :-1].astype(LD))
        off = np.abs(ratio - dlwd[:, :-1].astype(LD))[pos]
    assert off.max() <= 4 * 2.0 ** -53 * (1 + np.abs(dlwd[:, :-1][pos]).max())


def test_cases_have_zero_nodes_dead_energies_and_small_dl():
    zero = dead = small = 0
    for cid, gname in ALL:
        d, ref = AC.make_case(cid, gname), AC.case_reference(cid, gname)
        zero += int((d["dist"][0] == 0).any())
        dead += int(((ref["S"] == 0) & ~np.isnan(ref["kappa"])).any())
        small += sum(1 for p in d["planted"] if abs(p[3]) < 2.0 ** -10)
    assert zero >= len(ALL) - 2 and dead >= 10 and small >= 20


# ------------------------------------------------------------------------ 3. the model's grammar
def test_model_grammar_and_errors():
    import naima_amd as na
    from naima_amd import darray
    u = na.u
    pd = na.PowerLaw(1e36 / u.eV, 1 * u.TeV, 2.5)
    syn = na.Synchrotron(pd, B=1 * u.G)
    m = syn.self_absorption(1e15 * u.cm)
    assert isinstance(m, na.SynchrotronSelfAbsorption) and m.geometry == "sphere"
    assert na.models.SynchrotronSelfAbsorption is na.SynchrotronSelfAbsorption
    assert m.batch_size is None and not m.on_device
    assert syn.self_absorption(3 * u.pc, geometry="slab").geometry == "slab"
    for bad in (-1 * u.cm, 0 * u.cm, np.nan * u.cm, np.inf * u.cm):
        with pytest.raises(ValueError):
            syn.self_absorption(bad)
    for bad in (lambda: syn.self_absorption(3.0), lambda: syn.self_absorption(3.0 * u.s),
                lambda: syn.self_absorption(np.ones((2, 2)) * u.cm),
                lambda: na.SynchrotronSelfAbsorption(pd, 1 * u.cm),
                lambda: na.SynchrotronSelfAbsorption(na.InverseCompton(pd), 1 * u.cm)):
        with pytest.raises(TypeError):
            bad()
    for geo in ("cube", "Sphere", None):
        with pytest.raises(ValueError):
            syn.self_absorption(1 * u.cm, geometry=geo)
    # a batch: the radius per walker, the population per walker, both; sizes have to agree
    batch = na.Synchrotron(na.PowerLaw(np.full(3, 1e36) / u.eV, 1 * u.TeV, 2.5), B=1 * u.G)
    assert syn.self_absorption(np.array([1e15, 2e15, -1.0]) * u.cm).batch_size == 3
    assert batch.self_absorption(1e15 * u.cm).batch_size == 3
    assert batch.self_absorption(np.full(3, 1e15) * u.cm).batch_size == 3
    with pytest.raises(ValueError):
        batch.self_absorption(np.full(4, 1e15) * u.cm).batch_size
    # a particle grid per walker has no absorption kernel
    e = np.geomspace(1e-6, 1e-2, 5) * u.eV
    for kw in (dict(Eemin=np.array([1.0, 2.0]) * u.GeV), dict(Eemax=np.array([1.0, 2.0]) * u.PeV),
               dict(nEed=np.array([100, 50]))):
        s2 = na.Synchrotron(pd, B=1 * u.G, **kw)
        for call in (lambda: s2.self_absorption(1e15 * u.cm).opacity(e),
                     lambda: s2.self_absorption(1e15 * u.cm).absorption_area(e),
                     lambda: s2.flux(e, radius=1e15 * u.cm),
                     lambda: s2.sed(e, radius=1e15 * u.cm)):
            with pytest.raises(NotImplementedError, match="the same for every walker"):
                call()
    assert issubclass(darray.DSsa, darray.DFactor)
    with pytest.raises(ValueError):
        darray.DSsa(None, None, True, 1.0, "cube", 1, 1)
