"""The oracle (oracle/naima_np.py) against the reference: golden vectors made by
running the reference itself (tests/golden/gen_golden.py) and the known-answer
luminosities of the reference's tests/test_models.py."""
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import naima_np as O
from oracle import workloads_np as WN

HERE = os.path.dirname(os.path.abspath(__file__))
# the oracle repeats the reference's arithmetic on raw floats; only unit-conversion
# rounding (1 ulp per astropy .to()) separates them
RT = 2e-12


def _pds():
    return {
        "PowerLaw": O.ParticleDist("PowerLaw", amplitude=3e30, e_0=2e12, alpha=2.3),
        "ExponentialCutoffPowerLaw": O.ParticleDist(
            "ExponentialCutoffPowerLaw", amplitude=3e30, e_0=2e12, alpha=2.3, e_cutoff=30e12,
            beta=1.7),
        "BrokenPowerLaw": O.ParticleDist("BrokenPowerLaw", amplitude=3e30, e_0=2e12,
                                         e_break=0.5e12, alpha_1=1.6, alpha_2=2.9),
        "ExponentialCutoffBrokenPowerLaw": O.ParticleDist(
            "ExponentialCutoffBrokenPowerLaw", amplitude=3e30, e_0=2e12, e_break=0.5e12,
            alpha_1=1.6, alpha_2=2.9, e_cutoff=80e12, beta=0.8),
        "LogParabola": O.ParticleDist("LogParabola", amplitude=3e30, e_0=2e12, alpha=2.1,
                                      beta=0.15),
    }


def test_trapz_loglog_edges(golden):
    U = golden("units")
    for y, ref in zip(U["tz_y"], U["tz_out"]):
        assert_allclose(O.trapz_loglog(y, U["tz_x"]), ref, rtol=1e-14)
    assert_allclose(O.trapz_loglog(U["tz_y2d"], U["tz_x"], axis=0), U["tz_out2d"], rtol=1e-14)
    # exact power law with index -1 -> log branch
    x = U["tz_x"]
    assert_allclose(O.trapz_loglog(1 / x, x), np.log(x[-1] / x[0]), rtol=1e-13)


def test_particle_distributions(golden):
    U = golden("units")
    for k, pd in _pds().items():
        assert_allclose(pd(U["pd_e"]), U["pd_" + k], rtol=1e-13)


def test_grids(golden):
    U = golden("units")
    for i, (lo, hi, nd) in enumerate(U["grid_specs"]):
        g = O.electron_grid(lo, hi, nd)
        assert len(g) == U["grid_lens"][i]
        assert_allclose(g, U["grid_%d" % i], rtol=1e-14)
    assert_allclose(O.proton_grid(O.M_P_GEV + O.T_TH_GEV + 1e-4, 1e7, 100), U["pgrid_default"],
                    rtol=1e-14)
    assert_allclose(O.proton_grid(O.M_P_GEV + O.T_TH_GEV + 1e-4, 1e6, 100), U["pgrid_1PeV"],
                    rtol=1e-14)


def test_synchrotron_and_We(golden):
    U = golden("units")
    pds = _pds()
    gam = O.electron_grid(100e9, 1e15, 100)
    for tag, k in (("ecpl", "ExponentialCutoffPowerLaw"), ("bpl", "BrokenPowerLaw"),
                   ("lp", "LogParabola")):
        ne = O.nelec_on(pds[k], gam)
        assert_allclose(O.synchrotron_spectrum(U["E"], gam, ne, 1e-3), U["syn_" + tag], rtol=RT)
        assert_allclose(O.electron_energy_content(pds[k], gam), U["We_" + tag], rtol=RT)
        g10 = O.electron_grid(10e12, 1e15, 100)
        assert_allclose(O.electron_energy_content(pds[k], g10), U["We10_" + tag], rtol=RT)
    gam = O.electron_grid(1e9, 1e9 * O.MEC2_EV, 100)
    ne = O.nelec_on(pds["ExponentialCutoffPowerLaw"], gam)
    assert_allclose(O.synchrotron_spectrum(U["E"], gam, ne, 3.24e-6), U["syn_default"], rtol=RT)


def test_inverse_compton(golden):
    U = golden("units")
    pds = _pds()
    E = U["E"]
    gam = O.electron_grid(100e9, 1e15, 100)
    ne = O.nelec_on(pds["ExponentialCutoffPowerLaw"], gam)
    tot, per = O.ic_spectrum(E, gam, ne, [O.thermal_seed(s) for s in ("CMB", "FIR", "NIR")])
    assert_allclose(per, U["ic_3seeds_per"], rtol=RT)
    assert_allclose(tot, U["ic_3seeds"], rtol=RT)
    g2 = O.electron_grid(1e9, 1e9 * O.MEC2_EV, 100)
    seeds = [dict(type="thermal", T=5000.0, u=O.AR_CGS * 5000.0 ** 4, theta=None),
             dict(type="thermal", T=40.0, u=2.0 * O.ERG_PER_EV, theta=None)]
    tot, _ = O.ic_spectrum(E, g2, O.nelec_on(pds["BrokenPowerLaw"], g2), seeds)
    assert_allclose(tot, U["ic_custom"], rtol=RT)
    for ang in (45, 90, 135):
        seeds = [dict(type="thermal", T=20000.0, u=0.1, theta=np.deg2rad(ang))]
        tot, _ = O.ic_spectrum(E, gam, ne, seeds)
        assert_allclose(tot, U["ic_ani_%d" % ang], rtol=RT)
    tot, _ = O.ic_spectrum(E, gam, ne, [dict(type="array", energy=[50.0], density=[15.0])])
    assert_allclose(tot, U["ic_mono"], rtol=RT)
    tot, _ = O.ic_spectrum(E, gam, ne, [dict(type="array", energy=U["ic_arr_E"],
                                             density=U["ic_arr_n"])])
    assert_allclose(tot, U["ic_array"], rtol=RT)
    assert_allclose(tot, U["ic_array_edens"], rtol=1e-10)


def test_bremsstrahlung(golden):
    U = golden("units")
    pds = _pds()
    gam = O.electron_grid(O.MEC2_EV, 1e9 * O.MEC2_EV, 300)
    spec = O.brems_spectrum(U["E_brems"], gam, O.nelec_on(pds["ExponentialCutoffPowerLaw"], gam),
                            n0=2.5)
    assert_allclose(spec, U["brems_mec2"], rtol=RT)
    gam = O.electron_grid(100e6, 1e9 * O.MEC2_EV, 300)
    spec = O.brems_spectrum(U["E_brems"], gam, O.nelec_on(pds["BrokenPowerLaw"], gam))
    assert_allclose(spec, U["brems_default"], rtol=RT)


def test_pion_decay(golden):
    U = golden("units")
    pds = _pds()
    E = U["E_pp"]
    Ep = O.proton_grid(O.M_P_GEV + O.T_TH_GEV + 1e-4, 1e6, 100)
    lut = WN.get_lut()
    for eg, ana, lu in zip(U["ds_Eg"], U["ds_ana"], U["ds_lut"]):
        assert_allclose(O.pp_diffsigma(U["ds_Ep"], eg), ana, rtol=1e-12, atol=1e-300)
        assert_allclose(lut(U["ds_Ep"], eg), lu, rtol=1e-9, atol=1e-40)
    for tag, k in (("ecpl", "ExponentialCutoffPowerLaw"), ("bpl", "BrokenPowerLaw")):
        J = O.J_on(pds[k], Ep)
        assert_allclose(O.pion_spectrum(E, Ep, J), U["pp_ana_" + tag], rtol=1e-11)
        assert_allclose(O.pion_spectrum(E, Ep, J, diffsigma=lut), U["pp_lut_" + tag], rtol=1e-8)
        assert_allclose(O.proton_energy_content(pds[k], Ep), U["Wp_" + tag], rtol=RT)
    Ep = O.proton_grid(O.M_P_GEV + O.T_TH_GEV + 1e-4, 1e7, 100)
    J = O.J_on(pds["ExponentialCutoffPowerLaw"], Ep)
    assert_allclose(O.pion_spectrum(E, Ep, J, nh=3.0, nuclear_enhancement=False), U["pp_nonuc"],
                    rtol=1e-11)
    for hiE in ("Geant4", "SIBYLL", "QGSJET"):
        assert_allclose(O.pion_spectrum(E, Ep, J, hiE=hiE), U["pp_ana_" + hiE], rtol=1e-11)


def test_lnprobmodel_and_priors(golden):
    U = golden("units")
    flux = U["ll_flux"]
    d = dict(flux=flux, flux_error_lo=0.1 * flux, flux_error_hi=0.2 * flux, ul=U["ll_ul"],
             cl=U["ll_cl"])
    for m, ref in zip(U["ll_models"], U["ll_out"]):
        assert_allclose(O.lnprobmodel(m, d), ref, rtol=1e-13)
    assert_allclose(U["ll_out_sedmodel"], U["ll_out"], rtol=1e-12)
    assert_allclose(O.normal_prior(1.3, 1.0, 0.5), U["prior_normal"][0], rtol=1e-15)
    assert_allclose(O.log_uniform_prior(2.0, 1.0, 3.0), U["prior_logu"][0], rtol=1e-15)
    assert O.uniform_prior(1.0, 0.0, 2.0) == 0.0 and O.uniform_prior(3.0, 0.0, 2.0) == -np.inf


def test_lnprobmodel_confidence_level_indexed_by_violations(golden):
    """lnprob.npz (gen_golden_lnprob.py): asymmetric errors, five upper limits, a distinct cl per
    point and models violating 0 .. 4 of them -- the reference's cl[nviol] (core.py:89-92) pinned
    to a value; cl[nviol - 1], or lo / hi swapped, would miss it by far more than the tolerance"""
    z = golden("lnprob")
    d = dict(flux=z["flux"], flux_error_lo=z["flux_error_lo"], flux_error_hi=z["flux_error_hi"],
             ul=z["ul"], cl=z["cl"])
    assert not np.array_equal(d["flux_error_lo"], d["flux_error_hi"])
    assert sorted(set(z["nviol"].tolist())) == [0, 1, 2, 3, 4]
    for m, k, ref in zip(z["models"], z["nviol"], z["lnprobmodel"]):
        assert int(np.sum(m[z["ul"]] > z["flux"][z["ul"]])) == k
        assert_allclose(O.lnprobmodel(m, d), ref, rtol=1e-13)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_workloads(golden, name):
    z = golden(name)
    raw = WN.raw_from_npz(z)
    n = len(z["pars"]) if name != "cfg4" else 2
    for i in range(n):
        lp, flux, blob = WN.lnprob(name, z["pars"][i], raw)
        tol = 1e-8 if name == "cfg5" else 1e-10
        assert_allclose(flux, z["flux"][i], rtol=tol, atol=1e-300)
        assert_allclose(lp, z["lnprob"][i], rtol=1e-8)
        if not np.isnan(z["blob"][i]):
            assert_allclose(blob, z["blob"][i], rtol=1e-11)
    if name == "cfg5":
        raw = WN.raw_from_npz(z, "analytic_data_")
        for i in range(3):
            lp, flux, blob = WN.lnprob(name, z["pars"][i], raw, useLUT=False)
            assert_allclose(flux, z["flux_analytic"][i], rtol=1e-10)
            assert_allclose(lp, z["lnprob_analytic"][i], rtol=1e-8)


def test_cfg3_components(golden):
    z = golden("cfg3")
    p = z["pars"][0]
    pd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12, alpha=p[1],
                        e_cutoff=10 ** p[2] * 1e12, beta=p[4])
    g_ic = O.electron_grid(100e9, 1e9 * O.MEC2_EV, 100)
    g_sy = O.electron_grid(1e9, 1e9 * O.MEC2_EV, 100)
    assert_allclose(g_ic, z["c_ic_gam"], rtol=1e-14)
    assert_allclose(g_sy, z["c_syn_gam"], rtol=1e-14)
    assert_allclose(O.nelec_on(pd, g_ic), z["c_ic_nelec"], rtol=1e-13)
    E = WN.data_energy_eV(WN.raw_from_npz(z))
    _, per = O.ic_spectrum(E, g_ic, O.nelec_on(pd, g_ic),
                           [O.thermal_seed(s) for s in ("CMB", "FIR", "NIR")])
    assert_allclose(per, z["c_specic"], rtol=RT)
    assert_allclose(O.synchrotron_spectrum(E, g_sy, O.nelec_on(pd, g_sy), p[3] * 1e-6),
                    z["c_syn_spec"], rtol=RT)
    assert_allclose(O.electron_energy_content(pd, g_ic), z["c_We"], rtol=RT)


def test_known_answers():
    """The reference's own pins (tests/test_models.py:69-450), rtol 1e-7 as there."""
    KA = json.load(open(os.path.join(HERE, "golden", "known_answers.json")))
    E = np.logspace(0, 15, 1000)
    mec2 = O.MEC2_EV

    def lum(spec, EE=E):
        return O.trapz_loglog(spec * EE, EE) * O.ERG_PER_EV

    amp = 1.0 / mec2  # 1/mec2 in 1/eV
    dists = [O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=amp, e_0=20e12, alpha=2.0,
                            e_cutoff=10e12, beta=1.0),
             O.ParticleDist("PowerLaw", amplitude=amp, e_0=20e12, alpha=2.0),
             O.ParticleDist("BrokenPowerLaw", amplitude=amp, e_0=20e12, e_break=1e12,
                            alpha_1=1.5, alpha_2=2.5)]
    gam = O.electron_grid(100e9, 1e15, 100)
    lsy, We, lic = [], [], []
    for pd in dists:
        ne = O.nelec_on(pd, gam)
        lsy.append(lum(O.synchrotron_spectrum(E, gam, ne, 3.24e-6)))
        We.append(O.electron_energy_content(pd, gam))
        lic.append(lum(O.ic_spectrum(E, gam, ne, [O.thermal_seed("CMB")])[0]))
    assert_allclose(lsy, KA["syn_lum"], rtol=1e-7)
    assert_allclose(We, KA["We"], rtol=1e-7)
    assert_allclose(lic, KA["ic_lum"], rtol=1e-7)
    ne = O.nelec_on(dists[0], gam)
    assert_allclose(lum(O.synchrotron_spectrum(E, gam, ne, 1.0)), KA["syn_lum_B1G"], rtol=1e-7)
    g2 = O.electron_grid(1e9, 1e9 * mec2, 100)
    tot, _ = O.ic_spectrum(E, g2, O.nelec_on(dists[0], g2),
                           [O.thermal_seed(s) for s in ("CMB", "FIR", "NIR")])
    assert_allclose(lum(tot), KA["ic_lum_3seeds"], rtol=1e-7)
    ani = []
    for ang in (45, 90, 135):
        seeds = [dict(type="thermal", T=20000.0, u=0.1, theta=np.deg2rad(ang))]
        ani.append(lum(O.ic_spectrum(E, gam, O.nelec_on(dists[1], gam), seeds)[0]))
    assert_allclose(ani, KA["ic_ani_lum"], rtol=1e-7)
    E2 = np.logspace(8, 14, 100)
    g3 = O.electron_grid(mec2, 1e9 * mec2, 300)
    assert_allclose(lum(O.brems_spectrum(E2, g3, O.nelec_on(dists[0], g3)), E2), KA["brems_lum"],
                    rtol=1e-7)
    # pion decay: amplitudes reset to 1/TeV (tests/test_models.py:399-400)
    for pd in dists:
        pd.params["amplitude"] = 1e-12
    Epp = np.logspace(-3, 3, 60) * 1e12
    Ep = O.proton_grid(O.M_P_GEV + O.T_TH_GEV + 1e-4, 1e6, 100)
    lut = WN.get_lut()
    l_lut, l_ana, Wp = [], [], []
    for pd in dists:
        J = O.J_on(pd, Ep)
        l_lut.append(lum(O.pion_spectrum(Epp, Ep, J, diffsigma=lut), Epp))
        l_ana.append(lum(O.pion_spectrum(Epp, Ep, J), Epp))
        Wp.append(O.proton_energy_content(pd, Ep))
    assert_allclose(l_lut, KA["pp_lum_LUT"], rtol=1e-7)
    assert_allclose(l_ana, KA["pp_lum_noLUT"], rtol=1e-7)
    assert_allclose(Wp, KA["Wp"], rtol=1e-7)
    E3 = np.logspace(9, 13, 20)
    J = O.J_on(dists[0], Ep)
    assert_allclose(lum(O.pion_spectrum(E3, Ep, J, nuclear_enhancement=False), E3),
                    KA["pp_lum_nonuc"], rtol=1e-7)


def test_kelner06_oracle_pinned(golden):
    """PionDecayKelner06 restatement against the reference's output: identical at the
    reference's own quad tolerance (1e-3); the converged integrals differ from it by
    less than that tolerance (measured: 4e-5)"""
    z = golden("extra")
    E = z["k06_E_eV"]
    cases = (("pl", O.ParticleDist("PowerLaw", amplitude=4e35, e_0=1e12, alpha=2.2)),
             ("ecpl", O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=4e35, e_0=1e12,
                                     alpha=2.0, e_cutoff=1e14, beta=1.0)))
    for tag, pd in cases:
        def J(Et, pd=pd):
            return float(pd(Et * 1e12)) * 1e12
        spec, nhat = O.k06_spectrum(E, J, nh=2.0, epsrel=1e-3)
        assert_allclose(O.to_flux(spec, O.KPC_CM), z["k06_%s_flux" % tag], rtol=1e-12)
        assert_allclose(nhat, float(z["k06_%s_nhat" % tag]), rtol=1e-12)
        conv, _ = O.k06_spectrum(E, J, nh=2.0, epsrel=1e-10)
        assert_allclose(O.to_flux(conv, O.KPC_CM), z["k06_%s_flux" % tag], rtol=1e-3)
    hi = E >= 1e11
    spec, nhat = O.k06_spectrum(E[hi], lambda Et: float(cases[0][1](Et * 1e12)) * 1e12, nh=2.0)
    assert nhat == 1.0
    assert_allclose(O.to_flux(spec, O.KPC_CM), z["k06_pl_flux_hi_only"], rtol=1e-12)


# ---------------------------------------------------------------------------------------
# Kelner06: the converged reference that tests/test_gpu_kelner.py holds the kernel to.
# An adaptive rule's error estimate is only as good as the integrand is smooth inside each
# interval, so k06_spectrum(breaks_TeV=...) ends an interval at every kink.  Certified here by
# two independent methods: the same split quad at two tolerances, and mpmath's tanh-sinh
# rule at 30 digits on a separate restatement of the untransformed formulas.
# ---------------------------------------------------------------------------------------
def _mp_kelner06(tag):
    """mpmath (30 digits) restatement of radiative.py:1597-1728 for one parameter set:
    full(E_TeV), delta(E_TeV), wp() -> (value, mpmath's own relative error estimate)"""
    import mpmath as mp

    import kelner_cases as KC
    kind, par = KC._find(tag)
    p = {k: mp.mpf(float(v)) for k, v in dict(par, amplitude=KC.AMP, e_0=KC.E0).items()}
    KPI, MP_, MPI, ETH = (mp.mpf(v) for v in (O.K06_KPI, O.K06_MP_TEV, O.K06_MPI_TEV,
                                              O.K06_ETH_TEV))
    kinks = [mp.mpf(b) for b in O.k06_kinks(KC.breaks_TeV(par))]

    def J(Et):  # models.py:234-238, 330-335; 1/TeV
        x = Et * mp.mpf(1e12) / p["e_0"]
        if Et * mp.mpf(1e12) < p["e_break"]:
            v = x ** -p["alpha_1"]
        else:
            v = (p["e_break"] / p["e_0"]) ** (p["alpha_2"] - p["alpha_1"]) * x ** -p["alpha_2"]
        if "e_cutoff" in p:
            v *= mp.exp(-(Et * mp.mpf(1e12) / p["e_cutoff"]) ** p["beta"])
        return p["amplitude"] * v * mp.mpf(1e12)

    def sigma(Ep):  # :1625-1647
        L = mp.log(Ep)
        s = mp.mpf("34.3") + mp.mpf("1.88") * L + mp.mpf("0.25") * L ** 2
        if Ep <= mp.mpf(0.1):
            s *= (1 - (ETH / Ep) ** 4) ** 2 * (0 if Ep < ETH else 1)
        return s * mp.mpf("1e-27")

    def F(x, Ep):  # :1597-1623
        L = mp.log(Ep)
        B = mp.mpf("1.30") + mp.mpf("0.14") * L + mp.mpf("0.011") * L ** 2
        beta = 1 / (mp.mpf("1.79") + mp.mpf("0.11") * L + mp.mpf("0.008") * L ** 2)
        k = 1 / (mp.mpf("0.801") + mp.mpf("0.049") * L + mp.mpf("0.014") * L ** 2)
        xb = x ** beta
        F1 = B * (mp.log(x) / x) * ((1 - xb) / (1 + k * xb * (1 - xb))) ** 4
        F2 = (1 / mp.log(x) - 4 * beta * xb / (1 - xb)
              - 4 * k * beta * xb * (1 - 2 * xb) / (1 + k * xb * (1 - xb)))
        return F1 * F2

    def done(v, err, scale):
        return float(scale * v), float(err / abs(v))

    def full(Eg):
        Eg = mp.mpf(Eg)

        def f(x):
            # tanh-sinh nodes crowd towards x = 1, where ln x rounds to 0 (the limit is 0)
            # and F1 F2 cancels: twice the digits there
            if x == 1:
                return mp.mpf(0)
            with mp.workdps(2 * mp.mp.dps + 10):
                v = sigma(Eg / x) * J(Eg / x) * F(x, Eg / x) / x
            return +v
        ends = [mp.mpf(0)] + sorted(Eg / b for b in kinks if b > Eg) + [mp.mpf(1)]
        return done(*mp.quad(f, ends, error=True), O.C_CGS * 1e-12)

    def delta(Eg):
        Eg = mp.mpf(Eg)
        Epimin = Eg + MPI ** 2 / (4 * Eg)

        def f(Epi):
            Ep0 = MP_ + Epi / KPI
            return sigma(Ep0) * J(Ep0) / mp.sqrt(Epi ** 2 - MPI ** 2)
        ends = [Epimin] + [e for e in sorted((b - MP_) * KPI for b in kinks) if e > Epimin] \
            + [mp.inf]
        return done(*mp.quad(f, ends, error=True), 2 * O.C_CGS / O.K06_KPI * 1e-12)

    def wp():
        ends = [ETH] + [b for b in kinks if b > ETH] + [mp.inf]
        return done(*mp.quad(lambda E: E * J(E), ends, error=True), 1.0)

    return mp, full, delta, wp


@pytest.mark.parametrize("tag", ["bpl_above", "ecbpl_below"])
def test_kelner06_split_reference_is_converged(tag):
    """The split reference at epsrel 1e-11 (what the GPU tests use), at 1e-13 and mpmath at 30
    digits agree to 1e-10 on both branches and for Wp.  Measured over all six broken sets of
    kelner_cases: at most 3e-13 between any two of the three; mpmath's own error estimate is
    below 1e-19 everywhere.  (A
    difference of 2e-8 at 1 TeV once seen between mpmath and quad does not reproduce with
    the same break points on both sides: see profiles/NOTES_kelner.md.)"""
    import kelner_cases as KC
    mp, full, delta, wp = _mp_kelner06(tag)
    with mp.workdps(30):
        for is_full, energies in ((True, (1e11, 1e12, 3e13)), (False, (1e8, 1e9, 5e10))):
            for E in energies:
                q11 = KC.branch(tag, E, is_full)
                q13 = KC.branch(tag, E, is_full, epsrel=1e-13)
                m, merr = (full if is_full else delta)(E * 1e-12)
                print("%s %s %.0e eV: quad 1e-11 / 1e-13 - 1 = %.1e, / mpmath - 1 = %.1e "
                      "(mpmath's error estimate %.1e)"
                      % (tag, "full" if is_full else "delta", E, q11 / q13 - 1, q11 / m - 1, merr))
                assert merr < 1e-12
                assert_allclose(q11, q13, rtol=1e-10)
                assert_allclose(q11, m, rtol=1e-10)
        m, merr = wp()
        assert merr < 1e-12
        assert_allclose(KC.Wp_TeV(tag), KC.Wp_TeV(tag, epsrel=1e-13), rtol=1e-10)
        assert_allclose(KC.Wp_TeV(tag), m, rtol=1e-10)


def test_kelner06_split_reference_composition():
    """kelner_cases.spectrum (cached single integrals) is k06_spectrum(breaks_TeV=...).  The
    unsplit adaptive quad at the same tolerance lands on the same numbers (it bisects its way to
    a kink; measured 6e-11) -- the split adds the certainty that its error estimate holds"""
    import kelner_cases as KC
    E = KC.energies(1e11)
    for tag in ("bpl_above", "ecpl_b2.5"):
        kind, par = KC._find(tag)
        spec, nhat = O.k06_spectrum(E, KC.J_per_TeV(tag), epsrel=1e-11,
                                    breaks_TeV=KC.breaks_TeV(par))
        mine, mine_nhat = KC.spectrum(tag, E, 1e11)
        assert_allclose(mine, spec, rtol=1e-14)
        assert_allclose(mine_nhat, nhat, rtol=1e-14)
        plain, _ = O.k06_spectrum(E, KC.J_per_TeV(tag), epsrel=1e-11)
        err = np.abs(plain / spec - 1).max()
        print(tag, "unsplit quad at epsrel 1e-11 vs split: %.1e" % err)
        assert err < 1e-9
    # the analytic Wp of a power law: A e0^alpha Eth^(2 - alpha) / (alpha - 2)
    assert_allclose(KC.Wp_TeV("pl"), KC.AMP * 1e12 * 1.22e-3 ** -0.2 / 0.2, rtol=1e-11)
    # listed breaks are merged with the cross section's own kinks, sorted and unique
    assert O.k06_kinks((3.7, 0.1)) == [1.22e-3, 0.1, 3.7]
