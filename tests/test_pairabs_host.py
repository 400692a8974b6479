"""Pair-production absorption on the host: the restatement (tests/pairabs_cases.py) against the
mpmath golden file, the cross section's peak, the single-integral identity that the kernel uses,
the tabulated-field rule, and PairAbsorptionModel's grammar and errors (no GPU)."""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

import pairabs_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "pairabs.npz")))


def test_restatement_equals_the_golden_file(golden):
    eta = golden["eta"]
    np.testing.assert_array_equal(eta, PC.eta_grid())
    assert eta.size == 42 and eta[0] == 0.02 and eta[-1] == 1e4
    # doubles against mpmath at 30 digits: the composite rules converge to rounding, the Wien
    # side loses x0 * 2^-53 <~ 1e-13 in exp(-x)
    assert_allclose(PC.iso_np(eta), golden["iso"], rtol=1e-12, atol=0)
    assert np.all(golden["iso"] > 0) and np.all(np.isfinite(golden["iso"]))
    for deg in PC.ANGLES_DEG:
        ref = golden["ang%d" % deg]
        mu = 1.0 - np.cos(np.deg2rad(deg))
        big = ref >= 1e-280
        assert big.sum() >= 30
        assert_allclose(PC.ang_np(eta, mu)[big], ref[big], rtol=1e-12, atol=0)
        assert np.all(PC.ang_np(eta, mu)[~big] <= 1e-280)
    mono = golden["mono"]
    assert np.all(mono[eta <= 1.0] == 0.0) and np.all(mono[eta > 1.0] > 0.0)
    assert_allclose(PC.sigma_bar_np(eta), mono, rtol=1e-13, atol=0)
    # one ulp above the threshold: sbar = (sigma_T / 2) (s0 - 1)^(3/2) to leading order
    above = eta == np.nextafter(1.0, 2.0)
    assert_allclose(mono[above], 0.5 * (eta[above] - 1.0) ** 1.5, rtol=1e-12)


def test_cross_section_peak(golden):
    # mpmath at 30 digits: sigma is largest at s = 1.96790332, where it is 0.25563956 sigma_T
    assert_allclose(golden["sigma_peak_s"], 1.96790332, rtol=1e-8)
    assert_allclose(golden["sigma_peak"], 0.25563956, rtol=1e-7)
    assert round(float(golden["sigma_peak"]), 4) == 0.2556
    s = float(golden["sigma_peak_s"])
    assert_allclose(PC.sigma_np(s), golden["sigma_peak"], rtol=1e-14)
    assert PC.sigma_np(s * 0.99) < PC.sigma_np(s) > PC.sigma_np(s * 1.01)
    assert np.all(PC.sigma_np(np.array([0.0, 0.5, 1.0])) == 0.0)
    # the Thomson-like limits: sigma -> (3/8) sigma_T b at the threshold, (3/8)(ln 4s - 1)/s far above
    d = 2.0 ** -34
    assert_allclose(PC.sigma_np(1.0 + d), 3.0 / 8.0 * np.sqrt(d), rtol=1e-9)
    assert_allclose(PC.sigma_np(1e8), 3.0 / 8.0 * (np.log(4e8) - 1.0) / 1e8, rtol=1e-7)


@pytest.mark.parametrize("eta", [0.05, 0.9, 30.0])
def test_single_integral_identity(eta):
    import mpmath as mp
    with mp.workdps(25):
        a, b = PC.iso_mp(eta), PC.iso_single_mp(eta)
        assert abs(a - b) <= mp.mpf(10) ** -20 * abs(a)


def test_tabulated_rule_drops_both_segments_of_a_zero_node():
    E = 3e14  # eV: the threshold on eps is m^2 / E = 8.7e-4 eV
    eps = np.array([1e-4, 5e-4, 2e-3, 8e-3, 3e-2])
    n = np.array([50.0, 30.0, 0.0, 4.0, 1.0])
    y = n * PC.SIGMA_T * PC.sigma_bar_np(E * eps / PC.MEC2_EV ** 2)
    assert np.all(y[:2] == 0.0) and y[2] == 0.0 and np.all(y[3:] > 0.0)  # below threshold, n = 0
    only = PC.trapz_loglog_np(y[3:], eps[3:])
    assert only > 0.0
    assert PC.dtau_dl_table(E, eps, n)[0] == only
    # with the node filled in, its two segments come back
    n2 = n.copy()
    n2[2] = 10.0
    assert PC.dtau_dl_table(E, eps, n2)[0] > only


def test_constants_and_cmb_opacity():
    # k_B from the radiation constant is CODATA's 1.380649e-16 erg/K
    assert_allclose(PC.K_B_ERG, 1.380649e-16, rtol=1e-9)
    Tcmb = 2.72548
    tau = PC.dtau_dl_thermal(2.2e15, Tcmb, PC.AR_CGS * Tcmb ** 4) * 8.5 * PC.KPC_CM
    assert 1.15 < float(tau) < 1.25
    # theta = 0: nothing above the threshold; 180 degrees at eta is twice sigma's Planck average
    assert PC.ang_np(3.0, 0.0) == 0.0
    assert PC.dtau_dl_thermal(2.2e15, Tcmb, 1e-12, theta_rad=0.0) == 0.0


def test_constructor_grammar_units_and_errors():
    import naima_amd as na
    u = na.u
    m = na.PairAbsorptionModel(["CMB", "FIR", ["star", 2e4 * u.K, 10 * u.erg / u.cm ** 3,
                                                 120 * u.deg],
                                ["line", 1 * u.eV, 2 * u.eV / u.cm ** 3],
                                ["tab", [1e-3, 1e-2, 1e-1] * u.eV,
                                 [3.0, 2.0, 1.0] / (u.eV * u.cm ** 3)]],
                               [8.5 * u.kpc, 8.5 * u.kpc, 1 * u.au, 1 * u.pc, 2 * u.kpc])
    assert list(m.seed_photon_fields) == ["CMB", "FIR", "star", "line", "tab"]
    assert [s["type"] for s in m.seed_photon_fields.values()] == \
        ["thermal", "thermal", "thermal", "array", "array"]
    assert m.seed_photon_fields["star"]["isotropic"] is False
    assert m.batch_size is None and not m.on_device
    assert_allclose(m.path_length[2].to("cm").value, 1.495978707e13)
    one = na.PairAbsorptionModel("CMB-FIR", 3 * u.kpc)
    assert list(one.seed_photon_fields) == ["CMB", "FIR"] and len(one.path_length) == 2
    batch = na.PairAbsorptionModel(["CMB", ["d", np.array([20.0, 30.0, 40.0]) * u.K,
                                            np.array([0.3, 0.5, 0.7]) * u.eV / u.cm ** 3]],
                                   np.array([1.0, 2.0, 3.0]) * u.kpc)
    assert batch.batch_size == 3 and not batch.on_device
    with pytest.raises(ValueError, match="inconsistent"):
        na.PairAbsorptionModel([["d", np.array([20.0, 30.0]) * u.K, 1 * u.eV / u.cm ** 3]],
                               np.array([1.0, 2.0, 3.0]) * u.kpc).batch_size
    for bad in (lambda: na.PairAbsorptionModel("CMB", -1 * u.kpc),
                lambda: na.PairAbsorptionModel("CMB", np.nan * u.kpc),
                lambda: na.PairAbsorptionModel("CMB", np.inf * u.kpc),
                lambda: na.PairAbsorptionModel("CMB", [1 * u.kpc, 2 * u.kpc]),
                lambda: na.PairAbsorptionModel([["x", -3 * u.K, 1 * u.eV / u.cm ** 3]], 1 * u.kpc),
                lambda: na.PairAbsorptionModel([["x", 0 * u.K, 1 * u.eV / u.cm ** 3]], 1 * u.kpc),
                lambda: na.PairAbsorptionModel([["x", 30 * u.K, -1 * u.eV / u.cm ** 3]], 1 * u.kpc),
                lambda: na.PairAbsorptionModel([["x", 1 * u.eV, -1 * u.eV / u.cm ** 3]], 1 * u.kpc),
                lambda: na.PairAbsorptionModel([["x", 1 * u.eV, np.nan * u.eV / u.cm ** 3]],
                                               1 * u.kpc),
                lambda: na.PairAbsorptionModel([["f%d" % i, 30 * u.K, 1 * u.eV / u.cm ** 3]
                                                for i in range(9)], 1 * u.kpc)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: na.PairAbsorptionModel("CMB", 3.0),
                lambda: na.PairAbsorptionModel("CMB", 3.0 * u.s),
                lambda: na.PairAbsorptionModel([["x", 30 * u.K, 1 * u.cm]], 1 * u.kpc),
                lambda: na.PairAbsorptionModel(["XYZ"], 1 * u.kpc)):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(NotImplementedError, match="same for every walker"):
        na.PairAbsorptionModel([["x", np.ones((3, 2)) * u.eV, 1 * u.eV / u.cm ** 3]], 1 * u.kpc)
    assert "PairAbsorptionModel" in dir(na) and na.models.PairAbsorptionModel is na.PairAbsorptionModel


def test_factor_base_class():
    from naima_amd import darray
    assert issubclass(darray.DEbl, darray.DFactor) and issubclass(darray.DPairAbs, darray.DFactor)
    for name in ("apply", "get", "__mul__", "__rmul__", "__array__", "__getitem__", "size"):
        assert hasattr(darray.DEbl, name) and hasattr(darray.DPairAbs, name)
    with pytest.raises(ValueError, match="at most 8"):
        darray.DPairAbs(None, [None] * 9, 1, 1)
