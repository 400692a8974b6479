"""GPU parity: the HIP path (through the C ABI, via naima_amd's naima-shaped classes)
against the golden vectors made by the reference and against the oracle.

Tolerance: north_star asks for float64 flux rtol <= 1e-6 per energy.  The tests
hold the kernels to 1e-9 wherever the integrand is smooth (device pow/exp/log are
1-2 ulp and the reduction order differs) and state any looser bound next to it.
"""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

RT = 1e-10  # typical achieved: 1e-13 (1e-11 in exponentially suppressed tails)


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()  # fails loudly when the .so or the GPU is missing
    return naima_amd


def _pds(na):
    u = na.u
    return {
        "PowerLaw": na.PowerLaw(3e30 / u.eV, 2 * u.TeV, 2.3),
        "ExponentialCutoffPowerLaw": na.ExponentialCutoffPowerLaw(
            3e30 / u.eV, 2 * u.TeV, 2.3, 30 * u.TeV, 1.7),
        "BrokenPowerLaw": na.BrokenPowerLaw(3e30 / u.eV, 2 * u.TeV, 0.5 * u.TeV, 1.6, 2.9),
        "ExponentialCutoffBrokenPowerLaw": na.ExponentialCutoffBrokenPowerLaw(
            3e30 / u.eV, 2 * u.TeV, 0.5 * u.TeV, 1.6, 2.9, 80 * u.TeV, 0.8),
        "LogParabola": na.LogParabola(3e30 / u.eV, 2 * u.TeV, 2.1, 0.15),
    }


def test_integration_md_stub_is_executable(na, golden):
    """INTEGRATION.md section 1 -- the ctypes stub a naima maintainer would add as
    src/naima/_hip.py to put Synchrotron._spectrum (radiative.py:282-342) behind the C ABI -- is
    extracted from the document and EXECUTED as it stands (only the library's path is made
    absolute), and its synchrotron_batch gives the reference's own numbers: units.npz
    `syn_ecpl`, made by naima's Synchrotron(ECPL, B = 1 mG, 100 GeV .. 1 PeV).flux(E, 0)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "INTEGRATION.md")).read()
    block = re.search(r"```python\n(.*?)```", txt, re.S).group(1)
    assert "def synchrotron_batch" in block and '"libnaima_hip.so"' in block
    block = block.replace('"libnaima_hip.so"', repr(os.path.join(root, "naima_amd", "libnaima_hip.so")))
    ns = {}
    exec(compile(block, "INTEGRATION.md#1", "exec"), ns)
    U = golden("units")
    rows = np.array([[3e30, 2e12, 2.3, 30e12, 1.7, 0.0, 0.0, 0.0],
                     [3e30, 2e12, 2.3, 30e12, 1.7, 0.0, 0.0, 0.0]])
    spec = ns["synchrotron_batch"](rows, np.array([1e-3, 1e-3]), np.asarray(U["grid_2"]),
                                   np.asarray(U["E"]))
    assert spec.shape == (2, len(U["E"]))
    for r in spec:
        assert_allclose(r, U["syn_ecpl"], rtol=RT, atol=1e-300)


def test_abi_trapz_loglog(na, golden):
    """row 1 straight through the C ABI, incl. zero nodes / sign changes / b=-1"""
    from naima_amd._lib import get_context
    U = golden("units")
    ctx = get_context()
    x = U["tz_x"]
    y = U["tz_y"]
    out = ctx.empty((len(y),))
    ctx.call("nh_trapz_loglog", ctx.array(y), ctx.array(x), len(y), x.size, out)
    assert_allclose(out.get(), U["tz_out"], rtol=1e-12)
    yy = np.ascontiguousarray(U["tz_y2d"].T)
    out = ctx.empty((len(yy),))
    ctx.call("nh_trapz_loglog", ctx.array(yy), ctx.array(x), len(yy), x.size, out)
    assert_allclose(out.get(), U["tz_out2d"], rtol=1e-12)


def test_abi_integrate_tables_edges(na, golden):
    """the u/l segment form used by every reduction reproduces trapz_loglog's edge
    semantics: w = x*y with K = 1"""
    from naima_amd._lib import get_context
    U = golden("units")
    ctx = get_context()
    x, Y = U["tz_x"], U["tz_y"]
    n = x.size
    with np.errstate(all="ignore"):
        w = Y * x
        lw = np.zeros_like(w)
        lw[:, :-1] = np.log(np.abs(w[:, 1:] / w[:, :-1]))
    K = np.ones((n, 1))
    xd = ctx.array(x)
    lx = ctx.empty((n - 1,))
    ctx.call("nh_grid_logratio", xd, n, lx)
    out = ctx.empty((len(Y), 1))
    ctx.call("nh_integrate_tables", ctx.array(w), ctx.array(lw), len(Y), n, lx, ctx.array(K),
             ctx.array(np.zeros((n, 1))), 1, None, out, 1, 0, 1)
    assert_allclose(out.get()[:, 0], U["tz_out"], rtol=1e-13)


def test_particle_distributions(na, golden):
    U = golden("units")
    e = U["pd_e"] * na.u.eV
    for k, pd in _pds(na).items():
        # x**p is evaluated as exp(p ln x) on the device: 1e-15 where the spectrum
        # matters, up to t*1e-15 deep in the exponential cutoff exp(-t) (t ~ 400 here)
        assert_allclose(pd(e).to("1/eV").value, U["pd_" + k], rtol=2e-12)


def test_synchrotron_and_We(na, golden):
    u = na.u
    U = golden("units")
    pds = _pds(na)
    E = U["E"] * u.eV
    eprops = {"Eemin": 100 * u.GeV, "Eemax": 1 * u.PeV}
    for tag, k in (("ecpl", "ExponentialCutoffPowerLaw"), ("bpl", "BrokenPowerLaw"),
                   ("lp", "LogParabola")):
        sy = na.Synchrotron(pds[k], B=1 * u.mG, **eprops)
        assert_allclose(sy.flux(E, 0).to("1/(s eV)").value, U["syn_" + tag], rtol=RT, atol=1e-300)
        assert_allclose(sy.We.to("erg").value, U["We_" + tag], rtol=RT)
        assert_allclose(sy.compute_We(Eemin=10 * u.TeV).to("erg").value, U["We10_" + tag],
                        rtol=RT)
    sy = na.Synchrotron(pds["ExponentialCutoffPowerLaw"])
    assert_allclose(sy.flux(E, 0).value, U["syn_default"], rtol=RT, atol=1e-300)


def test_inverse_compton(na, golden):
    u = na.u
    U = golden("units")
    pds = _pds(na)
    ECPL, BPL = pds["ExponentialCutoffPowerLaw"], pds["BrokenPowerLaw"]
    E = U["E"] * u.eV
    eprops = {"Eemin": 100 * u.GeV, "Eemax": 1 * u.PeV}
    ic = na.InverseCompton(ECPL, seed_photon_fields=["CMB", "FIR", "NIR"], **eprops)
    assert_allclose(ic.flux(E, 0).value, U["ic_3seeds"], rtol=RT, atol=1e-300)
    for j in range(3):
        assert_allclose(ic.specic[j].value, U["ic_3seeds_per"][j], rtol=RT, atol=1e-300)
        assert_allclose(ic.flux(E, 0, seed=j).value, U["ic_3seeds_per"][j], rtol=RT, atol=1e-300)
    ic = na.InverseCompton(BPL, seed_photon_fields=[["bb", 5000 * u.K, 0],
                                                    ["bb2", 40 * u.K, 2.0 * u.eV / u.cm ** 3]])
    assert_allclose(ic.flux(E, 0).value, U["ic_custom"], rtol=RT, atol=1e-300)
    for ang in (45, 90, 135):
        ic = na.InverseCompton(ECPL, seed_photon_fields=[
            ["Star", 20000 * u.K, 0.1 * u.erg / u.cm ** 3, ang * u.deg]], **eprops)
        assert_allclose(ic.flux(E, 0).value, U["ic_ani_%d" % ang], rtol=RT, atol=1e-300)
    ic = na.InverseCompton(ECPL, seed_photon_fields=[["UV", 50 * u.eV, 15 * u.eV / u.cm ** 3]],
                           **eprops)
    assert_allclose(ic.flux(E, 0).value, U["ic_mono"], rtol=RT, atol=1e-300)
    Es = U["ic_arr_E"] * u.eV
    ns = U["ic_arr_n"] * u.Unit("1/(eV cm3)")
    ic = na.InverseCompton(ECPL, seed_photon_fields=[["arr", Es, ns]], **eprops)
    assert_allclose(ic.flux(E, 0).value, U["ic_array"], rtol=RT, atol=1e-300)
    ic = na.InverseCompton(ECPL, seed_photon_fields=[["arr", Es, Es ** 2 * ns]], **eprops)
    assert_allclose(ic.flux(E, 0).value, U["ic_array_edens"], rtol=RT, atol=1e-300)
    # the same seed given per walker (SSC path, nh_ic_seed_walkers) must agree
    nsw = u.Quantity(np.stack([ns.value, 2 * ns.value]), ns.unit)
    ic = na.InverseCompton(ECPL, seed_photon_fields=[["arr", Es, nsw]], **eprops)
    f = ic.flux(E, 0).value
    assert f.shape == (2, E.size)
    assert_allclose(f[0], U["ic_array"], rtol=RT, atol=1e-300)
    assert_allclose(f[1], 2 * U["ic_array"], rtol=RT, atol=1e-300)


def test_bremsstrahlung(na, golden):
    u = na.u
    U = golden("units")
    pds = _pds(na)
    E2 = U["E_brems"] * u.eV
    from naima_amd.constants import mec2
    br = na.Bremsstrahlung(pds["ExponentialCutoffPowerLaw"], n0=2.5 / u.cm ** 3, Eemin=mec2)
    assert_allclose(br.flux(E2, 0).value, U["brems_mec2"], rtol=RT, atol=1e-300)
    br = na.Bremsstrahlung(pds["BrokenPowerLaw"])
    assert_allclose([br.weight_ee, br.weight_ep], U["brems_weights"], rtol=1e-15)
    assert_allclose(br.flux(E2, 0).value, U["brems_default"], rtol=RT, atol=1e-300)


def test_pion_decay(na, golden):
    u = na.u
    U = golden("units")
    pds = _pds(na)
    Eg = U["E_pp"] * u.eV
    for tag, k in (("ecpl", "ExponentialCutoffPowerLaw"), ("bpl", "BrokenPowerLaw")):
        p = na.PionDecay(pds[k], useLUT=True, Epmax=1 * u.PeV)
        # LUT mode: FITPACK spline with ringing (20 % tiny negative nodes); 1e-8 as the
        # oracle-vs-reference bound for this mode
        assert_allclose(p.flux(Eg, 0).value, U["pp_lut_" + tag], rtol=1e-8)
        assert_allclose(p.Wp.to("erg").value, U["Wp_" + tag], rtol=RT)
        p.useLUT = False
        assert_allclose(p.flux(Eg, 0).value, U["pp_ana_" + tag], rtol=RT)
    p = na.PionDecay(pds["ExponentialCutoffPowerLaw"], useLUT=False, nuclear_enhancement=False,
                     nh=3.0 / u.cm ** 3)
    assert_allclose(p.flux(Eg, 0).value, U["pp_nonuc"], rtol=RT)
    for hiE in ("Geant4", "SIBYLL", "QGSJET"):
        p = na.PionDecay(pds["ExponentialCutoffPowerLaw"], useLUT=False, hiEmodel=hiE)
        assert_allclose(p.flux(Eg, 0).value, U["pp_ana_" + hiE], rtol=RT)


def test_abi_pion_tables(na, golden):
    """the differential cross-section tables themselves (analytic and FITPACK LUT)"""
    from naima_amd._lib import get_context
    from naima_amd.radiative import PionDecay, _lut_spline
    U = golden("units")
    ctx = get_context()
    Ep, Eg = U["ds_Ep"], U["ds_Eg"] * 1e9
    Kt, lnKt = ctx.empty((Ep.size, Eg.size)), ctx.empty((Ep.size, Eg.size))
    ctx.call("nh_table_pion_analytic", ctx.array(Ep), Ep.size, ctx.array(Eg), Eg.size, 1, 1, Kt,
             lnKt, Eg.size)
    assert_allclose(Kt.get().T, U["ds_ana"], rtol=1e-11, atol=1e-300)
    pd = _pds(na)["PowerLaw"]
    tx, ty, cf = _lut_spline(PionDecay(pd)._lut_file())
    ctx.call("nh_table_pion_lut", ctx.array(Ep), Ep.size, ctx.array(Eg), Eg.size, ctx.array(tx),
             tx.size, ctx.array(ty), ty.size, ctx.array(cf), Kt, lnKt, Eg.size)
    # atol: the spline rings at the 1e-41 level where the table is identically zero
    assert_allclose(Kt.get().T, U["ds_lut"], rtol=1e-9, atol=1e-40)


def test_lnprobmodel_and_priors(na, golden):
    u = na.u
    U = golden("units")
    flux = U["ll_flux"] * u.Unit("1/(cm2 s TeV)")
    d = dict(energy=U["ll_energy_TeV"] * u.TeV, flux=flux, flux_error_lo=0.1 * flux,
             flux_error_hi=0.2 * flux, ul=U["ll_ul"], cl=U["ll_cl"])
    models = U["ll_models"] * u.Unit("1/(cm2 s TeV)")
    assert_allclose(na.lnprobmodel(models, d), U["ll_out"], rtol=1e-12)
    assert_allclose(na.lnprobmodel(models[2], d), U["ll_out"][2], rtol=1e-12)
    sed = (models * d["energy"] ** 2).to("erg/(cm2 s)")
    assert_allclose(na.lnprobmodel(sed, d), U["ll_out_sedmodel"], rtol=1e-12)
    assert_allclose(na.normal_prior(1.3, 1.0, 0.5), U["prior_normal"][0])
    assert_allclose(na.log_uniform_prior(2.0, 1.0, 3.0), U["prior_logu"][0])


def test_lnprobmodel_confidence_level_indexed_by_violations(na, golden):
    """lnprob.npz: asymmetric errors, five upper limits, a distinct cl per point, models violating
    0 .. 4 of them -- the likelihood kernel against the reference, batched and one row at a time"""
    u = na.u
    z = golden("lnprob")
    fu = u.Unit("1/(cm2 s TeV)")
    d = dict(energy=z["energy_TeV"] * u.TeV, flux=z["flux"] * fu,
             flux_error_lo=z["flux_error_lo"] * fu, flux_error_hi=z["flux_error_hi"] * fu,
             ul=z["ul"], cl=z["cl"])
    models = z["models"] * fu
    assert_allclose(na.lnprobmodel(models, d), z["lnprobmodel"], rtol=1e-12)
    for i in (1, 4):
        assert_allclose(na.lnprobmodel(models[i], d), z["lnprobmodel"][i], rtol=1e-12)


def _data_from_npz(na, z, prefix="data_"):
    from naima_amd.datatable import make_data
    return make_data({k: z[prefix + k] for k in ("energy", "energy_unit", "flux", "flux_error_lo",
                                                  "flux_error_hi", "ul", "cl", "flux_unit")})


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_workloads_batched_and_single(na, golden, name):
    """the five BASELINE workloads: flux, blob and lnprob for the fixture walkers,
    evaluated as ONE batch (pars[ndim, N]) and one walker at a time"""
    from naima_amd import workloads as W
    z = golden(name)
    data = _data_from_npz(na, z)
    model = W.WORKLOADS[name]["model"](na)
    pars = z["pars"]
    tol = 1e-8 if name == "cfg5" else RT  # cfg5 default = LUT mode
    res = na.lnprob(pars.T, data, model, None)
    flux = res[1].to("1/(s cm2 eV)").value
    assert flux.shape == z["flux"].shape
    assert_allclose(flux, z["flux"], rtol=tol, atol=1e-300)
    assert_allclose(res[0], z["lnprob"], rtol=1e-7)
    if not np.isnan(z["blob"][0]):
        assert_allclose(res[2].to("erg").value, z["blob"], rtol=RT)
    one = na.lnprob(pars[1], data, model, None)
    assert_allclose(one[1].to("1/(s cm2 eV)").value, z["flux"][1], rtol=tol, atol=1e-300)
    assert_allclose(one[0], z["lnprob"][1], rtol=1e-7)
    prior = W.prior_for(name, na)
    if prior is not None:
        assert_allclose(prior(pars.T), z["lnprior"])
    if name == "cfg5":
        model = W.WORKLOADS[name]["model"](na, useLUT=False)
        data = _data_from_npz(na, z, "analytic_data_")
        res = na.lnprob(pars.T, data, model, None)
        assert_allclose(res[1].to("1/(s cm2 eV)").value, z["flux_analytic"], rtol=RT)
        assert_allclose(res[0], z["lnprob_analytic"], rtol=1e-7)


def test_cfg3_against_oracle_random_walkers(na, golden):
    """256 seeded walkers around p0: HIP batch vs the NumPy oracle, per energy"""
    from naima_amd import workloads as W
    from oracle import workloads_np as WN
    z = golden("cfg3")
    raw = WN.raw_from_npz(z)
    data = _data_from_npz(na, z)
    model = W.WORKLOADS["cfg3"]["model"](na)
    rng = np.random.default_rng(7)
    p0 = np.asarray(W.WORKLOADS["cfg3"]["p0"])
    pars = p0 * (1 + 0.02 * rng.standard_normal((256, p0.size)))
    res = na.lnprob(pars.T, data, model, W.prior_for("cfg3", na))
    flux = res[1].to("1/(s cm2 eV)").value
    for i in range(0, 256, 16):
        lp, f, We = WN.lnprob("cfg3", pars[i], raw)
        assert_allclose(flux[i], f, rtol=RT, atol=1e-300)
        assert_allclose(res[0][i], lp, rtol=1e-7)
        assert_allclose(res[2].to("erg").value[i], We, rtol=RT)


def test_errors_and_shapes(na):
    u = na.u
    ECPL = na.ExponentialCutoffPowerLaw(1e36 / u.eV, 10 * u.TeV, 2.5, 50 * u.TeV)
    ic = na.InverseCompton(ECPL, seed_photon_fields=["CMB", ["test", 5000 * u.K, 0]])
    ene = np.logspace(-3, 0, 5) * u.TeV
    assert_allclose(ic.sed(ene, seed="test").value, ic.sed(ene, seed=1).value)
    with pytest.raises(ValueError):
        ic.sed(ene, seed="FIR")
    with pytest.raises(ValueError):
        ic.sed(ene, seed=10)
    with pytest.raises(TypeError):
        na.Synchrotron(ECPL, B=1 * u.TeV)
    with pytest.raises(TypeError):
        na.InverseCompton(ECPL, seed_photon_fields=["XYZ"])
    sy = na.Synchrotron(ECPL, B=np.array([1.0, 2.0, 3.0]) * u.uG)
    assert sy.flux(ene).shape == (3, 5)
    assert sy.flux(ene[2]).shape == (3,)
    assert na.Synchrotron(ECPL).flux(ene).shape == (5,)
    # flux <-> sed <-> distance identities (tests/test_models.py:291-324 of the reference)
    d1, d2 = 2.5 * u.kpc, 10.0 * u.kpc
    f1, f2 = ic.flux(ene, d1).value, ic.flux(ene, d2).value
    assert_allclose(f1 / f2, 16.0)
    assert_allclose(ic.sed(ene, d1).value,
                    (ic.flux(ene, 0) * ene ** 2).to("erg/s").value
                    / (4 * np.pi * d1.to("cm").value ** 2))
    W = 1e49 * u.erg
    sy = na.Synchrotron(ECPL)
    sy.set_We(W, 1 * u.GeV, 100 * u.TeV)
    assert_allclose(sy.compute_We(1 * u.GeV, 100 * u.TeV).value, W.value, rtol=1e-12)


# ---------------------------------------------------------------------------
# device-resident step loop: lazy device parameters, fused prior+likelihood,
# hipGraph replay -- must reproduce the host-driven sampler step for step
# ---------------------------------------------------------------------------
def _cfg_problem(na, golden, name):
    from naima_amd import workloads as W
    z = golden(name)
    data = _data_from_npz(na, z)
    return W.WORKLOADS[name]["model"](na), data, W.prior_for(name, na), np.asarray(
        W.WORKLOADS[name]["p0"], dtype=float)


def test_lazy_device_values(na):
    from naima_amd._lib import get_context
    from naima_amd.darray import DPars
    ctx = get_context()
    host = np.random.default_rng(0).uniform(0.5, 2.0, size=(3, 40))
    P = DPars(ctx, ctx.array(host), 3, 40)
    u = na.u
    assert_allclose(np.asarray(10 ** P[0]), 10 ** host[0], rtol=1e-15)
    assert_allclose(np.asarray((10 ** P[0] / u.eV).to("1/TeV").value), 10 ** host[0] * 1e12,
                    rtol=1e-15)
    assert_allclose(np.asarray(P[1] * 3 + 2), host[1] * 3 + 2, rtol=1e-15)
    assert_allclose(np.asarray(2 / (P[1] * 4)), 2 / (host[1] * 4), rtol=1e-15)
    assert_allclose(np.asarray((P[1] - 1.0) ** 2), (host[1] - 1) ** 2, rtol=1e-14)
    assert_allclose(np.asarray(np.log10(P[2]) + np.exp(-P[1])), np.log10(host[2]) + np.exp(
        -host[1]), rtol=1e-14)
    assert_allclose(np.asarray(P[0] * P[1] / P[2]), host[0] * host[1] / host[2], rtol=1e-15)
    assert_allclose(np.asarray(2.5 ** P[0]), 2.5 ** host[0], rtol=1e-14)
    lp = (na.uniform_prior(P[0], 0.7, 1.5) + na.normal_prior(P[1], 1.0, 0.5)
          + na.log_uniform_prior(P[2], 0.6, 1.9) + 0.25).evaluate()
    ref = (np.where((0.7 <= host[0]) & (host[0] <= 1.5), 0, -np.inf)
           + (-0.5 * (2 * np.pi * 0.5) - (host[1] - 1) ** 2 / (2 * 0.5))
           + np.where((host[2] >= 0.6) & (host[2] <= 1.9), 1 / host[2], -np.inf) + 0.25)
    assert_allclose(np.asarray(lp), ref, rtol=1e-14)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_device_lnprob_equals_host_lnprob(na, golden, name):
    """the same unchanged model function on device-resident parameters"""
    from naima_amd._lib import get_context
    from naima_amd.darray import DPars
    model, data, prior, p0 = _cfg_problem(na, golden, name)
    z = golden(name)
    pars = z["pars"]
    n = len(pars)
    host = na.lnprob(pars.T, data, model, prior)
    ctx = get_context()
    P = DPars(ctx, ctx.array(np.ascontiguousarray(pars.T)), pars.shape[1], n)
    dev = na.lnprob(P, data, model, prior)
    assert_allclose(np.asarray(dev[0]), host[0], rtol=1e-12)
    assert_allclose(np.asarray(dev[1].to("1/(s cm2 eV)").value),
                    host[1].to("1/(s cm2 eV)").value, rtol=1e-13, atol=1e-300)
    if len(host) > 2 and hasattr(host[2], "unit"):
        assert_allclose(np.asarray(dev[2].to("erg").value), host[2].to("erg").value, rtol=1e-13)


@pytest.mark.parametrize("use_graph", [False, True])
def test_device_sampler_matches_host_sampler(na, golden, use_graph):
    from naima_amd.sampler import EnsembleSampler
    model, data, prior, p0 = _cfg_problem(na, golden, "cfg3")
    kw = dict(args=[data, model, prior], seed=42, naima_style=True)
    h = EnsembleSampler(32, 5, na.lnprob, **kw)
    d = EnsembleSampler(32, 5, na.lnprob, device=True, use_graph=use_graph, **kw)
    pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((32, 5)))
    sh = h.run_mcmc(pos, 6)
    sd = d.run_mcmc(pos, 6)
    assert_allclose(sd.coords, sh.coords, rtol=1e-9)
    assert_allclose(sd.log_prob, sh.log_prob, rtol=1e-7)
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-9)
    assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-7)
    assert_allclose(d.acceptance_fraction, h.acceptance_fraction)
    bh, bd = h.get_blobs(), d.get_blobs()
    assert bd[0].shape == bh[0].shape == (6, 32, 64)
    assert_allclose(bd[0], bh[0], rtol=1e-9, atol=1e-300)
    assert_allclose(bd[1], bh[1], rtol=1e-9)
    if use_graph:
        assert d._dev.graph is not None or d._dev.resident_launches > 0
    # continuing from the device state does not re-upload or re-evaluate
    sd2 = d.run_mcmc(sd, 3)
    sh2 = h.run_mcmc(sh, 3)
    assert_allclose(sd2.coords, sh2.coords, rtol=1e-9)


def test_rccl_single_rank_allgather(na):
    """the RCCL path of the C ABI (dlopen, communicator, all-gather on the context's
    stream) with a 1-rank communicator -- all a 1-GPU box can exercise"""
    import ctypes as C

    from naima_amd import _lib
    lib = _lib.load()
    ctx = _lib.Context(0)  # its own context: a communicator is bound to it
    buf = C.create_string_buffer(128)
    _lib._chk(lib.nh_comm_unique_id(buf))
    _lib._chk(lib.nh_comm_init(ctx.h, 0, 1, buf.raw))
    x = np.arange(16, dtype=float)
    send, recv = ctx.array(x), ctx.empty((16,))
    ctx.call("nh_comm_allgather", send, recv, 16)
    assert_allclose(recv.get(), x)
    _lib._chk(lib.nh_comm_destroy(ctx.h))
    ctx.close()


def test_rccl_communicator_after_torch_import(na):
    """bench.py's order of events: torch.distributed (gloo) first, then the RCCL
    communicator.  PyTorch bundles its own librccl and HIP runtime; the communicator must
    come from the RCCL of the runtime libnaima_hip is linked against (a dlopen by soname
    returned PyTorch's copy and ncclCommInitRank failed).  Also: the all-gather survives
    hipGraph capture and replay.  Separate process: it initialises a process group."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29800 + os.getpid() % 100),
               RANK="0", WORLD_SIZE="1")
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "rccl_graph_probe.py")],
                         cwd=root, env=env, timeout=300, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "eager ok: True" in out.stdout
    assert "captured + replayed ok: True" in out.stdout


@pytest.mark.parametrize("in_graph", ["0", "1", "auto"])
def test_sharded_path_with_rccl_on_one_rank(na, golden, tmp_path, in_graph):
    """everything of the multi-GPU loop except the second process: torch.distributed
    rendezvous, RCCL communicator, split graphs with the all-gathers between them, the
    likelihood written into the send buffer, accept after the exchange, gathered blobs --
    with a one-rank communicator, against the ordinary single-GPU loop.  in_graph = 1: the
    variant with the all-gathers captured into the step graphs; auto (the default): after
    the probe process has seen that work."""
    import subprocess
    import sys
    from naima_amd.sampler import EnsembleSampler
    from bench import build_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29900 + os.getpid() % 90),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", NAIMA_AMD_RCCL_IN_GRAPH=in_graph)
    out = subprocess.run([sys.executable, os.path.join(root, "tests",
                                                       "gpu_sharded_one_rank_worker.py"),
                          str(tmp_path)], cwd=root, env=env, timeout=600, capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    s = EnsembleSampler(64, 5, na.lnprob, args=[data, model, prior], seed=42, naima_style=True,
                        store_blobs=True, device=True)
    pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((64, 5)))
    st = s.run_mcmc(pos, 4)
    st = s.run_mcmc(st, 40)
    assert_allclose(np.load(tmp_path / "chain.npy"), s.get_chain(), rtol=1e-9)
    assert_allclose(np.load(tmp_path / "logp.npy"), s.get_log_prob(), rtol=1e-7)
    blobs = s.get_blobs()
    assert_allclose(np.load(tmp_path / "blob0.npy"), np.asarray(blobs[0]), rtol=1e-9, atol=1e-300)
    assert_allclose(np.load(tmp_path / "blob1.npy"), np.asarray(blobs[1]), rtol=1e-9)
    s2 = EnsembleSampler(64, 5, na.lnprob, args=[data, model, prior], seed=42, naima_style=True,
                         store_blobs=False, device=True)
    st2 = s2.run_mcmc(pos, 4)
    st2 = s2.run_mcmc(st2, 70)
    assert_allclose(np.load(tmp_path / "chain_noblobs.npy"), s2.get_chain(), rtol=1e-9)
    assert_allclose(np.load(tmp_path / "final_noblobs.npy"), st2.coords, rtol=1e-9)


def test_abi_move_kernels(na):
    """nh_move_propose / nh_move_accept / nh_scatter_rows against their NumPy twins, on
    the second slice of a two-half-step block (cursor = 1)"""
    from naima_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(3)
    N, ndim, ns = 24, 3, 12
    coords = rng.normal(size=(N, ndim))
    logp = rng.normal(size=N)
    perm = rng.permutation(N)
    S, Cset = perm[:ns], perm[ns:]
    partner = Cset[rng.integers(ns, size=ns)]
    z = ((2 - 1.0) * rng.random(ns) + 1) ** 2 / 2
    lnu = np.log(rng.random(ns))
    blk_h = np.zeros((2, 3 * ns))
    blk_h[1, :ns], blk_h[1, ns:2 * ns] = z, lnu
    iv = blk_h[:, 2 * ns:].view(np.int32)
    iv[1, :ns], iv[1, ns:] = S, partner
    blk = ctx.array(blk_h)
    cursor = ctx.array(np.array([1], dtype=np.int32), dtype=np.int32)
    cd, ld = ctx.array(coords.ravel()), ctx.array(logp)
    qT, fac = ctx.empty((ndim * ns,)), ctx.empty((ns,))
    ctx.call("nh_move_propose", cd, blk, cursor, ns, ndim, 0, ns, qT, fac)
    q = coords[partner] - (coords[partner] - coords[S]) * z[:, None]
    # the device contracts c - (c - s) z into an fma: last-bit differences
    assert_allclose(qT.get().reshape(ndim, ns).T, q, rtol=1e-13, atol=1e-15)
    assert_allclose(fac.get(), (ndim - 1) * np.log(z), rtol=1e-15)
    newlp = rng.normal(size=ns)
    acc = ctx.empty((ns,), dtype=np.int32)
    sel = ctx.empty((ns,), dtype=np.int32)
    nacc = ctx.array(np.zeros(N, dtype=np.int32), dtype=np.int32)
    ctx.call("nh_move_accept", cd, ld, blk, cursor, ctx.array(newlp), ns, ndim, acc, nacc, sel, 1)
    ok = lnu < (ndim - 1) * np.log(z) + newlp - logp[S]
    ref_c, ref_l = coords.copy(), logp.copy()
    ref_c[S[ok]], ref_l[S[ok]] = q[ok], newlp[ok]
    assert_allclose(acc.get(), ok.astype(int))
    assert_allclose(sel.get(), S)
    assert cursor.get()[0] == 2
    assert_allclose(cd.get().reshape(N, ndim), ref_c, rtol=1e-13, atol=1e-15)
    assert_allclose(ld.get(), ref_l)
    assert nacc.get().sum() == ok.sum()
    dst = ctx.array(np.zeros((N, 4)))
    src = rng.normal(size=(ns, 4))
    ctx.call("nh_scatter_rows", dst, 4, ctx.array(src), 4, sel, acc, 0, ns, 4)
    ref = np.zeros((N, 4))
    ref[S[ok]] = src[ok]
    assert_allclose(dst.get(), ref)


def test_abi_step_front_and_lnprob_accept(na):
    """nh_step_front (proposal + packs + particle weights + We reduction + history +
    cursor) against the separate entry points, then nh_lnprob_accept against
    nh_lnprob + nh_move_accept"""
    import ctypes as C
    from naima_amd._lib import get_context
    from naima_amd.darray import (nh_accept, nh_comp, nh_grid, nh_lazy, nh_moment, nh_pack,
                                  lazy_const)
    ctx = get_context()
    rng = np.random.default_rng(5)
    N, ndim, ns = 16, 3, 8
    coords = np.column_stack([rng.normal(33.0, 0.05, N), rng.normal(2.4, 0.05, N),
                              rng.normal(1.6, 0.05, N)])
    logp = rng.normal(size=N)
    blk_h = np.zeros((4, 3 * ns))
    iv = blk_h[:, 2 * ns:].view(np.int32)
    sl = []
    for h in range(3):
        perm = rng.permutation(N)
        S, partner = perm[:ns], perm[ns:][rng.integers(ns, size=ns)]
        z = (rng.random(ns) + 1) ** 2 / 2
        lnu = np.log(rng.random(ns))
        blk_h[h, :ns], blk_h[h, ns:2 * ns] = z, lnu
        iv[h, :ns], iv[h, ns:] = S, partner
        sl.append((S, partner, z, lnu))
    blk = ctx.array(blk_h)
    cursor = ctx.array(np.array([1], dtype=np.int32), dtype=np.int32)  # slice 1 accepted last
    done = ctx.array(np.zeros(1, dtype=np.int32), dtype=np.int32)
    cd, ld = ctx.array(coords.ravel()), ctx.array(logp)
    qT, fac = ctx.empty((ndim * ns,)), ctx.empty((ns,))
    # ECPL rows: amplitude = 10**q0 / eV, e0 = 1e13 eV, alpha = q1, ecut = 10**q2 TeV, beta 1
    cols = (nh_lazy * 8)()
    for j in range(8):
        cols[j] = lazy_const(0.0)
    cols[0] = nh_lazy(qT.ptr, 1, 1.0, 1.0, 0.0, 1, 0)
    cols[1] = lazy_const(1e13)
    cols[2] = nh_lazy(qT.ptr + 8 * ns, 1, 1.0, 1.0, 0.0, 0, 0)
    cols[3] = nh_lazy(qT.ptr + 16 * ns, 1, 1e12, 1.0, 0.0, 1, 0)
    cols[4] = lazy_const(1.0)
    rows = ctx.empty((ns, 8))
    pk = (nh_pack * 1)()
    pk[0].cols, pk[0].ncols, pk[0].ld, pk[0].out = cols, 8, 8, rows.ptr
    gam = np.logspace(3, 8, 120)
    e_eV = gam * 510998.9499961643
    gd, ed = ctx.array(gam), ctx.array(e_eV)
    lne, lx = ctx.array(np.log(e_eV)), ctx.empty((gam.size - 1,))
    ctx.call("nh_grid_logratio", gd, gam.size, lx)
    w, dlw = ctx.empty((ns, gam.size)), ctx.empty((ns, gam.size))
    grids = (nh_grid * 1)()
    grids[0] = nh_grid(ed.ptr, gd.ptr, w.ptr, dlw.ptr, 510998.9499961643, gam.size, 0, lne.ptr,
                       lx.ptr)
    K = gam * 8.187105776823886e-07
    Kt, dK = ctx.array(K), ctx.array(np.append(np.log(K[1:] / K[:-1]), 0.0))
    We = ctx.empty((ns, 1))
    mm = (nh_moment * 1)()
    mm[0] = nh_moment(0, 0, Kt.ptr, dK.ptr, We.ptr)
    hc, hl = ctx.array(np.zeros((2, N * ndim))), ctx.array(np.zeros((2, N)))
    hist = ctx.array(np.array([hc.ptr, hl.ptr, 1, 2], dtype=np.int64), dtype=np.int64)
    ctx.call("nh_step_front", cd, ld, blk, cursor, done, ns, ndim, 0, ns, qT, fac, pk, 1, 1,
             rows, grids, 1, mm, 1, hist)
    S, partner, z, lnu = sl[2]
    q = coords[partner] - (coords[partner] - coords[S]) * z[:, None]
    assert cursor.get()[0] == 2 and done.get()[0] == 0
    assert_allclose(qT.get().reshape(ndim, ns).T, q, rtol=1e-13)
    assert_allclose(fac.get(), (ndim - 1) * np.log(z), rtol=1e-15)
    rows_ref = np.zeros((ns, 8))
    rows_ref[:, 0], rows_ref[:, 1], rows_ref[:, 2] = 10 ** q[:, 0], 1e13, q[:, 1]
    rows_ref[:, 3], rows_ref[:, 4] = 1e12 * 10 ** q[:, 2], 1.0
    assert_allclose(rows.get(), rows_ref, rtol=1e-12)
    # history row 1 = the ensemble as it stood (cursor was odd: a step had closed)
    assert_allclose(hist.get(), [hc.ptr, hl.ptr, 2, 2])
    assert_allclose(hc.get()[1], coords.ravel())
    assert_allclose(hl.get()[1], logp)
    # the separate entry points on the rows the front kernel packed
    w2, dlw2, We2 = ctx.empty((ns, gam.size)), ctx.empty((ns, gam.size)), ctx.empty((ns, 1))
    ctx.call("nh_particle_weights", 1, rows, ns, ed, gd, gam.size, 510998.9499961643, w2, dlw2,
             None)
    ctx.call("nh_integrate_tables", w2, dlw2, ns, gam.size, lx, Kt, dK, 1, None, We2, 1, 0, 1)
    assert_allclose(w.get(), w2.get(), rtol=5e-13)
    assert_allclose(dlw.get(), dlw2.get(), rtol=1e-11, atol=1e-14)
    assert_allclose(We.get(), We2.get(), rtol=1e-12)

    # ---- nh_lnprob_accept == nh_lnprob followed by nh_move_accept (slice 2) ----------
    nE = 7
    comp = rng.random((ns, nE)) + 0.5
    cdv = ctx.array(comp)
    comps = (nh_comp * 1)()
    comps[0] = nh_comp(cdv.ptr, nE, 1.0)
    one = ctx.array(np.ones(nE))
    flux, err = ctx.array(rng.random(nE) + 0.5), ctx.array(np.full(nE, 0.3))
    ul = ctx.array(np.zeros(nE, dtype=np.int32), dtype=np.int32)
    cl = ctx.array(np.full(nE + 1, 0.9))
    tot_ref = ctx.empty((ns,))
    ctx.call("nh_lnprob", comps, 1, ns, nE, one, flux, err, err, ul, cl, None, None, 0, None,
             tot_ref)
    c2, l2 = ctx.array(coords.ravel()), ctx.array(logp)
    acc2 = ctx.empty((ns,), dtype=np.int32)
    sel2 = ctx.empty((ns,), dtype=np.int32)
    nacc2 = ctx.array(np.zeros(N, dtype=np.int32), dtype=np.int32)
    ctx.call("nh_move_accept", c2, l2, blk, cursor, tot_ref, ns, ndim, acc2, nacc2, sel2, 0)
    acc1 = ctx.empty((ns,), dtype=np.int32)
    sel1 = ctx.empty((ns,), dtype=np.int32)
    nacc1 = ctx.array(np.zeros(N, dtype=np.int32), dtype=np.int32)
    tot = ctx.empty((ns,))
    mv = nh_accept(cd.ptr, ld.ptr, blk.ptr, cursor.ptr, ns, ndim, 0, 0, acc1.ptr, nacc1.ptr,
                   sel1.ptr)
    ctx.call("nh_lnprob_accept", comps, 1, ns, nE, one, flux, err, err, ul, cl, None, None, 0,
             None, tot, C.addressof(mv))
    assert_allclose(tot.get(), tot_ref.get(), rtol=0)
    assert 0 <= acc1.get().sum() <= ns
    assert_allclose(acc1.get(), acc2.get())
    assert_allclose(sel1.get(), sel2.get())
    assert_allclose(nacc1.get(), nacc2.get())
    assert_allclose(cd.get(), c2.get(), rtol=0)
    assert_allclose(ld.get(), l2.get(), rtol=0)
    assert cursor.get()[0] == 2


def test_abi_last_producer_epilogues(na):
    """nh_synchrotron_lnprob and nh_integrate_tables_lnprob (the likelihood + accept as the
    epilogue of the last producer) against the separate entry points on the same inputs.  The
    table half covers nh_integrate_tables_lnprob's FALLBACK: N * nE = 480 < 1024 takes
    k_integrate_rows, which cannot carry the likelihood, so the entry point launches it
    separately (test_gpu_integrate.py::test_fused_epilogue_is_reached has the fused launch)"""
    import ctypes as C
    from naima_amd._lib import get_context
    from naima_amd.constants import MEC2_EV
    from naima_amd.darray import nh_accept, nh_comp
    ctx = get_context()
    rng = np.random.default_rng(8)
    N, ndim, ns, nE = 12, 3, 12, 40
    gam = np.logspace(3, 8.5, 150)
    e_eV = gam * MEC2_EV
    rows = np.zeros((N, 8))
    rows[:, 0] = 10 ** rng.normal(33, 0.1, N)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = 1e13, rng.uniform(2, 3, N), 5e13, 1.0
    gd, ed, rd = ctx.array(gam), ctx.array(e_eV), ctx.array(rows)
    w, dlw, lx = ctx.empty((N, gam.size)), ctx.empty((N, gam.size)), ctx.empty((gam.size - 1,))
    ctx.call("nh_particle_weights", 1, rd, N, ed, gd, gam.size, MEC2_EV, w, dlw, None)
    ctx.call("nh_grid_logratio", gd, gam.size, lx)
    E = np.geomspace(1e2, 1e5, nE)
    Ed, Bd = ctx.array(E), ctx.array(rng.uniform(5, 50, N) * 1e-6)
    other = ctx.array(rng.random((N, nE)) * 1e20)
    conv = ctx.array(np.ones(nE))
    flux, err = ctx.array(rng.random(nE) * 1e21), ctx.array(np.full(nE, 3e20))
    ulh = np.zeros(nE, dtype=np.int32)
    ulh[-2:] = 1
    ul, cl = ctx.array(ulh, dtype=np.int32), ctx.array(np.full(nE + 1, 0.9))
    coords, logp = rng.normal(size=(2 * ns, ndim)), rng.normal(-50, 5, 2 * ns)
    blk_h = np.zeros((1, 3 * ns))
    perm = rng.permutation(2 * ns)
    blk_h[0, :ns], blk_h[0, ns:2 * ns] = (rng.random(ns) + 1) ** 2 / 2, np.log(rng.random(ns))
    iv = blk_h[:, 2 * ns:].view(np.int32)
    iv[0, :ns], iv[0, ns:] = perm[:ns], perm[ns:][rng.integers(ns, size=ns)]
    logp[perm[:ns:2]] = -1e300  # every other active walker accepts whatever comes
    blk = ctx.array(blk_h)
    cursor = ctx.array(np.zeros(1, dtype=np.int32), dtype=np.int32)

    def state():
        return (ctx.array(coords.ravel()), ctx.array(logp), ctx.empty((ns,), dtype=np.int32),
                ctx.array(np.zeros(2 * ns, dtype=np.int32), dtype=np.int32),
                ctx.empty((ns,), dtype=np.int32))

    def mv_of(st):
        return nh_accept(st[0].ptr, st[1].ptr, blk.ptr, cursor.ptr, ns, ndim, 0, 0, st[2].ptr,
                         st[3].ptr, st[4].ptr)

    def comps_of(out, scale):
        c = (nh_comp * 2)()
        c[0], c[1] = nh_comp(other.ptr, nE, 1.0), nh_comp(out.ptr, nE, scale)
        return c

    def same(a, b):
        for x, y in zip(a, b):
            assert_allclose(x.get(), y.get(), rtol=1e-13)

    # ---- synchrotron -----------------------------------------------------------------
    o1, o2, t1, t2 = ctx.empty((N, nE)), ctx.empty((N, nE)), ctx.empty((N,)), ctx.empty((N,))
    s1, s2 = state(), state()
    m1, m2 = mv_of(s1), mv_of(s2)
    sa = (w, dlw, Bd, 1, N, gd, lx, gam.size, Ed, nE)
    ctx.call("nh_synchrotron", *sa, o1, nE)
    ctx.call("nh_lnprob_accept", comps_of(o1, 0.5), 2, N, nE, conv, flux, err, err, ul, cl, None,
             None, 0, None, t1, C.addressof(m1))
    ctx.call("nh_synchrotron_lnprob", *sa, o2, nE, comps_of(o2, 0.5), 2, 1, conv, flux, err, err,
             ul, cl, None, None, 0, t2, C.addressof(m2))
    assert_allclose(o2.get(), o1.get(), rtol=0)
    assert_allclose(t2.get(), t1.get(), rtol=1e-12)
    same(s1, s2)
    assert 0 < s1[2].get().sum() <= ns
    # ---- table reduction (one tile, one plane) ------------------------------------------
    K = rng.random((gam.size, nE)) + 0.1
    dK = np.zeros_like(K)
    dK[:-1] = np.log(K[1:] / K[:-1])
    Kt, dKt, sc = ctx.array(K), ctx.array(dK), ctx.array(rng.random(nE) + 0.5)
    s1, s2 = state(), state()
    m1, m2 = mv_of(s1), mv_of(s2)
    ia = (w, dlw, N, gam.size, lx, Kt, dKt, nE, sc)
    ctx.call("nh_integrate_tables", *ia, o1, nE, 1, 1)
    ctx.call("nh_lnprob_accept", comps_of(o1, 2.0), 2, N, nE, conv, flux, err, err, ul, cl, None,
             None, 0, None, t1, C.addressof(m1))
    ctx.call("nh_integrate_tables_lnprob", *ia, o2, nE, 1, comps_of(o2, 2.0), 2, 1, conv, flux, err,
             err, ul, cl, None, None, 0, t2, C.addressof(m2))
    assert_allclose(o2.get(), o1.get(), rtol=0)
    assert_allclose(t2.get(), t1.get(), rtol=1e-12)
    same(s1, s2)


def test_device_loop_front_kernel_history_and_multistep_graph(na, golden, monkeypatch):
    """store_blobs=False, the per-launch loop (NAIMA_AMD_RESIDENT=0: what a sharded run and
    plans the resident loop declines use): one k_half_step launch per half-step, the chain
    history kept on the device across block boundaries (32 steps), eight steps replayed per
    graph launch; the chain equals the host loop's"""
    from naima_amd.sampler import EnsembleSampler
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    model, data, prior, p0 = _cfg_problem(na, golden, "cfg3")
    kw = dict(args=[data, model, prior], seed=7, naima_style=True, store_blobs=False)
    h = EnsembleSampler(32, 5, na.lnprob, **kw)
    d = EnsembleSampler(32, 5, na.lnprob, device=True, **kw)
    pos = p0 * (1 + 0.003 * np.random.default_rng(2).standard_normal((32, 5)))
    sh = h.run_mcmc(pos, 3)
    sd = d.run_mcmc(pos, 3)
    assert d._dev.fused
    sh = h.run_mcmc(sh, 45)
    sd = d.run_mcmc(sd, 45)
    assert d._dev.multi_graph is not None and d._dev.resident_launches == 0
    assert d.get_chain().shape == (48, 32, 5)
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-8)
    assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-6)
    assert_allclose(d.acceptance_fraction, h.acceptance_fraction)
    # a generator consumer sees every step (no multi-step launches)
    n = sum(1 for _ in d.sample(sd, iterations=5))
    assert n == 5 and d.get_chain().shape == (53, 32, 5)


def test_graph_scratch_is_never_handed_out_again(na, golden):
    """buffers a captured graph writes on every replay stay out of the pool: foreign
    allocations of every bucket size, filled with NaN between two runs, change nothing"""
    from naima_amd._lib import get_context
    from naima_amd.sampler import EnsembleSampler
    model, data, prior, p0 = _cfg_problem(na, golden, "cfg3")
    kw = dict(args=[data, model, prior], seed=3, naima_style=True, store_blobs=False)
    h = EnsembleSampler(64, 5, na.lnprob, **kw)
    d = EnsembleSampler(64, 5, na.lnprob, device=True, **kw)
    pos = p0 * (1 + 0.003 * np.random.default_rng(4).standard_normal((64, 5)))
    sh, sd = h.run_mcmc(pos, 12), d.run_mcmc(pos, 12)
    ctx = get_context()
    junk = []
    for nb in [2 ** k for k in range(8, 23)]:
        for _ in range(3):
            junk.append(ctx.array(np.full(nb // 8, np.nan)))
    sh, sd = h.run_mcmc(sh, 12), d.run_mcmc(sd, 12)
    for a in junk:
        assert np.isnan(a.get()).all()  # and the graph did not write into them either
    assert_allclose(sd.coords, sh.coords, rtol=1e-9)
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-9)


@pytest.mark.parametrize("name", ["cfg3", "cfg4"])
def test_device_loop_two_ranks_one_gpu(na, golden, tmp_path, name):
    """walker sharding of the device-resident loop with 2 processes (gloo stands in for
    RCCL, which refuses two ranks on one GPU): split graphs around the exchange, same
    ensemble on both ranks and equal to the single-process run.  cfg3: the one-launch half-step
    around the all-gather; cfg4 (BASELINE's 4-GPU configuration): the separate kernels with the
    SSC seed integral, sharded the same way"""
    import subprocess
    import sys
    from naima_amd.sampler import EnsembleSampler
    from bench import build_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29700 + (os.getpid() % 1000)
    subprocess.check_call(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         os.path.join(root, "tests", "gpu_two_ranks_worker.py"), str(tmp_path), name],
        cwd=root, timeout=600, env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    c0, c1 = np.load(tmp_path / "coords_0.npy"), np.load(tmp_path / "coords_1.npy")
    assert_allclose(c0, c1, rtol=1e-12)
    model, p0, raw, data, prior, labels = build_problem(name, na)
    nd = p0.size
    s = EnsembleSampler(32, nd, na.lnprob, args=[data, model, prior], seed=42, naima_style=True,
                        store_blobs=True, device=True)
    pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((32, nd)))
    st = s.run_mcmc(pos, 6)
    assert_allclose(c0, st.coords, rtol=1e-9)
    assert_allclose(np.load(tmp_path / "logp_0.npy"), st.log_prob, rtol=1e-7)
    assert_allclose(np.load(tmp_path / "chain_1.npy"), s.get_chain(), rtol=1e-9)
    # blobs (model spectra, We) are kept on every rank although a walker's evaluating
    # rank changes from step to step
    blobs = s.get_blobs()
    assert len(blobs) >= 1
    for r in (0, 1):
        for b, x in enumerate(blobs):
            assert_allclose(np.load(tmp_path / ("blob%d_%d.npy" % (b, r))), np.asarray(x, dtype=float),
                            rtol=1e-9, atol=1e-300, equal_nan=True)
    s2 = EnsembleSampler(32, nd, na.lnprob, args=[data, model, prior], seed=42, naima_style=True,
                         store_blobs=False, device=True)
    st2 = s2.run_mcmc(pos, 3)
    st2 = s2.run_mcmc(st2, 37 if name != "cfg4" else 9)
    for r in (0, 1):
        assert_allclose(np.load(tmp_path / ("chain_noblobs_%d.npy" % r)), s2.get_chain(), rtol=1e-9)


def test_edge_shapes_against_oracle(na):
    """ragged and extreme sizes: minimum grid (10 nodes), a 3000-node grid (LDS staging
    above 64 KB in the synchrotron kernel), odd walker counts, one photon energy, photon
    energies that are all dead for synchrotron, and a batch of one"""
    from oracle import naima_np as O
    u = na.u
    rng = np.random.default_rng(11)

    def check(N, nE, Eemin_eV, Eemax_eV, nEed, Elo, Ehi, B0):
        E = np.geomspace(Elo, Ehi, nE) if nE > 1 else np.array([Elo])
        amp = 10 ** (33 + 0.05 * rng.standard_normal(N))
        alpha = 2.3 + 0.1 * rng.standard_normal(N)
        B = B0 * (1 + 0.05 * rng.standard_normal(N))
        sq = (lambda v: v[0]) if N == 1 else (lambda v: v)
        pd = na.ExponentialCutoffPowerLaw(sq(amp) / u.eV, 10 * u.TeV, sq(alpha), 30 * u.TeV)
        kw = dict(Eemin=Eemin_eV * u.eV, Eemax=Eemax_eV * u.eV, nEed=nEed)
        Eq = E * u.eV if nE > 1 else E[0] * u.eV
        syn = na.Synchrotron(pd, B=sq(B) * u.uG, **kw).flux(Eq, 0).value
        ic = na.InverseCompton(pd, seed_photon_fields=["CMB", "NIR"], **kw).flux(Eq, 0).value
        syn, ic = np.asarray(syn).reshape(N, nE), np.asarray(ic).reshape(N, nE)
        gam = O.electron_grid(Eemin_eV, Eemax_eV, nEed)
        for i in sorted(set([0, N // 2, N - 1])):
            opd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=amp[i], e_0=1e13,
                                 alpha=alpha[i], e_cutoff=30e12, beta=1.0)
            ne = O.nelec_on(opd, gam)
            # RT down to 200 orders of magnitude below the peak; further out in the
            # exp(-x) tail (x ~ 700) the relative error grows like x * 1e-15 (checked at 1e-6)
            ref = O.synchrotron_spectrum(E, gam, ne, B[i] * 1e-6)
            assert_allclose(syn[i], ref, rtol=RT, atol=ref.max() * 1e-200)
            assert_allclose(syn[i], ref, rtol=1e-6, atol=1e-300)
            ref, _ = O.ic_spectrum(E, gam, ne, [O.thermal_seed("CMB"), O.thermal_seed("NIR")])
            assert_allclose(ic[i], ref, rtol=RT, atol=ref.max() * 1e-200)

    check(N=3, nE=5, Eemin_eV=1e9, Eemax_eV=1.5e9, nEed=100, Elo=1e-6, Ehi=1e-3, B0=10.0)  # 17 -> min grid
    check(N=1, nE=1, Eemin_eV=1e9, Eemax_eV=1e15, nEed=100, Elo=2e3, Ehi=2e3, B0=12.0)
    check(N=257, nE=70, Eemin_eV=1e10, Eemax_eV=1e13, nEed=1000, Elo=1e-2, Ehi=1e12, B0=50.0)  # 3000 nodes
    check(N=5, nE=7, Eemin_eV=1e9, Eemax_eV=1e14, nEed=30, Elo=1e12, Ehi=1e14, B0=3.0)  # synchrotron all dead
    check(N=64, nE=130, Eemin_eV=1e8, Eemax_eV=5e16, nEed=10, Elo=1e-5, Ehi=1e13, B0=100.0)  # coarse grid


@pytest.mark.parametrize("tabulated", ["1", "0"])
def test_ssc_seed_edge_shapes_against_oracle(na, tabulated, monkeypatch):
    """nh_ic_seed_walkers_tab (the kernel tabulated once per set of grids: what a fit runs) and
    nh_ic_seed_walkers (the kernel evaluated per call: when the table does not fit) -- a seed
    density per walker, radiative.py:609-655 + 684 -- at the shapes
    their mapping cares about: 1 / 9 / 17 / 33 walkers (groups of 8 and of 16, padded groups), a
    seed spectrum of two nodes, seed nodes with ZERO density (the trapz_loglog zero rule,
    utils.py:347-348) at the ends and in the middle, a density that is the same at every node, a particle grid shorter than a wave's 64
    nodes and one that needs several gamma tiles, one photon energy"""
    from oracle import naima_np as O
    from naima_amd._lib import get_context
    monkeypatch.setenv("NAIMA_AMD_SSC_TABLE", tabulated)
    u = na.u
    rng = np.random.default_rng(3)
    ctx, seen = get_context(), []
    orig = ctx.call
    monkeypatch.setattr(ctx, "call", lambda name, *a: (seen.append(name), orig(name, *a))[1])

    def check(N, ns, nE, Eemin_eV, Eemax_eV, nEed, zeros=(), empty=(), flat=()):
        E = np.geomspace(1e3, 3e13, nE) if nE > 1 else np.array([2e9])
        se = np.geomspace(1e-6, 1e4, ns)
        base = 1e3 * (se / 1e-2) ** -1.4 * np.exp(-se / 2e3)
        sd = base[None, :] * 10 ** (0.3 * rng.standard_normal((N, ns)))
        for z in zeros:
            sd[:, z] = 0.0
        if zeros and N > 2:
            sd[1, ns // 3] = 0.0  # ... and a zero that only one walker has
        for wz in empty:  # walkers WITHOUT a seed field: packed out of the groups (k_ssc_order)
            sd[wz, :] = 0.0
        for wf in flat:  # the SAME density at every node: the walker's log-ratios are exact zeros
            sd[wf, :] = 7.0
        amp = 10 ** (33 + 0.05 * rng.standard_normal(N))
        alpha = 2.3 + 0.1 * rng.standard_normal(N)
        pd = na.ExponentialCutoffPowerLaw(amp / u.eV, 10 * u.TeV, alpha, 30 * u.TeV)
        seed = ["ssc", se * u.eV, u.Quantity(sd, u.Unit("1/(eV cm3)"))]
        ic = na.InverseCompton(pd, seed_photon_fields=[seed], Eemin=Eemin_eV * u.eV,
                               Eemax=Eemax_eV * u.eV, nEed=nEed)
        got = np.asarray(ic.flux(E * u.eV if nE > 1 else E[0] * u.eV, 0).value).reshape(N, nE)
        gam = O.electron_grid(Eemin_eV, Eemax_eV, nEed)
        for i in sorted(set([0, 1 % N, N // 2, N - 1])):
            opd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=amp[i], e_0=1e13,
                                 alpha=alpha[i], e_cutoff=30e12, beta=1.0)
            ne = O.nelec_on(opd, gam)
            ref = O.ic_seed_spectrum(E, gam, ne, dict(type="array", energy=se, density=sd[i]))
            assert_allclose(got[i], ref, rtol=RT, atol=np.abs(ref).max() * 1e-200)
        for wz in empty:
            assert np.all(got[wz] == 0.0)
        if empty:  # ... and their neighbours in the packed order are the walkers they were
            for i in sorted(set(range(N)) - set(empty))[::7]:
                opd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=amp[i], e_0=1e13,
                                     alpha=alpha[i], e_cutoff=30e12, beta=1.0)
                ref = O.ic_seed_spectrum(E, gam, O.nelec_on(opd, gam),
                                         dict(type="array", energy=se, density=sd[i]))
                assert_allclose(got[i], ref, rtol=RT, atol=np.abs(ref).max() * 1e-200)

    check(N=1, ns=12, nE=9, Eemin_eV=1e9, Eemax_eV=1e14, nEed=20)
    check(N=9, ns=2, nE=5, Eemin_eV=1e9, Eemax_eV=1e13, nEed=10)        # two seed nodes, 40 nodes
    check(N=17, ns=30, nE=70, Eemin_eV=1e8, Eemax_eV=1e15, nEed=40, zeros=(0, 29, 11))  # 280 nodes
    check(N=33, ns=25, nE=1, Eemin_eV=1e9, Eemax_eV=1.5e9, nEed=100, zeros=(5,))  # 17 -> 10 nodes
    check(N=8, ns=40, nE=66, Eemin_eV=1e10, Eemax_eV=1e13, nEed=100)      # 300 nodes, 5 tiles
    check(N=20, ns=40, nE=30, Eemin_eV=1e9, Eemax_eV=1e14, nEed=40, flat=(0, 19))
    check(N=150, ns=33, nE=19, Eemin_eV=1e9, Eemax_eV=1e14, nEed=30, zeros=(2,))  # 10 groups: two chunks
    # walkers without a seed density (what a proposal the prior forbids hands over): some, scattered
    # -- the last group of the packed order is mixed --, all but one, and every one
    check(N=40, ns=20, nE=7, Eemin_eV=1e9, Eemax_eV=1e13, nEed=30, empty=(0, 3, 4, 17, 38, 39))
    check(N=40, ns=20, nE=7, Eemin_eV=1e9, Eemax_eV=1e13, nEed=30, empty=tuple(set(range(40)) - {21}))
    check(N=9, ns=20, nE=7, Eemin_eV=1e9, Eemax_eV=1e13, nEed=30, empty=tuple(range(9)))
    check(N=1100, ns=8, nE=3, Eemin_eV=1e9, Eemax_eV=1e11, nEed=20, empty=tuple(range(5, 1100, 3)))
    assert ("nh_ic_seed_walkers_tab" in seen) == (tabulated == "1")
    assert ("nh_ic_seed_walkers" in seen) == (tabulated == "0")


def test_ssc_tabulated_kernel_against_the_evaluated_one(na, monkeypatch):
    """k_ssc_table restates what k_ic_seed_walkers evaluates per step: the two entry points
    agree to rounding (cfg4-like grids, 40 walkers; zero seed nodes)"""
    u = na.u
    rng = np.random.default_rng(8)
    N, ns, nE = 40, 100, 37
    E = np.geomspace(1e-5, 1e14, nE)
    se = np.geomspace(1e-7, 1e9, ns)
    sd = 1e3 * (se / 1e-2) ** -1.6 * np.exp(-se / 1e5) * 10 ** (0.2 * rng.standard_normal((N, ns)))
    sd[:, 0] = 0.0
    sd[3, 50] = 0.0
    amp = 10 ** (33 + 0.05 * rng.standard_normal(N))
    out = {}
    for tab in ("1", "0"):
        monkeypatch.setenv("NAIMA_AMD_SSC_TABLE", tab)
        pd = na.ExponentialCutoffPowerLaw(amp / u.eV, 10 * u.TeV, 2.4, 300 * u.TeV)
        ic = na.InverseCompton(pd, seed_photon_fields=[
            ["ssc", se * u.eV, u.Quantity(sd, u.Unit("1/(eV cm3)"))]],
            Eemin=1e8 * u.eV, Eemax=1e15 * u.eV, nEed=60)
        out[tab] = np.asarray(ic.flux(E * u.eV, 0).value)
    assert np.isfinite(out["1"]).all() and (out["1"] > 0).any()
    rel = np.abs(out["1"] - out["0"]) / np.abs(out["0"]).max(axis=1, keepdims=True)
    print("tabulated vs evaluated: max |diff| / max|row| = %.3g, identical %d of %d" %
          (rel.max(), (out["1"] == out["0"]).sum(), out["0"].size))
    assert_allclose(out["1"], out["0"], rtol=1e-13, atol=0)


def test_abi_table_interleave(na):
    """nh_table_interleave: {K, dlnK} pairs; a sign change between two non-zero nodes -> NaN (the
    NaN exponent of utils.py:336-345); with the grid's lx the log-ratios come in units of
    ln(x2/x1) (b + 1 of utils.py:336-339 itself), the zero marker and the NaN untouched"""
    from naima_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(4)
    nG, nK = 37, 5
    K = 10 ** rng.uniform(-30, 3, (nG, nK))
    K[:, 1] *= np.where(rng.random(nG) < 0.3, -1.0, 1.0)   # a column that changes sign
    K[[0, 7, 8, 36], 2] = 0.0                              # zero nodes
    x = np.geomspace(3.0, 2e9, nG) * (1 + 0.01 * rng.random(nG)).cumprod()
    lxh = np.log(x[1:] / x[:-1])
    with np.errstate(all="ignore"):
        dK = np.zeros_like(K)
        dK[:-1] = np.log(np.abs(K[1:] / K[:-1]))
    zero = np.zeros_like(K, dtype=bool)
    zero[:-1] = (K[:-1] == 0) | (K[1:] == 0)
    dK[zero] = 1e300                                        # k_table_dlog's marker
    flip = np.zeros_like(zero)
    flip[:-1] = (K[:-1] * K[1:] < 0)
    Kd, dKd = ctx.array(K), ctx.array(dK)
    lx = ctx.array(lxh)
    for with_lx in (False, True):
        kd = ctx.empty((2 * nG * nK,))
        ctx.call("nh_table_interleave", Kd, dKd, lx if with_lx else None, nG, nK, kd)
        got = kd.get().reshape(nG, nK, 2)
        assert np.array_equal(got[..., 0], K)
        d = got[..., 1]
        assert np.all(np.isnan(d[flip])) and not np.any(np.isnan(d[~flip]))
        assert np.all(d[zero] == 1e300)
        want = dK.copy()
        if with_lx:
            want[:-1] /= lxh[:, None]
        ok = ~flip & ~zero
        ok[-1] = False  # (the last row has no segment)
        assert_allclose(d[ok], want[ok], rtol=2e-16)


def test_synchrotron_grid_too_long_for_lds_is_an_error(na):
    """k_synchrotron stages three grid arrays in LDS (150 KB: 5034 nodes); a longer particle grid
    must come back as a NaimaHipError that says so, not as a launch failure or a wrong answer"""
    from naima_amd._lib import NaimaHipError
    u = na.u
    pd = na.ExponentialCutoffPowerLaw(1e33 / u.eV, 10 * u.TeV, 2.3, 30 * u.TeV)
    syn = na.Synchrotron(pd, B=10 * u.uG, Eemin=1 * u.GeV, Eemax=1 * u.PeV, nEed=1000)  # 6000 nodes
    with pytest.raises(NaimaHipError, match="LDS"):
        syn.flux(np.geomspace(1e-3, 1e4, 5) * u.eV, 0)
    ok = na.Synchrotron(pd, B=10 * u.uG, Eemin=1 * u.GeV, Eemax=1 * u.PeV, nEed=800)  # 4800 nodes
    assert np.all(np.isfinite(ok.flux(np.geomspace(1e-3, 1e4, 5) * u.eV, 0).value))
