"""GPU tests of nh_pp_leptons_kelner06 (naima_amd/csrc/nh_kelner_leptons.hip) and of
SecondaryLeptonsKelner06: the neutrinos and secondary electrons of pp collisions after Kelner,
Aharonian & Bugayov 2006.  The reference project has no counterpart, so the kernel is held to
tests/kelner_leptons_np.py -- adaptive quad split at every kink, pinned to the paper and
certified by mpmath in tests/test_kelner_leptons_host.py -- at the 1e-8 of the gamma-ray kernel
(tests/test_gpu_kelner.py), on every distribution kind, all four products and both sides of three
transition energies; to properties that need no reference; at the C entry point; and as a blob
of a device-resident fit."""
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kelner_cases as KC
import kelner_leptons_np as KL
from oracle import naima_np as O

pytestmark = pytest.mark.gpu

RTOL = 1e-8  # the kernel's documented distance from the converged integral
PRODUCTS = ("electron", "nu_e", "nu_mu", "nu_all")  # the entry point's 0..3
ENTRY = "nh_pp_leptons_kelner06"


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


@pytest.fixture(scope="module")
def ctx(na):
    from naima_amd import _lib
    return _lib.get_context()


def energies(Etrans_eV):
    """50 MeV (below m_pi: the clamp), 1 and 50 GeV, the two sides of Etrans, 1, 30, 300 TeV"""
    below = np.nextafter(Etrans_eV, 0)
    assert below * 1e-12 < Etrans_eV * 1e-12  # still apart in TeV, where the branch is chosen
    return np.unique([5e7, 1e9, 5e10, below, Etrans_eV, 1e12, 3e13, 3e14])


def _flux(na, k, E_eV):
    return np.atleast_2d(k.flux(E_eV * na.u.eV, 1 * na.u.kpc).to("1/(s cm2 eV)").value)


def _model(na, kind, product, Etrans_eV=1e11, nh=2.0, sets=None):
    u = na.u
    sets = KC.SETS[kind] if sets is None else sets
    return na.SecondaryLeptonsKelner06(KC.amd_pd(na, kind, [p for _, p in sets]),
                                       nh=nh / u.cm ** 3, Etrans=Etrans_eV * u.eV, product=product)


# ---------------------------------------------------------------------------------------
# against the converged reference
# ---------------------------------------------------------------------------------------
CASES = [(kind, 1e11) for kind in KC.SETS] + [(kind, Etr) for kind in KC.SETS if "Broken" in kind
                                              for Etr in (1e10, 1e12)]


@pytest.mark.parametrize("kind, Etrans_eV", CASES)
def test_converged_integrals(na, kind, Etrans_eV):
    """all four products and the three nhat of every parameter set of one kind (one walker
    each, one launch per product) within 1e-8 of the converged reference at 50 MeV ... 300 TeV,
    including both neighbours of Etrans; and the continuity at Etrans that nhat exists to give
    (measured figures: profiles/NOTES_kelner_leptons.md)"""
    tags = [t for t, _ in KC.SETS[kind]]
    E = energies(Etrans_eV)
    full = E * 1e-12 >= Etrans_eV * 1e-12
    lo, hi = np.flatnonzero(~full)[-1], np.flatnonzero(full)[0]  # the two sides of Etrans
    bad = []
    for product in PRODUCTS:
        k = _model(na, kind, product, Etrans_eV)
        f = _flux(na, k, E)
        nhat = np.atleast_2d(k.nhat)
        assert nhat.shape == (len(tags), 3)
        for j, tag in enumerate(tags):
            spec, ref_nhat = KL.spectrum(tag, E, Etrans_eV, product)
            err = np.abs(f[j] / O.to_flux(2.0 * spec, O.KPC_CM) - 1)
            errs = {"full": err[full].max(), "delta": err[~full].max(),
                    "nhat": np.abs(nhat[j] / ref_nhat - 1).max(),
                    "step at Etrans": abs(f[j, lo] / f[j, hi] - 1)}
            print("K06LERR %-12s %-8s Etrans %.0e eV: " % (tag, product, Etrans_eV)
                  + "  ".join("%s %.1e" % kv for kv in errs.items())
                  + "  (worst at %.6g eV)" % E[err.argmax()])
            bad += ["%s %s %s %.1e" % (tag, product, what, e) for what, e in errs.items()
                    if not e <= RTOL]
    assert not bad, bad


# ---------------------------------------------------------------------------------------
# properties that need no reference
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bpl_products(na):
    """the four products of the three broken power laws at the energies of Etrans = 1e11 eV"""
    E = energies(1e11)
    return E, {p: _flux(na, _model(na, "BrokenPowerLaw", p), E) for p in PRODUCTS}


def test_products_are_sums_of_components(bpl_products):
    """nu_all = nu_mu + nu_e (the products' table: all flavours are the two flavours), and the
    pion decay's own muon neutrino, nu_mu - electron, is the same whichever products it is formed
    from: sums of the same three numbers in another order, 1e-14 of the largest of them"""
    E, f = bpl_products
    assert all(np.all(v > 0) for v in f.values())
    assert_allclose(f["nu_all"], f["nu_mu"] + f["nu_e"], rtol=1e-14)
    numu1 = f["nu_mu"] - f["electron"]
    assert np.all(np.abs(f["nu_all"] - f["nu_e"] - f["electron"] - numu1) <= 1e-14 * f["nu_all"])
    assert np.all(f["nu_mu"] > f["electron"])


@pytest.mark.parametrize("kind", ["PowerLaw", "BrokenPowerLaw"])
def test_one_sided_energies(na, kind):
    """all energies above Etrans: nhat == 1 exactly and nu_e is the electrons' spectrum to the
    bit.  All below: the delta branch is matched all the same (unlike PionDecayKelner06), so
    the two one-sided calls are the two-sided one, and meet across Etrans"""
    E = energies(1e11)
    lo, hi = E[E < 1e11], E[E >= 1e11]
    above = {}
    for product in PRODUCTS:
        k = _model(na, kind, product)
        both = _flux(na, k, E)
        nhat_both = np.atleast_2d(k.nhat).copy()
        f_hi = _flux(na, k, hi)
        assert_array_equal(np.atleast_2d(k.nhat), 1.0)
        f_lo = _flux(na, k, lo)
        assert_array_equal(np.atleast_2d(k.nhat), nhat_both)
        assert np.all(nhat_both != 1.0)
        assert_array_equal(np.concatenate([f_lo, f_hi], axis=1), both)
        assert_allclose(f_lo[:, -1], f_hi[:, 0], rtol=RTOL)  # nextafter(Etrans, 0) | Etrans
        above[product] = f_hi
    assert_array_equal(above["nu_e"], above["electron"])


def test_linear_in_amplitude_and_density_batched_as_alone(na):
    """broken power laws: walkers in one launch == one at a time; the spectrum is linear in
    the amplitude and in nh (a product after the quadrature: a rounding or two each)"""
    u = na.u
    E = energies(1e11)
    amp = np.array([4e35, 1e35, 9e35, 12e35])
    nh = np.array([2.0, 1.0, 0.5, 6.0])
    par = dict(e_break=np.array([3.7e12, 2e10, KC.E_EDGE, 3.7e12]) * u.eV,
               alpha_1=np.array([1.8, 2.0, 1.8, 1.8]), alpha_2=np.array([2.9, 2.6, 2.9, 2.9]))
    kb = na.SecondaryLeptonsKelner06(
        na.BrokenPowerLaw(amp / u.eV, 1 * u.TeV, par["e_break"], par["alpha_1"], par["alpha_2"]),
        nh=nh / u.cm ** 3, product="nu_all")
    fb = _flux(na, kb, E)
    nb = kb.nhat
    assert nb.shape == (4, 3)
    for j in range(4):
        kj = na.SecondaryLeptonsKelner06(
            na.BrokenPowerLaw(amp[j] / u.eV, 1 * u.TeV, par["e_break"][j], par["alpha_1"][j],
                              par["alpha_2"][j]), nh=nh[j] / u.cm ** 3, product="nu_all")
        assert_allclose(fb[j], _flux(na, kj, E)[0], rtol=1e-13)
        assert kj.nhat.shape == (3,)
        assert_allclose(nb[j], kj.nhat, rtol=1e-13)
    # walker 3 is walker 0 with three times the amplitude and three times the density
    assert_allclose(fb[3], 9 * fb[0], rtol=1e-13)
    assert_allclose(nb[3], nb[0], rtol=1e-13)  # (ratios of two integrals, each linear)


@pytest.mark.parametrize("alpha, e_g, numu_g", [(2.0, 0.42443, 0.74802), (2.5, 0.33315, 0.55332),
                                                (3.0, 0.26487, 0.41219)])
def test_power_law_ratios_to_gamma(na, alpha, e_g, numu_g):
    """electrons / gamma rays and muon neutrinos / gamma rays of a pure power law at 1 TeV, the
    gamma rays from PionDecayKelner06: the pins of tests/test_kelner_leptons_host.py"""
    u = na.u
    pl = na.PowerLaw(1e36 / u.eV, 1 * u.TeV, alpha)
    gam = na.PionDecayKelner06(pl)
    g = gam.flux(1 * u.TeV, 1 * u.kpc).value
    e = gam.secondaries("electron").flux(1 * u.TeV, 1 * u.kpc).value
    m = gam.secondaries().flux(1 * u.TeV, 1 * u.kpc).value
    assert_allclose(e / g, e_g, rtol=1e-4)
    assert_allclose(m / g, numu_g, rtol=1e-4)


# ---------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------
E9 = np.array([5e7, 2e8, 1e9, np.nextafter(1e11, 0), 1e11, 1e12, 5e10, 3e13, 3e14])
SENTINEL = -7.25
NU_ALL = 3


def _rows(na, ctx):
    """three BPL walkers and the kind's enum value"""
    from naima_amd._lib import PD_KIND
    pd = KC.amd_pd(na, "BrokenPowerLaw", [p for _, p in KC.SETS["BrokenPowerLaw"]])
    return pd.device_rows(ctx, 3, amplitude_to=na.u.Unit("1/eV")), PD_KIND[pd.kind]


def _call(ctx, kind, rows, N, E, nE, ldo, Etr=1e11, match=1, product=NU_ALL, nhat=True, Nbuf=3):
    out = ctx.array(np.full((Nbuf, ldo), SENTINEL))
    nh = ctx.array(np.full((Nbuf, 3), SENTINEL)) if nhat else None
    ctx.call(ENTRY, kind, rows, N, ctx.array(E), nE, Etr, match, product, out, ldo, nh)
    return out.get(), None if nh is None else nh.get()


@pytest.fixture(scope="module")
def nine(na, ctx):
    rows, kind = _rows(na, ctx)
    out, nhat = _call(ctx, kind, rows, 3, E9, 9, 9)
    for j, (tag, _) in enumerate(KC.SETS["BrokenPowerLaw"]):
        spec, ref_nhat = KL.spectrum(tag, E9, 1e11, "nu_all")
        assert_allclose(out[j], spec, rtol=RTOL)
        assert_allclose(nhat[j], ref_nhat, rtol=RTOL)
    return out, nhat


@pytest.mark.parametrize("nE", [1, 2, 3, 4, 5, 9])
def test_entry_task_loop_and_padding(na, ctx, nine, nE):
    """nE + 2 tasks over four waves, ldo = nE + 3: a task's arithmetic does not depend on
    which wave runs it or on nE (``match`` is an argument), so the first nE columns are the
    nine-energy call's to the bit; the padding is not written"""
    rows, kind = _rows(na, ctx)
    out, nhat = _call(ctx, kind, rows, 3, E9[:nE], nE, nE + 3)
    assert_array_equal(out[:, :nE], nine[0][:, :nE])
    assert_array_equal(out[:, nE:], SENTINEL)
    assert_array_equal(nhat, nine[1])


def test_entry_optional_output_products_and_repeat(na, ctx, nine):
    rows, kind = _rows(na, ctx)
    for nhat in (False, True):
        out, n = _call(ctx, kind, rows, 3, E9, 9, 9, nhat=nhat)
        assert_array_equal(out, nine[0])  # (two identical calls, identical bits)
        if nhat:
            assert_array_equal(n, nine[1])
    # match = 0: no normalisation, whatever the energies
    out, n = _call(ctx, kind, rows, 3, E9, 9, 9, match=0)
    assert_array_equal(n, 1.0)
    full = E9 * 1e-12 >= 1e11 * 1e-12  # (in TeV, as the kernel decides it)
    assert_array_equal(out[:, full], nine[0][:, full])
    assert np.all(out[:, ~full] != nine[0][:, ~full])
    # every product has the same three nhat; electron is component 0 alone
    for product in range(3):
        o, n = _call(ctx, kind, rows, 3, E9, 9, 9, product=product)
        assert_array_equal(n, nine[1])
    e0, _ = _call(ctx, kind, rows, 3, E9, 9, 9, product=0, match=0)
    e1, _ = _call(ctx, kind, rows, 3, E9, 9, 9, product=0)
    assert_allclose(e0[:, ~full] * nine[1][:, :1], e1[:, ~full], rtol=1e-15)
    # fewer walkers than the buffers hold: the rows beyond N are not written
    out, n = _call(ctx, kind, rows, 2, E9, 9, 9)
    assert_array_equal(out[:2], nine[0][:2])
    assert_array_equal(out[2], SENTINEL)
    assert_array_equal(n[2], SENTINEL)
    # N = 0 is no error and no launch
    out, n = _call(ctx, kind, rows, 0, E9, 9, 9)
    assert_array_equal(out, SENTINEL)
    assert_array_equal(n, SENTINEL)


def test_entry_refusals(na, ctx):
    """every refused call raises NaimaHipError naming the entry point and launches nothing
    (the buffers are large enough for every refused shape all the same)"""
    from naima_amd._lib import NaimaHipError
    rows, kind = _rows(na, ctx)
    cap = 60 * 1024 // (3 * 8) - 2  # the largest nE whose 3 (nE + 2) results fit 60 KiB of LDS
    E = np.geomspace(1e8, 1e14, cap + 1)
    Ed = ctx.array(E)
    for what, kw in (("kind below the enum", dict(kind=-1)), ("kind above the enum", dict(kind=5)),
                     ("product below 0", dict(product=-1)), ("product above 3", dict(product=4)),
                     ("nE = 0", dict(nE=0)), ("negative nE", dict(nE=-1)),
                     ("ldo < nE", dict(nE=9, ldo=8)), ("Etrans = 0", dict(Etr=0.0)),
                     ("Etrans < 0", dict(Etr=-1e11)), ("Etrans NaN", dict(Etr=float("nan"))),
                     ("negative N", dict(N=-1)), ("nE above the LDS cap", dict(nE=cap + 1)),
                     ("params NULL", dict(rows=None)), ("E NULL", dict(E=None)),
                     ("out NULL", dict(out=None))):
        out = ctx.array(np.full((3, cap + 1), SENTINEL))
        side = ctx.array(np.full((3, 3), SENTINEL))
        a = dict(dict(kind=kind, rows=rows, N=3, E=Ed, nE=9, ldo=cap + 1, Etr=1e11, product=2,
                      out=out), **kw)
        with pytest.raises(NaimaHipError, match=ENTRY):
            ctx.call(ENTRY, a["kind"], a["rows"], a["N"], a["E"], a["nE"], a["Etr"], 1,
                     a["product"], a["out"], a["ldo"], side)
            pytest.fail("accepted: " + what)
        assert_array_equal(out.get(), SENTINEL)
        assert_array_equal(side.get(), SENTINEL)
    # the cap itself is accepted
    o, n = _call(ctx, kind, rows, 1, E[:cap], cap, cap, Nbuf=1)
    assert np.all(o > 0) and np.all(n[0] > 0)


# ---------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------
def test_class_device_resident_and_per_walker_density(na, ctx):
    """a model whose amplitude and density live in HBM: the spectrum stays there and equals
    the host model's; nh per walker is a factor per row"""
    from naima_amd.darray import DPars
    u = na.u
    host = np.array([[35.6, 35.0, 35.9], [2.0, 1.0, 0.5]])
    P = DPars(ctx, ctx.array(host), 2, 3)
    E = energies(1e11)

    def model(amp, nh):
        return na.SecondaryLeptonsKelner06(
            na.BrokenPowerLaw(amp / u.eV, 1 * u.TeV, 3.7 * u.TeV, 1.8, 2.9), nh=nh / u.cm ** 3)
    dev, hst = model(10 ** P[0], P[1]), model(10 ** host[0], host[1])
    assert dev.on_device and not hst.on_device
    fh = hst.flux(E * u.eV, 1 * u.kpc)
    fd = dev.flux(E * u.eV, 1 * u.kpc)
    assert getattr(fd.value, "__array_priority__", 0) == 30000  # (still in HBM)
    assert_allclose(np.asarray(fd.value), fh.value, rtol=1e-13)
    assert not hasattr(dev, "nhat") and hst.nhat.shape == (3, 3)
    one = model(10 ** host[0], 1.0).flux(E * u.eV, 1 * u.kpc)
    assert_allclose(fh.value, one.value * host[1][:, None], rtol=1e-15)
    spec, _ = KL.spectrum("bpl_above", E, 1e11, "nu_mu")
    assert_allclose(fh.to("1/(s cm2 eV)").value[1],
                    O.to_flux(spec * 10 ** host[0, 1] / KC.AMP, O.KPC_CM), rtol=RTOL)
    # sed() on top of flux(), scalar energy, scalar result
    s = model(1e35, 1.0).sed(1 * u.TeV, 1 * u.kpc)
    assert np.shape(s.value) == () and s.to("erg/(cm2 s)").value > 0


def test_class_secondaries_products_and_refusals(na, golden):
    u = na.u
    pd = na.PowerLaw(4e35 / u.eV, 1 * u.TeV, 2.2)
    gam = na.PionDecayKelner06(pd, nh=np.array([2.0, 3.0]) / u.cm ** 3, Etrans=30 * u.GeV)
    sec = gam.secondaries()
    assert isinstance(sec, na.SecondaryLeptonsKelner06) and sec.product == "nu_mu"
    assert sec.particle_distribution is pd
    assert sec.Etrans.to("eV").value == gam.Etrans.to("eV").value == 3e10
    assert_array_equal(sec.nh.value, gam.nh.value)
    E = np.array([1e10, 1e12]) * u.eV
    f = sec.flux(E, 1 * u.kpc)
    assert f.shape == (2, 2)
    assert_allclose(f[1].value, 1.5 * f[0].value, rtol=1e-15)
    own = na.SecondaryLeptonsKelner06(pd, nh=2 / u.cm ** 3, Etrans=30 * u.GeV, product="nu_mu")
    assert_array_equal(own.flux(E, 1 * u.kpc).value, f[0].value)
    assert gam.secondaries("nu_all").product == "nu_all"
    for bad in ("numu", "gamma", None):
        with pytest.raises(ValueError, match="'electron', 'nu_e', 'nu_mu', 'nu_all'"):
            na.SecondaryLeptonsKelner06(pd, product=bad)
    with pytest.raises(ValueError, match="nu_all"):
        gam.secondaries("muon")
    z = golden("extra")
    tm = na.TableModel(z["tm_energy_eV"] * u.eV, z["tm_values_per_eV"] / u.eV)
    with pytest.raises(TypeError, match="analytic naima_amd.models particle distribution"):
        na.SecondaryLeptonsKelner06(tm).flux(E, 1 * u.kpc)


# ---------------------------------------------------------------------------------------
# in a fit: the muon-neutrino spectrum as a blob
# ---------------------------------------------------------------------------------------
NU_E = np.array([1e12, 1e13, 1e14, 3e14, 1e15])


def _fit_models(na):
    u = na.u

    def gamma(pars):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV)
        return na.PionDecayKelner06(pd, nh=10 / u.cm ** 3)

    def plain(pars, data):
        return gamma(pars).flux(data, distance=2 * u.kpc)

    def with_blob(pars, data):
        g = gamma(pars)
        return g.flux(data, distance=2 * u.kpc), g.secondaries("nu_mu").flux(NU_E * u.eV,
                                                                             distance=2 * u.kpc)

    def prior(pars):
        return (na.uniform_prior(pars[0], 25, 45) + na.uniform_prior(pars[1], 1, 4)
                + na.uniform_prior(pars[2], 0, 5))
    return plain, with_blob, prior


def test_in_a_fit(na, monkeypatch):
    """32 walkers x 6 steps of a hadronic fit (log amplitude, index, log cut-off) with the
    nu_mu spectrum at 5 energies as a blob: every stored blob row is the host evaluation of
    SecondaryLeptonsKelner06 at that row of the chain; and the blob does not cost the model the
    device loop if the gamma-ray model alone takes it"""
    from naima_amd.datatable import make_data
    from naima_amd.sampler import EnsembleSampler
    u = na.u
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")  # (the recorded plan, as test_gpu_pairabs.py)
    plain, with_blob, prior = _fit_models(na)
    p0 = np.array([35.0, 2.1, 2.5])
    E = np.geomspace(3e11, 3e14, 12)
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    sed = (plain(p0, make_data(raw)) * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    raw["flux"] = sed * (1 + 0.1 * np.random.default_rng(5).standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.1 * sed
    data = make_data(raw)
    nw, steps = 32, 6
    pos = p0 + np.array([0.03, 0.01, 0.02]) * np.random.default_rng(3).standard_normal((nw, 3))

    def run(model, blobs):
        s = EnsembleSampler(nw, 3, na.lnprob, args=[data, model, prior], seed=17,
                            naima_style=True, store_blobs=blobs, device=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            s.run_mcmc(pos, steps)
        fell_back = [str(x.message) for x in w if "host-driven loop" in str(x.message)]
        return s, fell_back

    s0, fell_back0 = run(plain, False)
    s, fell_back = run(with_blob, True)
    print("gamma-ray model alone: %s; with the neutrino blob: %s"
          % (("host-driven loop: " + fell_back0[0]) if fell_back0 else "device loop",
             ("host-driven loop: " + fell_back[0]) if fell_back else "device loop"))
    if not fell_back0:
        assert not fell_back and s.device is True and s._dev is not None
    chain = s.get_chain()
    assert chain.shape == (steps, nw, 3) and len(np.unique(chain[..., 1])) > nw
    assert_allclose(chain, s0.get_chain(), rtol=1e-8)  # (a blob does not touch the chain)
    blob = np.asarray(s.get_blobs()[1], dtype=float)
    assert blob.shape == (steps, nw, NU_E.size)
    for k in range(steps):
        pars = np.ascontiguousarray(chain[k].T)
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV)
        host = na.SecondaryLeptonsKelner06(pd, nh=10 / u.cm ** 3, product="nu_mu")
        assert not host.on_device
        ref = host.flux(NU_E * u.eV, distance=2 * u.kpc).to("1/(s cm2 eV)").value
        assert_allclose(blob[k], ref, rtol=1e-12)
    assert np.all(blob > 0)
