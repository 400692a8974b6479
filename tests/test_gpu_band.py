"""Band-integrated flux and luminosity per walker on the GPU (naima's idiom
``trapz_loglog(spectrum * E, E)``, utils.py:285-355 of the reference, on a device spectrum):
``nh_trapz_loglog_comps`` against the oracle and against the dense route, the class API on device
parameters, and the integral as a blob and as a prior term of a fit on the device loop."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 63, 64, 65, 100, 1000)
WALKERS = (1, 3, 4, 5, 512)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


# ---------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------
def lazy_rows(ctx, N, n, seed):
    """random positive rows as a lazy matrix: two components (leading dimensions n + 3 and
    n + 1, scales 0.75 and 2.5e3), a per-energy factor and a per-walker row factor
    1.5 * r[w]; with the special rows the shape has room for (the last row is always random):
    one zero node, a sign change, an exact power law of index -1, all NaN"""
    from naima_amd.darray import TF_ID, nh_comp, nh_lazy
    rng = np.random.default_rng(seed)
    x = np.geomspace(0.3, 4e5, n) * (1 + 0.2 * rng.uniform(size=n) / max(n, 1))
    x = np.sort(x)
    lda, ldb = n + 3, n + 1
    A = np.full((N, lda), np.nan)   # (the padding is never read: a NaN there would show)
    B = np.full((N, ldb), np.nan)
    A[:, :n] = 10 ** rng.uniform(-3, 3, (N, n)) * x ** -1.7
    B[:, :n] = 10 ** rng.uniform(-6, -1, (N, n)) * x ** -0.4
    cf = x ** rng.uniform(0.5, 2.0)
    r = rng.uniform(0.5, 2.0, N)
    sa, sb = 0.75, 2.5e3
    kinds = ["zero", "sign", "plaw", "nan"][:max(N - 1, 0)]
    k = n // 2
    for row, kind in enumerate(kinds):
        if kind == "zero":
            A[row, k] = B[row, k] = 0.0
        elif kind == "sign":
            B[row, k:n] *= -1e6
        elif kind == "plaw":
            A[row, :n] = 3.0 / (x * cf)
            B[row, :n] = 1e-4 / (x * cf)
        else:
            A[row, :n] = np.nan
    dA, dB, dr = ctx.array(A), ctx.array(B), ctx.array(r)
    comps = (nh_comp * 2)(nh_comp(dA.ptr, lda, sa), nh_comp(dB.ptr, ldb, sb))
    lz = nh_lazy(dr.ptr, 1, 1.5, 1.0, 0.0, TF_ID, 0)
    return dict(x=x, cf=cf, comps=comps, lz=lz, kinds=kinds, keep=(dA, dB, dr), N=N, n=n,
                xd=ctx.array(x), cfd=ctx.array(cf))


def integrate(ctx, c, ldo=1, intervals=False):
    N, n = c["N"], c["n"]
    width = (n - 1 + 2) if intervals else ldo
    out = ctx.array(np.full((N, width), SENTINEL))
    name = "nh_trapz_loglog_comps_intervals" if intervals else "nh_trapz_loglog_comps"
    ctx.call(name, c["comps"], 2, c["cfd"], C.byref(c["lz"]), c["xd"], N, n, out, width)
    return out.get()


def dense_nodes(ctx, c):
    """the node values as nh_lincomb writes them: (host copy, device buffer)"""
    N, n = c["N"], c["n"]
    Y = ctx.empty((N, n))
    ctx.call("nh_lincomb", c["comps"], 2, c["cfd"], C.byref(c["lz"]), N, n, Y, n)
    return Y.get(), Y


@pytest.mark.parametrize("N", WALKERS)
@pytest.mark.parametrize("n", NS)
def test_entry_point_against_oracle_and_dense_route(na, N, n):
    """rtol 1e-12 against the oracle fed the same node values (what test_abi_trapz_loglog holds
    nh_trapz_loglog to), 1e-13 against nh_trapz_loglog of the dense matrix, the same bits at
    every call; ldo > 1 leaves the other columns alone.

    The sign-change row is compared with an absolute tolerance of 1e-12 times the sum of its
    absolute segment terms: its positive and negative halves cancel in part, so an error of one
    part in 1e12 of a term is more than that of the sum."""
    from naima_amd._lib import get_context
    from oracle import naima_np as O
    ctx = get_context()
    c = lazy_rows(ctx, N, n, seed=1000 * N + n)
    Y, Yd = dense_nodes(ctx, c)
    got3 = integrate(ctx, c, ldo=3)
    assert np.all(got3[:, 1:] == SENTINEL)
    got = got3[:, 0]
    again = integrate(ctx, c, ldo=1)[:, 0]
    assert np.array_equal(got, again, equal_nan=True)
    assert np.array_equal(integrate(ctx, c, ldo=3)[:, 0], got, equal_nan=True)
    ref = O.trapz_loglog(Y, c["x"])
    seg = O.trapz_loglog(Y, c["x"], intervals=True) if n > 1 else np.zeros((N, 0))
    dense = ctx.empty((N,))
    ctx.call("nh_trapz_loglog", Yd, c["xd"], N, n, dense)
    dense = dense.get()
    if n == 1:
        assert np.all(got == 0.0) and np.all(ref == 0.0)
        return
    special = dict(zip(c["kinds"], range(len(c["kinds"]))))
    nan_row = special.get("nan")
    for w in range(N):
        print("N=%d n=%d row %d: %r vs oracle %r, dense %r" % (N, n, w, got[w], ref[w], dense[w])
              ) if w < 6 else None
        if w == nan_row:
            assert np.isnan(got[w]) and np.isnan(ref[w]) and np.isnan(dense[w])
            continue
        assert np.isfinite(got[w])
        atol = 1e-12 * np.abs(seg[w]).sum() if w == special.get("sign") else 0.0
        assert_allclose(got[w], ref[w], rtol=1e-12, atol=atol)
        assert_allclose(got[w], dense[w], rtol=1e-13, atol=atol)
    if "zero" in special and n > 2:
        k = n // 2  # the two segments at the zero node contribute nothing
        assert np.all(seg[special["zero"], max(k - 1, 0):k + 1] == 0.0)
    if "plaw" in special:
        # index -1: the log branch, x1 y1 ln(x2/x1) summed = y0 x0 ln(x_n / x_0)
        w = special["plaw"]
        assert_allclose(got[w], Y[w, 0] * c["x"][0] * np.log(c["x"][-1] / c["x"][0]), rtol=1e-11)


@pytest.mark.parametrize("N,n", [(1, 2), (3, 65), (5, 64), (4, 1000), (512, 100)])
def test_intervals_entry_point(na, N, n):
    from naima_amd._lib import get_context
    from oracle import naima_np as O
    ctx = get_context()
    c = lazy_rows(ctx, N, n, seed=7 * N + n)
    Y, _ = dense_nodes(ctx, c)
    out = integrate(ctx, c, intervals=True)
    assert np.all(out[:, n - 1:] == SENTINEL)
    got = out[:, :n - 1]
    ref = O.trapz_loglog(Y, c["x"], intervals=True)
    total = integrate(ctx, c)[:, 0]
    nan_row = dict(zip(c["kinds"], range(len(c["kinds"])))).get("nan")
    for w in range(N):
        if w == nan_row:
            assert np.all(np.isnan(got[w]))
            continue
        assert_allclose(got[w], ref[w], rtol=1e-12, atol=0)
        assert_allclose(got[w].sum(), total[w], rtol=1e-13, atol=1e-13 * np.abs(got[w]).sum())
    assert np.array_equal(integrate(ctx, c, intervals=True), out, equal_nan=True)


def test_without_factors_and_bad_arguments(na):
    from naima_amd._lib import NaimaHipError, get_context
    from naima_amd.darray import nh_comp
    from oracle import naima_np as O
    ctx = get_context()
    rng = np.random.default_rng(5)
    N, n = 6, 70
    x = np.geomspace(1.0, 1e4, n)
    A = 10 ** rng.uniform(-2, 2, (N, n))
    dA, xd = ctx.array(A), ctx.array(x)
    comps = (nh_comp * 1)(nh_comp(dA.ptr, n, 1.0))
    out = ctx.empty((N,))
    ctx.call("nh_trapz_loglog_comps", comps, 1, None, None, xd, N, n, out, 1)
    assert_allclose(out.get(), O.trapz_loglog(A, x), rtol=1e-12)
    plain = ctx.empty((N,))
    ctx.call("nh_trapz_loglog", dA, xd, N, n, plain)
    assert np.array_equal(out.get(), plain.get())  # (the same nodes, the same order of summation)
    narrow = (nh_comp * 1)(nh_comp(dA.ptr, n - 1, 1.0))
    for args in ((narrow, 1, None, None, xd, N, n, out, 1), (comps, 0, None, None, xd, N, n, out, 1),
                 (comps, 9, None, None, xd, N, n, out, 1), (comps, 1, None, None, xd, N, n, out, 0)):
        with pytest.raises(NaimaHipError):
            ctx.call("nh_trapz_loglog_comps", *args)
    with pytest.raises(NaimaHipError):
        ctx.call("nh_trapz_loglog_comps_intervals", comps, 1, None, None, xd, N, n, out, n - 2)


# ---------------------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------------------
HOST = np.array([[33.0, 33.4, 32.6, 33.1, 32.9],
                 [2.1, 2.5, 2.9, 1.8, 2.3],
                 [1.0, 1.7, 2.3, 1.4, 0.6],
                 [5.0, 12.0, 40.0, 100.0, 3.0]])
GRID = dict(lo_eV=1e9, hi_eV=510e12, per_decade=50)


def _radiative(na, cls, p, lut=True):
    u = na.u
    pd = na.ExponentialCutoffPowerLaw(10 ** p[0] / u.eV, 10 * u.TeV, p[1], 10 ** p[2] * u.TeV)
    ekw = dict(Eemin=1 * u.GeV, Eemax=510 * u.TeV, nEed=50)
    if cls == "Synchrotron":
        return na.Synchrotron(pd, B=p[3] * u.uG, **ekw)
    if cls == "InverseCompton":
        return na.InverseCompton(pd, seed_photon_fields=["CMB", "FIR"], **ekw)
    if cls == "Bremsstrahlung":
        return na.Bremsstrahlung(pd, n0=1 / u.cm ** 3, **ekw)
    return na.PionDecay(pd, nh=1 / u.cm ** 3, Epmin=2 * u.GeV, Epmax=1 * u.PeV, nEpd=40,
                        useLUT=lut)


def _oracle_spectrum(cls, p, E_eV, lut=True):
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    pd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12, alpha=p[1],
                        e_cutoff=10 ** p[2] * 1e12, beta=1.0)
    if cls == "PionDecay":
        Ep = O.proton_grid(2.0, 1e6, 40)
        return O.pion_spectrum(E_eV, Ep, O.J_on(pd, Ep), 1.0,
                               diffsigma=WN.get_lut() if lut else None)
    gam = O.electron_grid(GRID["lo_eV"], GRID["hi_eV"], GRID["per_decade"])
    ne = O.nelec_on(pd, gam)
    if cls == "Synchrotron":
        return O.synchrotron_spectrum(E_eV, gam, ne, p[3] * 1e-6)
    if cls == "InverseCompton":
        return O.ic_spectrum(E_eV, gam, ne, [O.thermal_seed("CMB"), O.thermal_seed("FIR")])[0]
    return O.brems_spectrum(E_eV, gam, ne, n0=1.0)


def _energies(cls):
    return np.geomspace(1e-1, 1e5, 45) if cls == "Synchrotron" else np.geomspace(1e9, 5e13, 45)


CLASSES = [("Synchrotron", True), ("InverseCompton", True), ("Bremsstrahlung", True),
           ("PionDecay", False), ("PionDecay", True)]


@pytest.mark.parametrize("cls,lut", CLASSES, ids=["%s-%s" % (c, "lut" if l else "analytic")
                                                  if c == "PionDecay" else c for c, l in CLASSES])
def test_class_luminosity_on_device_parameters(na, cls, lut):
    """trapz_loglog(rad.flux(E, 0 cm) * E, E).to('erg/s') on a walker batch of device parameters
    against the oracle's spectrum integrated by the oracle's trapz_loglog: rtol 1e-9 (DESIGN 2's
    bar for classes against the oracle), 1e-8 with the look-up table"""
    from naima_amd._lib import get_context
    from naima_amd.darray import DMat, DPars, DVec
    from naima_amd.utils import trapz_loglog
    from oracle import naima_np as O
    u = na.u
    ctx = get_context()
    P = DPars(ctx, ctx.array(HOST), *HOST.shape)
    Ev = _energies(cls)
    E = Ev * u.eV
    rad = _radiative(na, cls, P, lut)
    flux = rad.flux(E, 0 * u.cm)
    assert isinstance(flux.value, DMat)
    lum = trapz_loglog(flux * E, E).to("erg/s")
    assert isinstance(lum, u.Quantity) and isinstance(lum.value, DVec) and lum.value.n == 5
    assert lum.unit == u.erg / u.s
    got = np.asarray(lum.value)
    ref = np.array([O.trapz_loglog(_oracle_spectrum(cls, HOST[:, w], Ev, lut) * Ev, Ev)
                    for w in range(HOST.shape[1])]) * O.ERG_PER_EV
    print(cls, lut, np.abs(got / ref - 1).max())
    assert np.all(ref > 0)
    assert_allclose(got, ref, rtol=1e-8 if (cls == "PionDecay" and lut) else 1e-9)
    # E * flux is the same matrix; intervals=True sums to the integral and stays on the device
    assert np.array_equal(np.asarray(trapz_loglog(E * flux, E).to("erg/s").value), got)
    seg = trapz_loglog(flux * E, E, intervals=True)
    assert isinstance(seg.value, DMat) and seg.value.shape == (5, Ev.size - 1)
    assert_allclose(np.asarray(seg.to("erg/s").value).sum(axis=1), got, rtol=1e-13)
    # axis=1 is the energy axis too; any other axis is refused
    assert np.array_equal(np.asarray(trapz_loglog(flux * E, E, axis=1).to("erg/s").value), got)
    with pytest.raises(ValueError, match="axis"):
        trapz_loglog(flux * E, E, axis=0)


@pytest.mark.parametrize("cls", ["Synchrotron", "InverseCompton", "Bremsstrahlung", "PionDecay"])
def test_host_parameters_are_unchanged(na, cls):
    """on host parameters the call returns a host Quantity, bit-equal to the dense path of
    before (nh_trapz_loglog on an upload of the rows, called directly)"""
    from naima_amd._lib import get_context
    from naima_amd.utils import trapz_loglog
    u = na.u
    ctx = get_context()
    Ev = _energies(cls)
    E = Ev * u.eV
    rad = _radiative(na, cls, HOST)
    y = rad.flux(E, 0 * u.cm) * E
    assert isinstance(y.value, np.ndarray) and y.shape == (5, Ev.size)
    lum = trapz_loglog(y, E)
    assert isinstance(lum, u.Quantity) and isinstance(lum.value, np.ndarray)
    out = ctx.empty((5,))
    ctx.call("nh_trapz_loglog", ctx.array(np.ascontiguousarray(y.value)), ctx.array(Ev), 5,
             Ev.size, out)
    assert np.array_equal(lum.value, out.get())
    assert lum.unit == y.unit * E.unit
    one = trapz_loglog(y[0], E)
    assert np.ndim(one.value) == 0 and one.value == lum.value[0]
    # ... and the device result is the number the download path gave
    from naima_amd.darray import DPars
    P = DPars(ctx, ctx.array(HOST), *HOST.shape)
    dev = trapz_loglog(_radiative(na, cls, P).flux(E, 0 * u.cm) * E, E)
    assert_allclose(np.asarray(dev.value), lum.value, rtol=1e-12)


def test_ratio_and_unit_conversion_stay_on_the_device(na):
    from naima_amd._lib import get_context
    from naima_amd.darray import DPars, DVec
    from naima_amd.utils import trapz_loglog
    u = na.u
    ctx = get_context()
    P = DPars(ctx, ctx.array(HOST), *HOST.shape)
    Ex = np.geomspace(2e3, 1e4, 12) * u.eV
    Eg = np.geomspace(1.0, 100.0, 20) * u.TeV
    syn, ic = _radiative(na, "Synchrotron", P), _radiative(na, "InverseCompton", P)
    calls = []
    real = ctx.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    ctx.call = spy
    try:
        Lx = trapz_loglog(syn.flux(Ex, 0 * u.cm) * Ex, Ex)
        Lg = trapz_loglog(ic.flux(Eg, 0 * u.cm) * Eg, Eg)
        n0 = len(calls)
        Lx_erg, Lg_erg = Lx.to("erg/s"), Lg.to("erg/s")
        assert len(calls) == n0  # .to() is a scale: nothing launched
        ratio = Lx / Lg
        hard = (Lx_erg / Lg_erg)
    finally:
        del ctx.call
    assert calls.count("nh_trapz_loglog_comps") == 2 and calls.count("nh_ew_binary") == 2
    for q in (Lx_erg, Lg_erg, ratio, hard):
        assert isinstance(q, u.Quantity) and isinstance(q.value, DVec)
    assert Lx_erg.value.ptr == Lx.value.ptr and Lx_erg.value.a != Lx.value.a
    sh, ih = _radiative(na, "Synchrotron", HOST), _radiative(na, "InverseCompton", HOST)
    Lxh = trapz_loglog(sh.flux(Ex, 0 * u.cm) * Ex, Ex).to("erg/s").value
    Lgh = trapz_loglog(ih.flux(Eg, 0 * u.cm) * Eg, Eg).to("erg/s").value
    assert_allclose(np.asarray(Lx_erg.value), Lxh, rtol=1e-12)
    assert_allclose(np.asarray(hard.value), Lxh / Lgh, rtol=1e-12)
    assert_allclose(np.asarray(ratio.to(u.dimensionless_unscaled).value), Lxh / Lgh, rtol=1e-12)
    # a bare device vector for a dimensionless product, as the host path returns a bare array
    bare = trapz_loglog(syn.flux(Ex, 0 * u.cm).value, Ex.value)
    assert isinstance(bare, DVec)
    # the EBL factor at a per-walker redshift is applied first
    z = P[2] * 0.1
    ebl = na.EblAbsorptionModel(z)
    absorbed = trapz_loglog(ebl.transmission(Eg) * ic.flux(Eg, 0 * u.cm) * Eg, Eg).to("erg/s")
    assert isinstance(absorbed.value, DVec)
    tr = na.EblAbsorptionModel(HOST[2] * 0.1).transmission(Eg)
    want = trapz_loglog(ih.flux(Eg, 0 * u.cm) * tr * Eg, Eg).to("erg/s").value
    assert_allclose(np.asarray(absorbed.value), want, rtol=1e-12)
    only = trapz_loglog(ebl.transmission(Eg), Eg.value)
    assert isinstance(only, DVec)
    assert_allclose(np.asarray(only), trapz_loglog(tr, Eg.value), rtol=1e-12)


# ---------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------
EB_TEV = np.geomspace(1.0, 100.0, 25)


def cfg3_with_luminosity(na, blob=True):
    """bench.build_problem's cfg3 model (RXJ1713 Syn+IC, blob We) with the 1-100 TeV
    inverse-Compton luminosity as a second blob"""
    from naima_amd.utils import trapz_loglog
    u = na.u
    Eb = EB_TEV * u.TeV

    def model(pars, data):
        ECPL = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10.0 * u.TeV, pars[1],
                                            (10 ** pars[2]) * u.TeV, pars[4])
        IC = na.InverseCompton(ECPL, seed_photon_fields=["CMB", "FIR", "NIR"], Eemin=100 * u.GeV)
        SYN = na.Synchrotron(ECPL, B=pars[3] * u.uG)
        flux = IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)
        We = IC.compute_We(Eemin=1 * u.TeV)
        if not blob:
            return flux, We
        lum = trapz_loglog(IC.flux(Eb, 0 * u.cm) * Eb, Eb).to("erg/s")
        return flux, We, lum

    return model


def oracle_ic_band(p, d_kpc=0.0):
    """the oracle's IC spectrum of cfg3 at walker p, times E, integrated over 1-100 TeV by the
    oracle's trapz_loglog: erg/s, or erg/(cm2 s) at a distance"""
    from oracle import naima_np as O
    pd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12,
                        alpha=p[1], e_cutoff=10 ** p[2] * 1e12, beta=p[4])
    g = O.electron_grid(100e9, 1e9 * O.MEC2_EV, 100)
    E = EB_TEV * 1e12
    ic, _ = O.ic_spectrum(E, g, O.nelec_on(pd, g), [O.thermal_seed(s) for s in ("CMB", "FIR", "NIR")])
    return O.trapz_loglog(O.to_flux(ic, d_kpc * O.KPC_CM) * E, E) * O.ERG_PER_EV


@pytest.fixture(scope="module")
def problem(na):
    from bench import build_problem
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    rng = np.random.default_rng(12)
    pos = p0 * (1 + 0.005 * rng.standard_normal((32, p0.size)))
    return dict(plain=model, p0=p0, raw=raw, data=data, prior=prior, labels=list(labels), pos=pos)


def _sampler(na, pr, model, device, prior=None, seed=23):
    from naima_amd.sampler import EnsembleSampler
    return EnsembleSampler(32, pr["p0"].size, na.lnprob,
                           args=[pr["data"], model, prior or pr["prior"]], seed=seed,
                           naima_style=True, store_blobs=True, device=device)


STEPS = 7


def test_luminosity_blob_keeps_the_device_loop(na, problem):
    """fails on the parent commit: there the sampler warns 'a blob of type ndarray cannot be
    kept in HBM' and falls back to the host-driven loop"""
    pr = problem
    d = _sampler(na, pr, cfg3_with_luminosity(na), True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.run_mcmc(pr["pos"], STEPS)
    assert d.device is True and d._dev is not None and d._dev.fused
    assert "nh_trapz_loglog_comps" in d._dev._plan.calls and not d._dev.mega
    # the blob does not disturb the fit: the model without it (the resident loop), and the
    # host-driven loop of the model with it
    plain = _sampler(na, pr, pr["plain"], True)
    plain.run_mcmc(pr["pos"], STEPS)
    h = _sampler(na, pr, cfg3_with_luminosity(na), False)
    h.run_mcmc(pr["pos"], STEPS)
    assert h.device is False
    for other in (plain, h):
        assert_allclose(d.get_chain()[-1], other.get_chain()[-1], rtol=1e-8)
        assert_allclose(d.get_log_prob()[-1], other.get_log_prob()[-1], rtol=1e-8)
    blobs = d.get_blobs()
    assert len(blobs) == 3
    lum = np.asarray(blobs[2], dtype=float)
    assert lum.shape == (STEPS, 32)
    assert d.blob_units[2] == na.u.erg / na.u.s
    assert_allclose(lum, np.asarray(h.get_blobs()[2], dtype=float), rtol=1e-8)
    assert_allclose(np.asarray(blobs[1], dtype=float), np.asarray(plain.get_blobs()[1], dtype=float),
                    rtol=1e-8)
    final = d.get_chain()[-1]
    ref = np.array([oracle_ic_band(p) for p in final])
    print("blob against the oracle:", np.abs(lum[-1] / ref - 1).max())
    assert_allclose(lum[-1], ref, rtol=1e-9)
    assert len(np.unique(lum)) > 32  # (it moved with the walkers)


def test_luminosity_blob_on_the_sharded_code_path(na, problem, monkeypatch):
    """the blob travels with the log-probabilities through the all-gather of a sharded
    half-step (one rank here): the same chain and the same blob"""
    pr = problem
    d = _sampler(na, pr, cfg3_with_luminosity(na), True)
    d.run_mcmc(d.run_mcmc(pr["pos"], 3), STEPS - 3)
    monkeypatch.setenv("NAIMA_AMD_FORCE_SHARDED", "1")
    s = _sampler(na, pr, cfg3_with_luminosity(na), True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.run_mcmc(s.run_mcmc(pr["pos"], 3), STEPS - 3)
    assert s.device and s._dev.sharded and s._dev.fused
    assert_allclose(s.get_chain(), d.get_chain(), rtol=1e-8)
    assert_allclose(np.asarray(s.get_blobs()[2], dtype=float),
                    np.asarray(d.get_blobs()[2], dtype=float), rtol=1e-8)


def test_same_per_launch_loop_gives_the_same_chain_bit_for_bit(na, problem, monkeypatch):
    """with the one-launch and resident kernels switched off both models run the same per-launch
    loop; the band's spectrum is its own flux(Eb) evaluation, so the launches that make the
    data's spectrum are the same and the chains are equal bit for bit"""
    monkeypatch.setenv("NAIMA_AMD_MEGA", "0")
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    pr = problem
    a = _sampler(na, pr, cfg3_with_luminosity(na), True)
    b = _sampler(na, pr, cfg3_with_luminosity(na, blob=False), True)
    for s in (a, b):
        st = s.run_mcmc(pr["pos"], 3)
        s.run_mcmc(st, STEPS)  # (the second call replays captured step graphs)
        assert s.device and s._dev.fused and not s._dev.mega
    assert np.array_equal(a.get_chain(), b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(np.asarray(a.get_blobs()[1]), np.asarray(b.get_blobs()[1]))
    extra = list(a._dev._plan.calls)
    for name in b._dev._plan.calls:
        extra.remove(name)
    print("launches the blob adds:", extra)
    assert "nh_trapz_loglog_comps" in extra
    lum = np.asarray(a.get_blobs()[2], dtype=float)
    assert lum.shape == (3 + STEPS, 32)
    ref = np.array([oracle_ic_band(p) for p in a.get_chain()[-1][:8]])
    assert_allclose(lum[-1][:8], ref, rtol=1e-9)


@pytest.fixture(scope="module")
def band_prior(na, problem):
    """(prior for the samplers, the oracle's prior): cfg3's prior plus a normal prior on the
    1-100 TeV inverse-Compton energy flux at 1 kpc, from an IC object rebuilt from pars"""
    from naima_amd.utils import trapz_loglog
    from oracle import naima_np as O
    u = na.u
    pr = problem
    Eb = EB_TEV * u.TeV
    f0 = oracle_ic_band(pr["p0"], 1.0)
    mu, sigma = 1.3 * f0, (0.1 * f0) ** 2
    base = pr["prior"]

    def prior(pars):
        ECPL = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10.0 * u.TeV, pars[1],
                                            (10 ** pars[2]) * u.TeV, pars[4])
        IC = na.InverseCompton(ECPL, seed_photon_fields=["CMB", "FIR", "NIR"], Eemin=100 * u.GeV)
        F = trapz_loglog(IC.flux(Eb, 1 * u.kpc) * Eb, Eb).to("erg/(cm2 s)").value
        return base(pars) + na.normal_prior(F, mu, sigma)

    def oprior(p):
        return float(np.asarray(base(p))) + O.normal_prior(oracle_ic_band(p, 1.0), mu, sigma)

    return prior, oprior


@pytest.fixture(scope="module")
def prior_run(na, problem, band_prior):
    pr = problem
    prior, _ = band_prior
    d = _sampler(na, pr, cfg3_with_luminosity(na), True, prior=prior)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st = d.run_mcmc(pr["pos"], 3)
        d.run_mcmc(st, STEPS - 3)  # (the second call replays captured graphs)
    return d


def test_prior_on_the_integral(na, problem, band_prior, prior_run):
    from oracle import workloads_np as WN
    pr, d = problem, prior_run
    prior, oprior = band_prior
    assert d.device is True and d._dev is not None
    print("prior on the integral: fused", d._dev.fused, "one launch", d._dev.mega)
    h = _sampler(na, pr, cfg3_with_luminosity(na), False, prior=prior)
    h.run_mcmc(h.run_mcmc(pr["pos"], 3), STEPS - 3)
    assert d.get_chain().shape == h.get_chain().shape == (STEPS, 32, 5)
    assert_allclose(d.get_chain()[-1], h.get_chain()[-1], rtol=1e-8)
    assert_allclose(d.get_log_prob()[-1], h.get_log_prob()[-1], rtol=1e-8)
    # the prior term matters: without it the ensemble ends elsewhere
    free = _sampler(na, pr, cfg3_with_luminosity(na), True)
    free.run_mcmc(pr["pos"], STEPS)
    assert not np.allclose(free.get_log_prob()[-1], d.get_log_prob()[-1], rtol=1e-3)
    final, lp = d.get_chain()[-1], d.get_log_prob()[-1]
    ref = np.array([WN.lnprob("cfg3", p, pr["raw"], prior=oprior)[0] for p in final])
    print("lnprob against oracle likelihood + oracle prior:", np.abs(lp / ref - 1).max())
    assert_allclose(lp, ref, rtol=1e-7)


def test_plot_table_and_saved_run_show_the_blob(na, problem, prior_run, tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    from naima_amd.analysis import read_run, save_results_table, save_run
    from naima_amd.plot import plot_blob
    d = prior_run
    d.data, d.labels = problem["data"], problem["labels"]
    d.run_info = dict(n_walkers=32, n_run=STEPS)
    lum = np.asarray(d.get_blobs()[2], dtype=float)
    fig = plot_blob(d, blobidx=2, label="L_IC(1-100 TeV)")
    ax = fig.axes[0]
    assert "L_IC(1-100 TeV)" in ax.get_xlabel() and "erg" in ax.get_xlabel()
    t = save_results_table(str(tmp_path / "fit"), d)
    assert "blob2" in t["label"] and "blob1" in t["label"]
    i = t["label"].index("blob2")
    assert_allclose(t["median"][i], np.median(lum), rtol=1e-12)
    assert t["meta"]["blob2_unit"] == d.blob_units[2].name and "erg" in d.blob_units[2].name
    assert "blob2_unit" in open(str(tmp_path / "fit_results.ecsv")).read()
    back = read_run(save_run(str(tmp_path / "run.npz"), d))
    got = np.asarray(back.get_blobs()[2], dtype=float)
    assert np.array_equal(got, lum)
    assert back.blob_units[2] == d.blob_units[2]


def test_run_sampler_keeps_the_blob_units_through_burn_in(na, problem, tmp_path):
    """naima's flow burn-in -> reset -> run (core.py:483-487, 529-530): the run starts from a
    state that has its log-probabilities, so the units found at the first evaluation must
    survive the reset for the table and the saved run to show them"""
    from naima_amd.analysis import save_results_table
    pr = problem
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s, _ = na.run_sampler(data_table=pr["data"], p0=pr["p0"], labels=pr["labels"],
                              model=cfg3_with_luminosity(na), prior=pr["prior"], nwalkers=32,
                              nburn=3, nrun=5, prefit=False, seed=2, verbose=False)
    assert s.device and np.shape(s.get_blobs()[2]) == (5, 32)
    assert s.blob_units is not None and s.blob_units[2] == na.u.erg / na.u.s
    assert s.blob_units[1] == na.u.erg
    t = save_results_table(str(tmp_path / "fit"), s)
    assert t["meta"]["blob2_unit"] == s.blob_units[2].name


def test_integral_of_a_held_back_synchrotron_spectrum(na, problem):
    """the example's model: its 2-10 keV flux integrates a synchrotron spectrum whose launch
    the device loop holds back for the likelihood to ride on; the integral flushes it first.
    Device loop against host-driven loop, both extra blobs"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        from rxj1713_luminosity import ElectronSynICBands
    finally:
        sys.path.pop(0)
    pr = problem
    d = _sampler(na, pr, ElectronSynICBands, True)
    h = _sampler(na, pr, ElectronSynICBands, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.run_mcmc(d.run_mcmc(pr["pos"], 2), 4)
    h.run_mcmc(h.run_mcmc(pr["pos"], 2), 4)
    assert d.device and d._dev.fused and h.device is False
    assert d._dev._plan.calls.count("nh_trapz_loglog_comps") == 2
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-8)
    bd, bh = d.get_blobs(), h.get_blobs()
    assert len(bd) == len(bh) == 4
    for j in (2, 3):
        x, y = np.asarray(bd[j], dtype=float), np.asarray(bh[j], dtype=float)
        assert x.shape == y.shape == (6, 32) and np.all(x > 0)
        assert_allclose(x, y, rtol=1e-8)
    assert d.blob_units[3] == na.u.erg / (na.u.cm ** 2 * na.u.s)


def test_luminosity_example():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "rxj1713_luminosity.py"),
                        "64", "40", "120"], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device loop: True" in r.stdout and "saved and read back" in r.stdout, r.stdout
    for name, unit in (("L_IC(1-100 TeV)", "erg/s"), ("F_syn(2-10 keV)", "erg/(cm2 s)")):
        line = [ln for ln in r.stdout.splitlines() if ln.strip().startswith(name)][0]
        assert unit in line, line
        w = line.split()
        med, lo, hi = float(w[w.index("median") + 1]), float(w[w.index("16%") + 1]), \
            float(w[w.index("84%") + 1])
        true = float(line.split("parameters")[1].strip(" )"))
        assert lo < med < hi and 0.8 * true < med < 1.25 * true, line
