"""GPU tests of nh_pion_kelner06 (naima_amd/csrc/nh_kelner.hip), the one radiative kernel that
does its own quadrature and therefore promises more than parity with the reference: the
CONVERGED integrals.  Held here to a reference that is converged where the integrands have
kinks (oracle.k06_spectrum / k06_Wp with break points; tests/test_oracle.py certifies it to
1e-10 against mpmath) on all five distribution kinds, on both sides of three transition
energies; to properties that need no reference; and at the C entry point."""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kelner_cases as KC
from oracle import naima_np as O

pytestmark = pytest.mark.gpu

RTOL = 1e-8  # the kernel's documented distance from the converged integral
TEV_ERG = 1.602176634


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


def _flux(na, k, E_eV):
    return np.atleast_2d(k.flux(E_eV * na.u.eV, 1 * na.u.kpc).to("1/(s cm2 eV)").value)


# ---------------------------------------------------------------------------------------
# against the converged reference
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Etrans_eV", KC.ETRANS_EV)
@pytest.mark.parametrize("kind", list(KC.SETS))
def test_converged_integrals(na, kind, Etrans_eV):
    """flux, nhat and Wp of every parameter set of one kind (one walker each, one launch)
    within 1e-8 of the converged reference at 1 MeV ... 300 TeV, including m_pi/2 exactly and
    both neighbours of Etrans; and the continuity at Etrans that nhat exists to give"""
    u = na.u
    tags = [t for t, _ in KC.SETS[kind]]
    E = KC.energies(Etrans_eV)
    k = na.PionDecayKelner06(KC.amd_pd(na, kind, [p for _, p in KC.SETS[kind]]),
                             nh=2 / u.cm ** 3, Etrans=Etrans_eV * u.eV)
    f = _flux(na, k, E)
    nhat, Wp = np.atleast_1d(k.nhat), np.atleast_1d(k.Wp.to("erg").value)
    full = E * 1e-12 >= Etrans_eV * 1e-12
    lo, hi = np.flatnonzero(~full)[-1], np.flatnonzero(full)[0]  # the two sides of Etrans
    bad = []
    for j, tag in enumerate(tags):
        spec, ref_nhat = KC.spectrum(tag, E, Etrans_eV)
        err = np.abs(f[j] / O.to_flux(2.0 * spec, O.KPC_CM) - 1)
        errs = {"full": err[full].max(), "delta": err[~full].max(),
                "nhat": abs(nhat[j] / ref_nhat - 1),
                "Wp": abs(Wp[j] / (KC.Wp_TeV(tag) * TEV_ERG) - 1),
                "step at Etrans": abs(f[j, lo] / f[j, hi] - 1)}
        print("K06ERR %-12s Etrans %.0e eV: " % (tag, Etrans_eV)
              + "  ".join("%s %.1e" % kv for kv in errs.items())
              + "  (worst at %.6g eV)" % E[err.argmax()])
        bad += ["%s %s %.1e" % (tag, what, e) for what, e in errs.items() if not e <= RTOL]
    assert not bad, bad


@pytest.mark.parametrize("kind", ["PowerLaw", "BrokenPowerLaw"])
def test_one_sided_energies_need_no_nhat(na, kind):
    """all energies below Etrans, all above: nhat == 1.0 exactly (radiative.py:1743), and the
    spectra are the branches' own integrals"""
    u = na.u
    tags = [t for t, _ in KC.SETS[kind]]
    k = na.PionDecayKelner06(KC.amd_pd(na, kind, [p for _, p in KC.SETS[kind]]),
                             nh=2 / u.cm ** 3)
    E = KC.energies(1e11)
    for side in (E[E < 1e11], E[E >= 1e11]):
        f = _flux(na, k, side)
        assert_array_equal(np.atleast_1d(k.nhat), 1.0)
        for j, tag in enumerate(tags):
            spec, nhat = KC.spectrum(tag, side, 1e11)
            assert nhat == 1.0
            assert_allclose(f[j], O.to_flux(2.0 * spec, O.KPC_CM), rtol=RTOL)


# ---------------------------------------------------------------------------------------
# properties that need no reference
# ---------------------------------------------------------------------------------------
def test_delta_branch_symmetry(na):
    """The delta-functional branch sees E_gamma only through E_gamma + m_pi^2 / (4 E_gamma),
    which E_gamma and m_pi^2 / (4 E_gamma) share up to its rounding: a few 1e-16, which the
    spectrum follows with a logarithmic slope of order alpha, also next to m_pi/2 where
    acosh is steep (its argument is then 1 + O(eps^2)) -- 1e-12 leaves two orders of room"""
    u = na.u
    Eg = np.array([1e6, 1e7, 5e7, 6.5e7, 6.74e7, KC.M_PI_EV / 2 * (1 - 1e-9)])
    mirror = KC.M_PI_EV ** 2 / (4 * Eg)
    assert mirror.max() < 1e10
    for kind in ("PowerLaw", "BrokenPowerLaw", "ExponentialCutoffBrokenPowerLaw"):
        k = na.PionDecayKelner06(KC.amd_pd(na, kind, [p for _, p in KC.SETS[kind]]),
                                 nh=2 / u.cm ** 3, Etrans=1e10 * u.eV)
        f = _flux(na, k, np.concatenate([Eg, mirror, [1e12]]))  # (1 TeV: nhat != 1 too)
        assert np.all(f > 0)
        assert_allclose(f[:, :Eg.size], f[:, Eg.size:2 * Eg.size], rtol=1e-12)


def test_linear_in_amplitude_and_density_batched_as_alone(na):
    """broken power laws: walkers in one launch == one at a time; the spectrum is linear in
    the amplitude and in nh (a product after the quadrature: a rounding or two each)"""
    u = na.u
    E = KC.energies(1e11)
    amp = np.array([4e35, 1e35, 9e35, 12e35])
    nh = np.array([2.0, 1.0, 0.5, 6.0])
    par = dict(e_break=np.array([3.7e12, 2e10, KC.E_EDGE, 3.7e12]) * u.eV,
               alpha_1=np.array([1.8, 2.0, 1.8, 1.8]), alpha_2=np.array([2.9, 2.6, 2.9, 2.9]))
    kb = na.PionDecayKelner06(
        na.BrokenPowerLaw(amp / u.eV, 1 * u.TeV, par["e_break"], par["alpha_1"], par["alpha_2"]),
        nh=nh / u.cm ** 3)
    fb = _flux(na, kb, E)
    nb, wb = kb.nhat, kb.Wp.to("erg").value
    for j in range(4):
        kj = na.PionDecayKelner06(
            na.BrokenPowerLaw(amp[j] / u.eV, 1 * u.TeV, par["e_break"][j], par["alpha_1"][j],
                              par["alpha_2"][j]), nh=nh[j] / u.cm ** 3)
        assert_allclose(fb[j], _flux(na, kj, E)[0], rtol=1e-13)
        assert_allclose(nb[j], kj.nhat, rtol=1e-13)
        assert_allclose(wb[j], kj.Wp.to("erg").value, rtol=1e-13)
    # walker 3 is walker 0 with three times the amplitude and three times the density
    assert_allclose(fb[3], 9 * fb[0], rtol=1e-13)
    assert_allclose(wb[3], 3 * wb[0], rtol=1e-13)
    assert_allclose(nb[3], nb[0], rtol=1e-13)  # (a ratio of two integrals, each linear)


# ---------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------
E9 = np.array([1e6, KC.M_PI_EV / 2, 1e9, np.nextafter(1e11, 0), 1e11, 1e12, 5e10, 3e13, 3e14])
SENTINEL = -7.25


def _rows(na, ctx):
    """three BPL walkers and the kind's enum value"""
    from naima_amd._lib import PD_KIND
    pd = KC.amd_pd(na, "BrokenPowerLaw", [p for _, p in KC.SETS["BrokenPowerLaw"]])
    return pd, pd.device_rows(ctx, 3, amplitude_to=na.u.Unit("1/eV")), PD_KIND[pd.kind]


def _call(ctx, kind, rows, N, E, nE, ldo, Etr=1e11, mixed=1, nhat=True, wp=True, Nbuf=3):
    out = ctx.array(np.full((Nbuf, ldo), SENTINEL))
    nh = ctx.array(np.full(Nbuf, SENTINEL)) if nhat else None
    w = ctx.array(np.full(Nbuf, SENTINEL)) if wp else None
    ctx.call("nh_pion_kelner06", kind, rows, N, ctx.array(E), nE, Etr, mixed, out, ldo, nh, w)
    return out.get(), None if nh is None else nh.get(), None if w is None else w.get()


@pytest.fixture(scope="module")
def nine(na, ctx):
    pd, rows, kind = _rows(na, ctx)
    out, nhat, wp = _call(ctx, kind, rows, 3, E9, 9, 9)
    for j, (tag, _) in enumerate(KC.SETS["BrokenPowerLaw"]):
        spec, ref_nhat = KC.spectrum(tag, E9, 1e11)
        assert_allclose(out[j], spec, rtol=RTOL)
        assert_allclose(nhat[j], ref_nhat, rtol=RTOL)
        assert_allclose(wp[j], KC.Wp_TeV(tag), rtol=RTOL)
    return out, nhat, wp


@pytest.mark.parametrize("nE", [1, 2, 3, 4, 5, 9])
def test_entry_task_loop_and_padding(na, ctx, nine, nE):
    """nE + 3 tasks over four waves, ldo = nE + 3: a task's arithmetic does not depend on
    which wave runs it or on nE (``mixed`` is an argument), so the first nE columns are the
    nine-energy call's to the bit; the padding is not written"""
    pd, rows, kind = _rows(na, ctx)
    out, nhat, wp = _call(ctx, kind, rows, 3, E9[:nE], nE, nE + 3)
    assert_array_equal(out[:, :nE], nine[0][:, :nE])
    assert_array_equal(out[:, nE:], SENTINEL)
    assert_array_equal(nhat, nine[1])
    assert_array_equal(wp, nine[2])


def test_entry_optional_outputs_and_repeat(na, ctx, nine):
    pd, rows, kind = _rows(na, ctx)
    for nhat, wp in ((True, False), (False, True), (False, False), (True, True)):
        out, n, w = _call(ctx, kind, rows, 3, E9, 9, 9, nhat=nhat, wp=wp)
        assert_array_equal(out, nine[0])  # (the last: two identical calls, identical bits)
        if nhat:
            assert_array_equal(n, nine[1])
        if wp:
            assert_array_equal(w, nine[2])
    # mixed = 0: no normalisation, whatever the energies
    out, n, w = _call(ctx, kind, rows, 3, E9, 9, 9, mixed=0)
    assert_array_equal(n, 1.0)
    full = E9 * 1e-12 >= 1e11 * 1e-12  # (in TeV, as the kernel decides it)
    assert_array_equal(out[:, full], nine[0][:, full])
    assert_allclose(out[:, ~full] * nine[1][:, None], nine[0][:, ~full], rtol=1e-15)
    # fewer walkers than the buffers hold: the rows beyond N are not written
    out, n, w = _call(ctx, kind, rows, 2, E9, 9, 9)
    assert_array_equal(out[:2], nine[0][:2])
    assert_array_equal(out[2], SENTINEL)
    assert n[2] == SENTINEL and w[2] == SENTINEL
    # N = 0 is no error and no launch
    out, n, w = _call(ctx, kind, rows, 0, E9, 9, 9)
    assert_array_equal(out, SENTINEL)
    assert_array_equal(n, SENTINEL)
    assert_array_equal(w, SENTINEL)


def test_entry_refusals(na, ctx):
    """every refused call raises NaimaHipError naming the entry point and launches nothing
    (the buffers are large enough for every refused shape all the same)"""
    from naima_amd._lib import NaimaHipError
    pd, rows, kind = _rows(na, ctx)
    cap = 60 * 1024 // 8 - 3  # the largest nE whose nE + 3 results fit the 60 KiB of LDS
    E = np.geomspace(1e8, 1e14, cap + 1)
    for what, kw in (("kind below the enum", dict(kind=-1)), ("kind above the enum", dict(kind=5)),
                     ("nE = 0", dict(nE=0)), ("negative nE", dict(nE=-1)),
                     ("ldo < nE", dict(nE=9, ldo=8)), ("Etrans = 0", dict(Etr=0.0)),
                     ("Etrans < 0", dict(Etr=-1e11)), ("Etrans NaN", dict(Etr=float("nan"))),
                     ("negative N", dict(N=-1)), ("nE above the LDS cap", dict(nE=cap + 1))):
        a = dict(dict(kind=kind, N=3, nE=9, ldo=cap + 1, Etr=1e11), **kw)
        out = ctx.array(np.full((3, cap + 1), SENTINEL))
        side = ctx.array(np.full((2, 3), SENTINEL))
        with pytest.raises(NaimaHipError, match="nh_pion_kelner06"):
            ctx.call("nh_pion_kelner06", a["kind"], rows, a["N"], ctx.array(E), a["nE"], a["Etr"],
                     1, out, a["ldo"], side, C.c_void_p(side.ptr + 24))
            pytest.fail("accepted: " + what)
        assert_array_equal(out.get(), SENTINEL)
        assert_array_equal(side.get(), SENTINEL)
    with pytest.raises(NaimaHipError, match="nh_pion_kelner06"):
        ctx.call("nh_pion_kelner06", kind, None, 3, ctx.array(E), 9, 1e11, 1, out, 9, None, None)
    # the cap itself is accepted
    o, n, w = _call(ctx, kind, rows, 1, E[:cap], cap, cap, Nbuf=1)
    assert np.all(o > 0) and n[0] > 0 and w[0] > 0


# ---------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------
def test_class_device_resident_wp_and_per_walker_density(na, ctx):
    """a model whose amplitude lives in HBM: Wp and the spectrum stay there and equal the
    host model's; nh per walker is a factor per row"""
    from naima_amd.darray import DPars
    u = na.u
    host = np.array([[35.6, 35.0, 35.9], [2.0, 1.0, 0.5]])
    P = DPars(ctx, ctx.array(host), 2, 3)
    E = KC.energies(1e11)

    def model(amp, nh):
        return na.PionDecayKelner06(
            na.BrokenPowerLaw(amp / u.eV, 1 * u.TeV, 3.7 * u.TeV, 1.8, 2.9), nh=nh / u.cm ** 3)
    dev, hst = model(10 ** P[0], P[1]), model(10 ** host[0], host[1])
    assert dev.on_device and not hst.on_device
    wd = dev.Wp
    assert wd.on_device  # (still in HBM)
    assert_allclose(np.asarray(wd.to("erg").value), hst.Wp.to("erg").value, rtol=1e-13)
    fh = hst.flux(E * u.eV, 1 * u.kpc)
    assert_allclose(np.asarray(dev.flux(E * u.eV, 1 * u.kpc).value), fh.value, rtol=1e-13)
    one = model(10 ** host[0], 1.0).flux(E * u.eV, 1 * u.kpc)
    assert_allclose(fh.value, one.value * host[1][:, None], rtol=1e-15)
    spec, _ = KC.spectrum("bpl_above", E, 1e11)
    assert_allclose(fh.to("1/(s cm2 eV)").value[1],
                    O.to_flux(spec * 10 ** host[0, 1] / KC.AMP, O.KPC_CM), rtol=RTOL)


def test_class_refuses_a_table_model(na, golden):
    u = na.u
    z = golden("extra")
    tm = na.TableModel(z["tm_energy_eV"] * u.eV, z["tm_values_per_eV"] / u.eV)
    k = na.PionDecayKelner06(tm)
    with pytest.raises(TypeError, match="analytic naima_amd.models particle distribution"):
        k.flux(np.array([1e10, 1e12]) * u.eV, 1 * u.kpc)
    with pytest.raises(TypeError, match="TableModel"):
        k.Wp
