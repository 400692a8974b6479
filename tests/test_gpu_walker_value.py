"""Every parameter that may be given per walker, given in its three forms: a loop of scalars
(naima's API, one walker at a time), a 1-D host array, and a device value (a ``DVec`` out of a
``DPars``, what a model function on the device loop builds from ``pars[i]``).  The same numbers
have to give the same spectra, or factors, in all three; the result's type and shape follow the
form: an ndarray (n_E,) per scalar, an ndarray (N, n_E) for a host array, a lazy device matrix or
factor of shape (N, n_E) for a device value.

Public API only.  N = 3 walkers and N = 1 (a batch of one), 5 energies (so N != n_E) and 20
nodes per decade on the particle grids.

A bound of ``0`` below asserts the same bits: the forms then reach the kernel as the same
numbers (a host batch of pair absorption or the cooling solve is uploaded as given and converted
as a device value is; a per-walker factor multiplies the same spectrum), or, for ``nh`` of
PionDecay on the device, happen to round alike for these values.  Elsewhere the bound is the one
the suite already holds the same comparison to:
  * a per-walker factor on a shared table (nh, n0, a seed's u), host array vs scalars and device
    vs host: 1e-13 (test_gpu_general.py, per-walker densities);
  * a grid per walker (Eemin, nEed, Epmax), host array -- the general kernel -- vs scalars -- the
    cached table: 1e-10, the protons' spectrum 1e-9; device vs host 1e-13 (test_gpu_general.py,
    general path);
  * EBL redshift, host array vs scalars: 1e-12 (test_gpu_ebl.py).
"""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

NE = 5
E_X = np.geomspace(1e2, 1e5, NE)  # eV: synchrotron
E_G = np.geomspace(1e9, 1e13, NE)  # gamma rays
E_A = np.geomspace(1e12, 1e15, NE)  # where dust and star light absorb


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def _pd(na):
    u = na.u
    return na.ExponentialCutoffPowerLaw(1e33 / u.eV, 10 * u.TeV, 2.4, 50 * u.TeV)


def _inj(na):
    u = na.u
    return na.PowerLaw(1e36 / u.eV / u.s, 1 * u.TeV, 2.2)


# name -> (values of 3 walkers, v -> result, bound host array vs scalars, bound device vs host,
#          the host result of a batch of one has a walker axis, a device value gives a lazy result)
# A device Eemin, nEed or Epmax alone does not make a model "on the device" (its amplitude would,
# in a fit): the general kernel's spectra are then downloaded, an (N, n_E) ndarray.  A host Epmax
# of one walker goes through the walker loop, which stacks: (1, n_E).
CASES = {
    "B": ([10.0, 20.0, 30.0], lambda na, u, v: na.Synchrotron(
        _pd(na), B=v * u.uG, nEed=20).flux(E_X * u.eV, 1 * u.kpc), 0, 1e-13, False, True),
    "n0": ([0.3, 1.0, 4.0], lambda na, u, v: na.Bremsstrahlung(
        _pd(na), n0=v / u.cm ** 3, nEed=20).flux(E_G * u.eV, 1 * u.kpc), 1e-13, 1e-13, False, True),
    "nh-PionDecay": ([0.3, 1.0, 4.0], lambda na, u, v: na.PionDecay(
        _pd(na), nh=v / u.cm ** 3, nEpd=20).flux(E_G * u.eV, 1 * u.kpc), 0, 0, False, True),
    "nh-PionDecayKelner06": ([0.3, 1.0, 4.0], lambda na, u, v: na.PionDecayKelner06(
        _pd(na), nh=v / u.cm ** 3).flux(E_G * u.eV, 1 * u.kpc), 0, 0, False, True),
    "nh-SecondaryLeptonsKelner06": ([0.3, 1.0, 4.0], lambda na, u, v: na.SecondaryLeptonsKelner06(
        _pd(na), nh=v / u.cm ** 3).flux(E_G * u.eV, 1 * u.kpc), 0, 1e-13, False, True),
    "seed-u": ([0.2, 0.5, 1.1], lambda na, u, v: na.InverseCompton(
        _pd(na), seed_photon_fields=[["FIR", 30 * u.K, v * u.eV / u.cm ** 3]],
        nEed=20).flux(E_G * u.eV, 1 * u.kpc), 1e-13, 1e-13, False, True),
    "Eemin": ([1.0, 7.0, 60.0], lambda na, u, v: na.Synchrotron(
        _pd(na), B=20 * u.uG, Eemin=v * u.GeV, nEed=20).flux(E_X * u.eV, 1 * u.kpc),
        1e-10, 1e-13, False, False),
    "nEed": ([20, 25, 30], lambda na, u, v: na.Synchrotron(
        _pd(na), B=20 * u.uG, nEed=v).flux(E_X * u.eV, 1 * u.kpc), 1e-10, 1e-13, False, False),
    "Epmax": ([0.1, 1.0, 10.0], lambda na, u, v: na.PionDecay(
        _pd(na), Epmax=v * u.PeV, nEpd=20).flux(E_G * u.eV, 1 * u.kpc), 1e-9, 1e-13, True, False),
    "redshift": ([0.05, 0.3, 1.2], lambda na, u, v: na.EblAbsorptionModel(v).transmission(
        E_G * u.eV), 1e-12, 0, True, True),
    "path_length": ([5.0, 10.0, 20.0], lambda na, u, v: na.PairAbsorptionModel(
        [["FIR", 30 * u.K, 0.5 * u.eV / u.cm ** 3]], v * u.kpc).transmission(E_A * u.eV),
        0, 0, False, True),
    "pair-T": ([3000.0, 5000.0, 8000.0], lambda na, u, v: na.PairAbsorptionModel(
        [["star", v * u.K, 1 * u.eV / u.cm ** 3]], 1 * u.kpc).transmission(E_A * u.eV),
        0, 0, False, True),
    "cooled-B": ([5.0, 20.0, 80.0], lambda na, u, v: na.CooledElectrons(
        _inj(na), v * u.uG, 3e3 * u.yr, n_per_decade=20)(E_G * 100 * u.eV), 0, 0, True, True),
    "cooled-age": ([3e2, 3e3, 3e4], lambda na, u, v: na.CooledElectrons(
        _inj(na), 20 * u.uG, v * u.yr, n_per_decade=20)(E_G * 100 * u.eV), 0, 0, True, True),
}


def _is_lazy(na, r):
    from naima_amd.darray import DFactor
    return isinstance(r, DFactor) or (isinstance(r, na.u.Quantity) and r.on_device)


def _host(na, r):
    return np.asarray(r.value if isinstance(r, na.u.Quantity) else r)


def _same(got, ref, bound, what):
    diff = np.abs(got - ref) / np.where(ref != 0, np.abs(ref), 1.0)
    print("%-40s max relative difference %.3e (bound %g)" % (what, np.nanmax(diff), bound))
    assert np.all(np.isfinite(ref)) and np.any(ref != 0), what
    if bound == 0:
        assert_array_equal(got, ref, err_msg=what)
    else:
        assert_allclose(got, ref, rtol=bound, atol=1e-300, err_msg=what)


@pytest.mark.parametrize("N", [3, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_three_forms_agree(na, name, N):
    from naima_amd._lib import get_context
    from naima_amd.darray import DPars
    u = na.u
    values, build, loop_bound, dev_bound, one_has_axis, dev_lazy = CASES[name]
    vals = np.array(values[:N], dtype=float)
    scalar = int if name == "nEed" else float

    loop = [build(na, u, scalar(v)) for v in vals]
    for r in loop:
        assert not _is_lazy(na, r) and _host(na, r).shape == (NE,)
    loop = np.stack([_host(na, r) for r in loop])

    host = build(na, u, vals.astype(int) if name == "nEed" else vals)
    assert not _is_lazy(na, host)
    host = _host(na, host)
    assert isinstance(host, np.ndarray)
    assert host.shape == ((N, NE) if N > 1 or one_has_axis else (NE,)), host.shape
    host = host.reshape(N, NE)
    _same(host, loop, loop_bound, "%s N=%d: host array vs scalars" % (name, N))

    ctx = get_context()
    pars = DPars(ctx, ctx.array(np.stack([vals, vals + 1.0])), 2, N)
    dev = build(na, u, pars[0])
    assert _is_lazy(na, dev) is dev_lazy
    if dev_lazy:
        assert tuple(dev.shape) == (N, NE)
    else:  # (downloaded: the shape of a host result, a batch of one without its walker axis)
        assert isinstance(dev.value, np.ndarray) and dev.shape == ((N, NE) if N > 1 else (NE,))
    _same(_host(na, dev).reshape(N, NE), host, dev_bound, "%s N=%d: device value vs host array" % (name, N))
