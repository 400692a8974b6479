"""EBL absorption with the redshift a free parameter (models.py:470-552 of the reference,
examples/absorbed_SynIC.py): nh_ebl_table / nh_ebl_apply against the scalar path, the device
factor in a model on the device loop against the host-driven loop and the oracle, the bands,
and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

from test_ebl_host import ebl_restated
from test_gpu_shapes import KPC, _repr, check_oracle, make_raw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SGRID, IGRID = (1e9, 1e15, 60), (1e11, 1e15, 80)
P0 = np.array([33.0, 2.4, 1.5, 1.0, 0.3])


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def redshift_batch():
    """every tie point 0.015 + 0.01 k with its two neighbours, every tabulated z, the edges,
    and random values up to beyond the table: >= 2000 redshifts"""
    ties = 0.015 + 0.01 * np.arange(398)
    z = [ties, np.nextafter(ties, -np.inf), np.nextafter(ties, np.inf), np.arange(0.01, 4, 0.01),
         np.array([0.0, -0.0, np.nextafter(0.01, 0.0), 0.01, 3.99, 3.995, 4.0, 50.0])]
    z.append(np.random.default_rng(3).uniform(0.0, 4.2, 2000 - sum(len(a) for a in z)))
    return np.concatenate(z)


def energies(na):
    from naima_amd import units as u
    g = np.load(os.path.join(HERE, "golden", "extra.npz"))
    return np.concatenate([g["ebl_e_eV"], np.geomspace(0.5e9, 2e14, 200)]) * u.eV


@pytest.fixture(scope="module")
def host_batch(na):
    """(z, e, transmission rows, __call__ rows) of the host batch"""
    z, e = redshift_batch(), energies(na)
    m = na.EblAbsorptionModel(z)
    tr = m.transmission(e)
    call = m(e)
    return z, e, tr, call


def test_host_batch_is_the_scalar_path_at_every_redshift(na, host_batch):
    z, e, tr, call = host_batch
    assert z.size >= 2000 and tr.shape == (z.size, e.size) and call.shape == (z.size, e.size)
    assert isinstance(tr, np.ndarray) and isinstance(call, na.u.Quantity)
    memo = {}
    for w, zw in enumerate(z):
        m = na.EblAbsorptionModel(float(zw))
        key = m._values.value.tobytes()  # (the scalar result depends on its column alone)
        if key not in memo:
            memo[key] = (m.transmission(e), np.asarray(m(e).value, dtype=float))
        st, sc = memo[key]
        assert_allclose(tr[w], st, rtol=1e-12, err_msg="z=%r" % zw)
        assert_allclose(call.value[w], sc, rtol=1e-12, atol=0, err_msg="z=%r" % zw)
    assert len(memo) == 400  # (every column and the z < 0.01 row)


def test_device_batch_is_bit_identical_to_the_host_batch(na, host_batch):
    from naima_amd import _lib
    from naima_amd.darray import DEbl, DPars
    z, e, tr, call = host_batch
    ctx = _lib.get_context()
    pars = DPars(ctx, ctx.array(np.stack([np.zeros_like(z), z])), 2, z.size)
    for zz in (pars[1], pars[1] * na.u.dimensionless_unscaled):
        m = na.EblAbsorptionModel(zz)
        t = m.transmission(e)
        assert isinstance(t, DEbl) and t.shape == (z.size, e.size)
        np.testing.assert_array_equal(t.get(), tr)
        np.testing.assert_array_equal(np.asarray(t), tr)
        c = m(e)
        np.testing.assert_array_equal(np.asarray(c.value), call.value)


def test_invalid_redshifts_give_nan_rows(na):
    from naima_amd import _lib
    from naima_amd.darray import DPars
    e = energies(na)
    z = np.array([0.5, -0.1, np.nan, np.inf, 1.0, -0.0, -np.inf])
    bad = np.array([False, True, True, True, False, False, True])
    tr = na.EblAbsorptionModel(z).transmission(e)
    assert np.all(np.isnan(tr[bad])) and not np.any(np.isnan(tr[~bad]))
    for w in np.nonzero(~bad)[0]:
        assert_allclose(tr[w], na.EblAbsorptionModel(float(z[w])).transmission(e), rtol=1e-12)
    ctx = _lib.get_context()
    dev = na.EblAbsorptionModel(DPars(ctx, ctx.array(z[None, :]), 1, z.size)[0]).transmission(e)
    np.testing.assert_array_equal(dev.get(), tr)
    with pytest.raises(ValueError):
        na.EblAbsorptionModel(-0.1)


def absorbed(na, blobs=True):
    """Synchrotron + EBL-absorbed IC on the CMB (examples/absorbed_SynIC.py of the reference);
    pars: log10 amplitude, alpha, log10(cutoff / TeV), log10(B / uG), z.  Blobs: the model, We
    above 1 TeV, the transmission."""
    from oracle import naima_np as O
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV)
        SYN = na.Synchrotron(pd, B=10 ** pars[3] * u.uG, Eemin=SGRID[0] * u.eV,
                             Eemax=SGRID[1] * u.eV, nEed=SGRID[2])
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=IGRID[0] * u.eV,
                               Eemax=IGRID[1] * u.eV, nEed=IGRID[2])
        T = na.EblAbsorptionModel(pars[4] * u.dimensionless_unscaled).transmission(data)
        flux = T * IC.flux(data, distance=1 * u.kpc) + SYN.flux(data, distance=1 * u.kpc)
        if not blobs:
            return flux
        return flux, IC.compute_We(Eemin=1 * u.TeV), T

    def omodel(p, E):
        pd = O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12,
                            alpha=p[1], e_cutoff=10 ** p[2] * 1e12, beta=1.0)
        gs, gi = O.electron_grid(*SGRID), O.electron_grid(*IGRID)
        sy = O.synchrotron_spectrum(E, gs, O.nelec_on(pd, gs), 10 ** p[3] * 1e-6)
        ic, _ = O.ic_spectrum(E, gi, O.nelec_on(pd, gi), [O.thermal_seed("CMB")])
        We = O.electron_energy_content(pd, O.electron_grid(1e12, IGRID[1], IGRID[2]))
        return O.to_flux(sy + ic * ebl_restated(p[4], E)[0], KPC), We

    return model, omodel


def unabsorbed(na):
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV)
        SYN = na.Synchrotron(pd, B=10 ** pars[3] * u.uG, Eemin=SGRID[0] * u.eV,
                             Eemax=SGRID[1] * u.eV, nEed=SGRID[2])
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=IGRID[0] * u.eV,
                               Eemax=IGRID[1] * u.eV, nEed=IGRID[2])
        return (IC.flux(data, distance=1 * u.kpc) + SYN.flux(data, distance=1 * u.kpc),
                IC.compute_We(Eemin=1 * u.TeV))

    return model


def _prior(na, z_lo=0.0):
    def prior(pars):
        return (na.uniform_prior(pars[0], 20, 45) + na.uniform_prior(pars[1], 1, 4)
                + na.uniform_prior(pars[2], -1, 3) + na.uniform_prior(pars[3], -1, 4)
                + (na.uniform_prior(pars[4], z_lo, 5) if z_lo is not None else 0.0))

    def oprior(p):
        from oracle import naima_np as O
        b = [(20, 45), (1, 4), (-1, 3), (-1, 4)] + ([(z_lo, 5)] if z_lo is not None else [])
        return float(sum(O.uniform_prior(p[i], lo, hi) for i, (lo, hi) in enumerate(b)))

    return prior, oprior


def _raw(omodel):
    E = np.concatenate([np.geomspace(1e3, 1e4, 6), np.geomspace(1e10, 2e13, 12)])
    true = _repr(omodel(P0, E)[0], E, "erg/(cm2 s)")
    return make_raw(E, true, "erg/(cm2 s)", np.random.default_rng(41), uls=(3, 15),
                    ul_factor=(1.6, 2.5))


def _pos(nw, z_width=0.05, seed=5):
    pos = P0 + np.array([0.05, 0.01, 0.02, 0.01, z_width]) * \
        np.random.default_rng(seed).standard_normal((nw, P0.size))
    return pos


def test_device_factor_times_a_device_flux(na):
    from naima_amd import _lib
    from naima_amd.darray import DEbl, DMat, DPars
    from naima_amd.datatable import make_data
    model, omodel = absorbed(na)
    data = make_data(_raw(omodel))
    pos = _pos(32)
    pos[:4, 4] = [0.0, 0.012, 0.025, 3.0]
    ctx = _lib.get_context()
    out = model(DPars(ctx, ctx.array(np.ascontiguousarray(pos.T)), 5, 32), data)
    host = model(np.ascontiguousarray(pos.T), data)
    assert isinstance(out[0].value, DMat) and isinstance(out[2], DEbl)
    assert_allclose(np.asarray(out[0].value), host[0].to(out[0].unit).value, rtol=1e-13,
                    atol=0)
    np.testing.assert_array_equal(out[2].get(), host[2])
    # either side, bare or as a Quantity
    u = na.u
    IC = na.InverseCompton(na.ExponentialCutoffPowerLaw(
        10 ** DPars(ctx, ctx.array(np.ascontiguousarray(pos.T)), 5, 32)[0] / u.eV, 10 * u.TeV,
        2.4, 30 * u.TeV), seed_photon_fields=["CMB"])
    f = IC.flux(data, distance=1 * u.kpc)
    a = np.asarray((f * out[2]).value)
    np.testing.assert_array_equal(a, np.asarray((out[2] * f).value))
    np.testing.assert_array_equal(np.asarray(f.value.__mul__(out[2])), a)
    assert_allclose(a, np.asarray(f.value) * host[2], rtol=1e-15)


def _loops(na, nw, steps, prior, model, env=(), **kw):
    from naima_amd.sampler import EnsembleSampler
    _, omodel = absorbed(na)
    from naima_amd.datatable import make_data
    data = make_data(_raw(omodel))
    k = dict(args=[data, model, prior], seed=31, naima_style=True, store_blobs=True, **kw)
    return EnsembleSampler(nw, P0.size, na.lnprob, **k), \
        EnsembleSampler(nw, P0.size, na.lnprob, device=True, **k)


def test_device_loop_equals_host_loop_and_oracle(na, monkeypatch):
    import warnings
    model, omodel = absorbed(na)
    prior, oprior = _prior(na)
    nw, steps = 64, (3, 17)
    pos = _pos(nw)
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    h, d = _loops(na, nw, steps, prior, model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no fallback warning)
        sh, sd = h.run_mcmc(pos, steps[0]), d.run_mcmc(pos, steps[0])
        sh, sd = h.run_mcmc(sh, steps[1]), d.run_mcmc(sd, steps[1])
    assert d.device and d._dev is not None and d._dev.fused and not d._dev.mega
    assert d._dev.graph is not None or d._dev.step_graph is not None
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-8)
    assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-6)
    assert_allclose(d.acceptance_fraction, h.acceptance_fraction)
    assert 0.05 < np.mean(d.acceptance_fraction) < 0.95
    bh, bd = h.get_blobs(), d.get_blobs()
    assert len(bd) == len(bh) == 3
    for x, y in zip(bd, bh):
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        assert x.shape == y.shape and x.shape[:2] == (sum(steps), nw)
        assert_allclose(x, y, rtol=1e-8, atol=1e-300)
    # the z column actually moved and reached several tabulated redshifts
    assert len(np.unique(np.round(d.get_chain()[..., 4], 2))) > 5
    run = dict(chain=d.get_chain(), lp=d.get_log_prob(),
               blobs=[np.asarray(b, dtype=float) for b in bd], units=list(d.blob_units))
    raw = _raw(omodel)
    check_oracle(na, {"per-launch": run}, raw, lambda p: omodel(p, raw["energy"]), oprior,
                 tag="absorbed")
    # the sharded code path makes the same chain
    monkeypatch.setenv("NAIMA_AMD_FORCE_SHARDED", "1")
    _, s = _loops(na, nw, steps, prior, model)
    st = s.run_mcmc(pos, steps[0])
    s.run_mcmc(st, steps[1])
    assert s._dev.sharded and s._dev.fused
    assert_allclose(s.get_chain(), d.get_chain(), rtol=1e-8)


def test_negative_redshifts_without_a_prior_follow_nan_policy(na, monkeypatch):
    model, _ = absorbed(na)
    prior, _ = _prior(na, z_lo=None)
    nw = 64
    pos = _pos(nw, z_width=0.004, seed=9)
    pos[:, 4] = np.abs(pos[:, 4] - P0[4]) + 0.001  # (close to 0: proposals below it occur)
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    for device in (False, True):
        h, d = _loops(na, nw, (0, 0), prior, model)
        s = d if device else h
        with pytest.raises(ValueError, match="Probability function returned NaN"):
            with np.errstate(all="ignore"):
                s.run_mcmc(pos, 40)
                s.get_chain()  # (the device loop raises when its results reach the host)
    h, d = _loops(na, nw, (0, 0), prior, model, nan_policy="reject")
    with np.errstate(all="ignore"):
        h.run_mcmc(pos, 20)
        d.run_mcmc(pos, 20)
        cd = d.get_chain()  # (the device loop's counts reach the host with its results)
    assert h.nan_proposals > 0 and d.nan_proposals == h.nan_proposals
    assert_allclose(cd, h.get_chain(), rtol=1e-8)


def test_one_launch_more_than_without_absorption(na, monkeypatch):
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    monkeypatch.setenv("NAIMA_AMD_MEGA", "0")
    prior, _ = _prior(na)
    calls = []
    full = absorbed(na)[0]

    def absorbed_we(pars, data):  # (the same blobs as the model without absorption)
        return full(pars, data)[:2]

    for model in (unabsorbed(na), absorbed_we):
        _, d = _loops(na, 64, (0, 0), prior, model)
        d.run_mcmc(_pos(64), 4)
        assert d._dev.fused and not d._dev.mega
        calls.append(list(d._dev._plan.calls))
    plain, ebl = calls
    print("\nlaunches: without absorption %s, with %s" % (plain, ebl))
    assert "nh_ebl_apply" in ebl and len(ebl) <= len(plain) + 1
    rest = list(ebl)
    rest.remove("nh_ebl_apply")
    assert sorted(set(rest)) == sorted(set(plain))


def test_bands_on_device_parameters(na, monkeypatch):
    from naima_amd import plot
    model, _ = absorbed(na)
    prior, _ = _prior(na)
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    _, d = _loops(na, 64, (0, 0), prior, model)
    d.run_mcmc(_pos(64), 6)
    d.data, d.labels, d.modelfn = d.args[0], ["a", "b", "c", "d", "z"], model
    seen = []
    real = plot._evaluate_device

    def spy(*a):
        r = real(*a)
        seen.append(r is not None)
        return r

    monkeypatch.setattr(plot, "_evaluate_device", spy)
    er = [1e9, 5e13] * na.u.eV
    x1, ci1 = plot._calc_CI(d, e_range=er, e_npoints=40, n_samples=60, seed=4)
    assert seen and all(seen)
    monkeypatch.setattr(plot, "_evaluate_device", lambda *a: None)
    x2, ci2 = plot._calc_CI(d, e_range=er, e_npoints=40, n_samples=60, seed=4)
    assert_allclose(x1.value, x2.value)
    for (a1, b1), (a2, b2) in zip(ci1, ci2):
        assert_allclose(a1.value, a2.to(a1.unit).value, rtol=1e-12)
        assert_allclose(b1.value, b2.to(b1.unit).value, rtol=1e-12)


def test_absorbed_synic_example():
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "absorbed_synic.py"),
                        "64", "60", "140"], capture_output=True, text=True, timeout=900,
                       cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "saved and read back" in r.stdout, r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("z percentiles")][0]
    lo, hi, true = (float(v) for v in line.split(":")[1].split())
    assert lo <= true <= hi, line
