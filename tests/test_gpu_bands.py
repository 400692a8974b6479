"""Posterior bands on the GPU: nh_column_select against np.sort, naima's _calc_CI / find_ML on
stored blobs against the reference (tests/golden/bands.npz), e_range bands of a device run
against the oracle's spectra at the same draws, the host-parameter fallback, read_run(modelfn=)
and the figures of save_diagnostic_plots / plot_fit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_bands_host import FU, Stub, bands  # noqa: E402

pytestmark = pytest.mark.gpu

RT_MODEL = 1e-9  # the spectrum tolerance of the loop tests (test_gpu_shapes.py)


def select(x, ncol, ranks):
    """nh_column_select of the first ncol columns of host x [M][ld] at ``ranks``"""
    import ctypes as C

    from naima_amd import _lib
    ctx = _lib.get_context()
    M, ld = x.shape
    dx = ctx.array(x)
    out = ctx.empty((len(ranks), ncol))
    ctx.call("nh_column_select", dx, M, ncol, ld, (C.c_int * len(ranks))(*ranks), len(ranks), out)
    return out.get()


def nasty(rng, M, ld):
    """lognormal columns with ties, +-inf, +-0, subnormals and NaNs scattered through"""
    x = np.exp(rng.normal(-20, 4, size=(M, ld))) * np.where(rng.random((M, ld)) < 0.3, -1, 1)
    k = max(1, M // 50)
    for v in (np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-310, np.nan):
        idx = rng.integers(0, M, size=(k, ld))
        np.put_along_axis(x, idx, v, axis=0)
    x[:, 0] = np.round(x[:, 0] * 1e9) / 1e9  # heavy ties
    if ld > 2:
        x[:, 2] = 1.25  # all equal
    return x


@pytest.mark.parametrize("M,ncol", [(1, 1), (2, 5), (63, 64), (64, 261), (65, 5), (1000, 64),
                                    (1000, 261), (2 ** 17 + 3, 64), (2 ** 17 + 3, 1),
                                    (2097152, 5)])
def test_column_select_is_np_sort(M, ncol):
    rng = np.random.default_rng(M * 7 + ncol)
    ld = ncol + 3
    x = nasty(rng, M, ld)
    want_all = np.sort(x[:, :ncol], axis=0)
    # ranks: both ends, R = 16 (duplicates allowed), and in the middle of the NaN block
    ranks = sorted(set([0, M - 1, M // 2, M // 3]))
    ranks += list(rng.integers(0, M, size=16 - len(ranks)))
    for rk in (ranks, [M - 1], [0]):
        got = select(x, ncol, [int(r) for r in rk])
        want = want_all[rk]
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)  # (NaN where NaN, -0.0 == +0.0)


def test_column_select_nan_below_and_above_a_rank():
    """a column with NaNs: ranks below the NaN block get numbers, ranks inside it get NaN"""
    x = np.array([[3.0], [np.nan], [-1.0], [np.inf], [np.nan], [0.0], [-0.0], [-np.inf]])
    x = np.repeat(x, 3, axis=1)
    x[:, 1] = [np.nan] * 8
    got = select(x, 3, list(range(8)))
    np.testing.assert_array_equal(got, np.sort(x, axis=0))


def test_column_select_rejects_bad_arguments():
    import ctypes as C

    from naima_amd import _lib
    ctx = _lib.get_context()
    dx = ctx.array(np.zeros((4, 3)))
    out = ctx.empty((2, 3))
    for M, ncol, ld, ranks, msg in ((4, 3, 3, [0, 4], "rank"), (4, 3, 3, [-1], "rank"),
                                    (0, 3, 3, [0], "M == 0"), (4, 4, 3, [0], "ncol > ld"),
                                    (2 ** 31, 3, 3, [0], "2\\^31"),
                                    (4, 3, 3, list(range(4)) * 5, "R must")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            ctx.call("nh_column_select", dx, M, ncol, ld, (C.c_int * len(ranks))(*ranks),
                     len(ranks), out)


@pytest.mark.parametrize("name", ["logn", "edge"])
def test_calc_CI_on_stored_blobs_equals_the_reference(name):
    from naima_amd import plot as P
    z = bands()
    s = Stub(z, name)
    for last in (0, 1):
        for ci, confs in enumerate(([3, 1], [3, 1, 0.5], [2])):
            mx, CI = P._calc_CI(s, 0, confs=list(confs), last_step=bool(last))
            got = np.array([[lo.to(FU).value, hi.to(FU).value] for lo, hi in CI])
            np.testing.assert_array_equal(got, z["%s__last%d__ci%d" % (name, last, ci)])
            assert np.array_equal(mx.to("TeV").value, z[name + "__energy_TeV"])
    ML, MLp, MLerr, (mx, my) = P.find_ML(s, 0)
    assert ML == z[name + "__ML"] and np.array_equal(MLp, z[name + "__MLp"])


@pytest.fixture(scope="module")
def cfg3_run():
    import naima_amd as na
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    nw = 64
    s = EnsembleSampler(nw, p0.size, na.lnprob, args=[data, model, prior], seed=5,
                        naima_style=True, device=True)
    start = p0 * (1 + 0.01 * np.random.default_rng(1).standard_normal((nw, p0.size)))
    s.run_mcmc(start, 10)
    s.data, s.labels, s.modelfn = data, list(labels), model
    return s, raw


E_RANGE_EV = (1e-2, 1e14)


def test_e_range_band_of_a_device_run_matches_the_oracle(cfg3_run):
    from naima_amd import plot as P
    from naima_amd import units as u
    from oracle import workloads_np as WN
    s, raw = cfg3_run
    e_range = [E_RANGE_EV[0] * u.eV, E_RANGE_EV[1] * u.eV]
    confs = [3, 1, 0.5]
    n = 300
    mx, CI = P._calc_CI(s, 0, confs=confs, e_range=e_range, e_npoints=48, n_samples=n, seed=9)
    E = np.logspace(np.log10(E_RANGE_EV[0]), np.log10(E_RANGE_EV[1]), 48)
    np.testing.assert_allclose(mx.to("eV").value, E, rtol=1e-15)
    pars = s.get_chain(flat=True)[np.random.RandomState(9).randint(len(s.get_chain(flat=True)),
                                                                   size=n)]
    spec = np.array([WN.model_cfg3(p, E)[0] for p in pars])  # 1/(s cm2 eV)
    ranks = P._band_ranks(n, confs)
    want = np.sort(spec, axis=0)[ranks]
    # an order statistic moves by no more than the largest change of its column's inputs
    bound = np.max(RT_MODEL * np.abs(spec), axis=0) + 1e-200
    for j, (lo, hi) in enumerate(CI):
        for k, band in enumerate((lo, hi)):
            got = band.to("1/(s cm2 eV)").value
            assert np.all(np.abs(got - want[2 * j + k]) <= bound), (j, k)
    # the ML model on the same grid
    _, MLp, _, (mx2, my2) = P._calc_ML(s, 0, e_range=e_range, e_npoints=48)
    np.testing.assert_allclose(my2.to("1/(s cm2 eV)").value, WN.model_cfg3(MLp, E)[0],
                               rtol=RT_MODEL, atol=1e-200)


def test_4096_draws_run_on_the_device(cfg3_run, monkeypatch):
    from naima_amd import plot as P
    from naima_amd import units as u
    s, _ = cfg3_run

    def no_host(*a, **k):
        raise AssertionError("the host-parameter path was taken")

    monkeypatch.setattr(P, "_evaluate_host", no_host)
    e_range = [1 * u.keV, 10 * u.TeV]
    mx, CI = P._calc_CI(s, 0, confs=[3, 1], e_range=e_range, e_npoints=64, n_samples=4096,
                        seed=4)
    _, model = P._read_or_calc_samples(s, 0, n_samples=4096, e_range=e_range, e_npoints=64,
                                       seed=4)
    v = np.asarray(model.value)
    assert v.shape == (4096, 64)
    want = np.sort(v, axis=0)[P._band_ranks(4096, [3, 1])]
    got = np.array([b.to(model.unit).value for pair in CI for b in pair])
    np.testing.assert_array_equal(got, want)
    # chunked evaluation fills one buffer with the same rows
    monkeypatch.setattr(P, "_EVAL_BATCH", 1000)
    _, model2 = P._read_or_calc_samples(s, 0, n_samples=4096, e_range=e_range, e_npoints=64,
                                        seed=4)
    np.testing.assert_allclose(np.asarray(model2.value), v, rtol=1e-13, atol=0)


def test_tuple_blob_band_is_over_its_own_energies(cfg3_run):
    from naima_amd import plot as P
    from naima_amd import units as u
    s, _ = cfg3_run
    model = s.modelfn
    Eown = np.logspace(2, 12, 30) * u.eV

    def with_pair(pars, data):
        flux, We = model(pars, data)
        return flux, (Eown, model(pars, {"energy": Eown, "flux": data["flux"]})[0])

    class S2:
        pass

    s2 = S2()
    s2.__dict__.update(get_chain=s.get_chain, data=s.data, modelfn=with_pair)
    mx, CI = P._calc_CI(s2, 1, confs=[1], e_range=[1 * u.keV, 1 * u.TeV], e_npoints=20,
                        n_samples=200, seed=2)
    assert np.array_equal(mx.value, Eown.value)
    s2.modelfn = model
    _, CI0 = P._calc_CI(s2, 0, confs=[1], e_range=[1e2 * u.eV, 1e12 * u.eV], e_npoints=30,
                        n_samples=200, seed=2)
    for a, b in zip(CI[0], CI0[0]):
        np.testing.assert_allclose(a.value, b.to(a.unit).value, rtol=1e-12, atol=0)


def test_numpy_model_takes_the_host_parameter_path():
    """a functional model written in numpy (a power law with a per-walker low-energy cutoff) gives
    a host array for device parameters, not a device matrix: the draws are evaluated as one
    host-parameter batch, uploaded and selected"""
    import naima_amd as na
    from naima_amd import plot as P
    u = na.u

    def model(pars, data):
        E = data["energy"].to("TeV").value
        amp, alpha, emin = (np.asarray(pars[i], dtype=float)[..., None] for i in range(3))
        return u.Quantity(amp * E ** -alpha * np.exp(-emin / E), "1/(cm2 s TeV)")

    class S:
        pass

    rng = np.random.default_rng(3)
    chain = np.stack([rng.lognormal(-25, 0.2, (6, 8)), rng.normal(2.3, 0.1, (6, 8)),
                      rng.uniform(0.1, 2.0, (6, 8))], -1)
    s = S()
    s.get_chain = lambda flat=False: chain.reshape(-1, 3) if flat else chain
    s.data = {"energy": np.ones(3) * u.TeV, "flux": np.ones(3) * u.Unit("1/(cm2 s TeV)")}
    s.modelfn = model
    calls = []
    real = P._evaluate_host
    P._evaluate_host = lambda *a: calls.append(1) or real(*a)
    try:
        e_range = [100 * u.GeV, 50 * u.TeV]
        mx, CI = P._calc_CI(s, 0, confs=[1, 2], e_range=e_range, e_npoints=16, n_samples=40,
                            seed=1)
    finally:
        P._evaluate_host = real
    assert calls
    pars = P._draw(s, 40, False, 1)
    host = model(np.ascontiguousarray(pars.T), {"energy": mx})
    want = np.sort(np.asarray(host.value), axis=0)[P._band_ranks(40, [1, 2])]
    got = np.array([b.to(host.unit).value for pair in CI for b in pair])
    np.testing.assert_array_equal(got, want)


def test_radiative_model_with_eemin_per_walker_takes_the_host_parameter_path():
    """Bremsstrahlung with Eemin (and the electron-electron weight) as fit parameters shapes the
    particle grid per walker: on device parameters the radiative class raises
    NotImplementedError, so the draws go through the model as one [ndim][n] host batch, and the
    band is the order statistics of the same model evaluated draw by draw"""
    import naima_amd as na
    from naima_amd import _lib
    from naima_amd import plot as P
    from naima_amd.darray import DPars
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 1 * u.TeV, pars[1], 10 * u.TeV)
        br = na.Bremsstrahlung(pd, n0=1 / u.cm ** 3, Eemin=pars[2] * u.GeV, weight_ee=pars[3])
        return br.flux(data, distance=1 * u.kpc)

    class S:
        pass

    rng = np.random.default_rng(8)
    chain = np.stack([rng.normal(33.0, 0.1, (5, 8)), rng.normal(2.2, 0.1, (5, 8)),
                      rng.uniform(0.1, 10.0, (5, 8)), rng.uniform(1.0, 1.2, (5, 8))], -1)
    s = S()
    s.get_chain = lambda flat=False: chain.reshape(-1, 4) if flat else chain
    s.data = {"energy": np.ones(3) * u.TeV, "flux": np.ones(3) * u.Unit("1/(cm2 s TeV)")}
    s.modelfn = model
    e_range = [100 * u.MeV, 100 * u.GeV]
    n, confs = 30, [1, 2]
    pars = P._draw(s, n, False, 5)
    _, data = P._energy_grid(s, e_range, 24)
    ctx = _lib.get_context()
    with pytest.raises(NotImplementedError):
        try:
            model(DPars(ctx, ctx.array(np.ascontiguousarray(pars[:2].T)), 4, 2), data)
        finally:
            ctx.flush()
    mx, CI = P._calc_CI(s, 0, confs=confs, e_range=e_range, e_npoints=24, n_samples=n, seed=5)
    one = np.array([np.asarray(model(p, data).to("1/(cm2 s eV)").value) for p in pars])
    assert one.shape == (n, 24) and np.all(np.ptp(one, axis=0) > 0)
    want = np.sort(one, axis=0)[P._band_ranks(n, confs)]
    got = np.array([b.to("1/(cm2 s eV)").value for pair in CI for b in pair])
    bound = 1e-12 * np.max(np.abs(one), axis=0)
    assert np.all(np.abs(got - want) <= bound)


def test_wrong_output_shapes_and_indices_raise(cfg3_run):
    """a host batch that comes back as one spectrum, or with the parameters broadcast along the
    energies (n draws == n energies), is a wrong blob, not a band of copies; a bare output has
    no model 1"""
    from naima_amd import plot as P
    from naima_amd import units as u
    s, _ = cfg3_run

    class S:
        pass

    t = S()
    t.get_chain, t.data = s.get_chain, s.data
    e_range = [1 * u.keV, 10 * u.TeV]
    for bad in (lambda p, d: u.Quantity(np.ones(d["energy"].value.size), "1/(cm2 s eV)"),
                lambda p, d: u.Quantity(np.asarray(p[1]) * d["energy"].value, "1/(cm2 s eV)")):
        t.modelfn = bad
        with pytest.raises(TypeError, match="wrong blob format"):
            P._calc_CI(t, 0, e_range=e_range, e_npoints=50, n_samples=50, seed=1)
    t.modelfn = s.modelfn
    with pytest.raises(IndexError, match="no model 2"):
        P._calc_CI(t, 2, e_range=e_range, e_npoints=10, n_samples=10, seed=1)

    def bare(p, d):
        return s.modelfn(p, d)[0]

    t.modelfn = bare
    with pytest.raises(IndexError, match="no model 1"):
        P._calc_CI(t, 1, e_range=e_range, e_npoints=10, n_samples=10, seed=1)


def test_read_run_with_modelfn_replots_with_e_range(cfg3_run, tmp_path):
    from naima_amd import plot as P
    from naima_amd import units as u
    from naima_amd.analysis import read_run, save_run
    s, _ = cfg3_run
    fn = save_run(str(tmp_path / "run.npz"), s)
    r = read_run(fn, modelfn=s.modelfn)
    e_range = [1 * u.keV, 10 * u.TeV]
    a = P._calc_CI(r, 0, confs=[2], e_range=e_range, e_npoints=20, seed=6)
    b = P._calc_CI(s, 0, confs=[2], e_range=e_range, e_npoints=20, seed=6)
    for x, y in zip(a[1][0], b[1][0]):
        np.testing.assert_array_equal(x.value, y.to(x.unit).value)
    # ... and stored-blob bands of the saved run are those of the live sampler
    a, b = P._calc_CI(r, 0), P._calc_CI(s, 0)
    np.testing.assert_array_equal(a[1][0][0].value, b[1][0][0].to(a[1][0][0].unit).value)


def test_diagnostic_plots(cfg3_run, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    import naima_amd as na
    from naima_amd import plot as P
    from naima_amd.core import sed_conversion
    s, _ = cfg3_run
    out = str(tmp_path / "run")
    with pytest.warns(UserWarning, match="corner"):
        na.save_diagnostic_plots(out, s)
    for label in s.labels:
        if "log(" in label or "log10(" in label:
            label = label.split("(")[-1].split(")")[0]
        assert os.path.getsize("%s_chain_%s.png" % (out, label)) > 0, label
    assert os.path.getsize(out + "_model0.png") > 0
    assert os.path.getsize(out + "_model1.png") > 0
    na.save_diagnostic_plots(out, s, pdf=True)
    assert os.path.getsize(out + "_plots.pdf") > 0
    # the polygons of plot_fit's bands are _calc_CI's, SED-converted
    confs = [3, 1]
    f = na.plot_fit(s, 0, confs=confs, n_samples=None)
    ax = f.axes[0]
    polys = [c for c in ax.collections if type(c).__name__ in ("PolyCollection",
                                                               "FillBetweenPolyCollection")]
    assert len(polys) == 2
    mx, CI = P._calc_CI(s, 0, confs=confs)
    f_unit, sedf = sed_conversion(mx, CI[0][0].unit, True)
    x = mx.to(s.data["energy"].unit).value
    for poly, (lo, hi) in zip(polys, CI):
        v = poly.get_paths()[0].vertices
        pts = set(map(tuple, v.tolist()))
        for y in ((hi * sedf).to(f_unit).value, (lo * sedf).to(f_unit).value):
            assert all((xi, yi) in pts for xi, yi in zip(x, y))
    plt.close("all")
