"""naima_amd.predictive on the GPU (nh_ppc_rows, nh_ppc_counts, nh_pit_columns) against the NumPy
restatement tests/predictive_np.py at rtol 1e-9, atol 1e-12 (DESIGN section 2's bound for an entry
point against its oracle): replicates and row statistics over the wave stride's edges, with every
kind of table, independent of how the rows are cut into calls; the counts as integers; the PIT
over the chunking's edges and far in the lower tail; the public API with units; and a whole fit,
through save_run / read_run, save_results_table and plot_ppc."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import predictive_np as R  # noqa: E402
from test_infocrit_host import TABLES, spectra, table  # noqa: E402
from test_predictive_host import M as BUMP_M  # noqa: E402
from test_predictive_host import NE as BUMP_NE  # noqa: E402
from test_predictive_host import SEED, bump, power_law  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
ERG_PER_TEV = 1.602176634
FILL = 7.0


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def padded(x, pad, fill=np.nan):
    host = np.full((x.shape[0], x.shape[1] + pad), fill)
    host[:, :x.shape[1]] = x
    return host


def columns(c, t):
    """the data columns of a table() dict on the device, as the entry points take them"""
    return (c.array(t["conv"]), c.array(t["flux"]), c.array(t["flux_error_lo"]),
            c.array(t["flux_error_hi"]), c.array(t["ul"].astype(np.int32), dtype=np.int32))


def distinct(x, t):
    """the spectra with no model value equal to its datum (the helper's first rows are exact
    multiples of flux / conv: the runs statistic would hang on the last bit of a product)"""
    x = x * (1.0 + 1e-3 * np.sin(1.0 + np.arange(x.size).reshape(x.shape)))
    assert not np.any(x * t["conv"] == t["flux"])
    return x


def dev_rows(x, t, seed=0, row0=0, pad=0, want_y=True, want_t=True):
    """nh_ppc_rows through the C ABI: (Y [M][nE] or None, T [M][6] or None); x and Y inside
    matrices of ld = nE + pad whose padding must stay what it was"""
    c = ctx()
    M, nE = x.shape
    dx = c.array(padded(x, pad))
    dY = c.array(np.full((M, nE + pad), FILL)) if want_y else None
    dT = c.array(np.full((M, 6), FILL)) if want_t else None
    c.call("nh_ppc_rows", dx, M, nE, nE + pad, *columns(c, t), seed, row0, dY, nE + pad, dT)
    Y = T = None
    if want_y:
        Y = dY.get()
        assert np.all(Y[:, nE:] == FILL)
        Y = Y[:, :nE]
    if want_t:
        T = dT.get()
    return Y, T


def ref_rows(x, t, seed=0, row0=0):
    return R.ppc_rows(x, t["conv"], t["flux"], t["flux_error_lo"], t["flux_error_hi"], t["ul"],
                      seed, row0)


def check_rows(x, t, Y, T, seed=0, row0=0):
    wantY, wantT, below = ref_rows(x, t, seed, row0)
    ul = t["ul"]
    mc = x * t["conv"]
    if T is not None:
        np.testing.assert_allclose(T, wantT, rtol=RTOL, atol=ATOL)
        np.testing.assert_array_equal(T[:, 4:], wantT[:, 4:])  # runs: integers
    if Y is not None:
        scale = np.maximum(t["flux_error_lo"], t["flux_error_hi"])
        err = np.abs(Y - wantY)
        bound = 1e-9 * np.abs(wantY) + 1e-12 * scale
        print("largest |Y - want| / bound: %.3g" % np.max(err / bound))
        assert np.all(err <= bound)
        np.testing.assert_array_equal((Y < mc)[:, ~ul], below[:, ~ul])
        assert not np.any((Y == mc)[:, ~ul])
        assert Y[:, ul].tobytes() == mc[:, ul].tobytes()


# ---------------------------------------------------------------------------------------
# 1. replicates and row statistics
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nE", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("M", [1, 3, 257])
def test_rows_against_the_restatement(nE, M):
    t = table("some-mixed", nE=nE, seed=nE)
    x = distinct(spectra(t, M, seed=M), t)
    seed = 1000003 * nE + M
    for pad in (0, 3):
        Y, T = dev_rows(x, t, seed, pad=pad)
        check_rows(x, t, Y, T, seed)
        Yo, none = dev_rows(x, t, seed, pad=pad, want_t=False)
        none2, To = dev_rows(x, t, seed, pad=pad, want_y=False)
        assert none is None and none2 is None
        assert Yo.tobytes() == Y.tobytes() and To.tobytes() == T.tobytes()


@pytest.mark.parametrize("kind", TABLES)
def test_rows_with_every_kind_of_table(kind):
    from naima_amd import predictive as P
    from naima_amd import units as u
    t = table(kind, nE=70)
    x = distinct(spectra(t, 9), t)
    Y, T = dev_rows(x, t, 5, pad=1)
    check_rows(x, t, Y, T, 5)
    t1 = dict(t, conv=np.ones(70))
    data = make_table("1/(s cm2 TeV)", t1, np.logspace(-1, 2, 70))
    model = u.Quantity(x * t["conv"], "1/(s cm2 TeV)")
    if kind.startswith("only"):
        assert np.all(T == 0.0)
        with pytest.raises(ValueError, match="every data point is an upper limit"):
            P.ppc(model, data)
        pit, viol = P.pit(model, data)
        assert np.all(np.isnan(pit)) and np.all((viol >= 0.0) & (viol <= 1.0))
    else:
        assert np.all(T[:, :4] > 0.0) and np.all(T[:, 4:] >= 1.0)
        r = P.ppc(model, data, seed=5)
        assert r["n_points"] == 70 - t["ul"].sum() and r["n_ul"] == t["ul"].sum()
        assert r["n_samples"] == 9 and r["n_bad"] == 0
        assert np.array_equal(np.isnan(r["pit"]), t["ul"])
        assert np.array_equal(np.isnan(r["ul_violation"]), ~t["ul"])


def test_rows_do_not_depend_on_the_cut_and_do_on_the_seed():
    t = table("some-mixed", nE=70)
    x = distinct(spectra(t, 300), t)
    Y, T = dev_rows(x, t, 11)
    Ya, Ta = dev_rows(x[:130], t, 11, row0=0)
    Yb, Tb = dev_rows(x[130:], t, 11, row0=130)
    assert np.concatenate([Ya, Yb]).tobytes() == Y.tobytes()
    assert np.concatenate([Ta, Tb]).tobytes() == T.tobytes()
    again = dev_rows(x, t, 11)
    assert again[0].tobytes() == Y.tobytes() and again[1].tobytes() == T.tobytes()
    Y2, T2 = dev_rows(x, t, 12)
    assert np.all((Y2 != Y)[:, ~t["ul"]]) and np.all((Y2 == Y)[:, t["ul"]])
    # the seed's high word is part of the key, the row's high word part of the counter
    Y3, _ = dev_rows(x, t, 11 + 2 ** 32)
    assert np.all((Y3 != Y)[:, ~t["ul"]])
    Yh, Th = dev_rows(x, t, 11, row0=2 ** 32)
    assert np.all((Yh != Y)[:, ~t["ul"]])
    check_rows(x, t, Yh, Th, 11, row0=2 ** 32)
    check_rows(x, t, Y3, None, 11 + 2 ** 32)


# ---------------------------------------------------------------------------------------
# 2. counts
# ---------------------------------------------------------------------------------------
def dev_counts(T):
    c = ctx()
    d = T if hasattr(T, "ptr") else c.array(T)
    out = c.array(np.full(4, 99, dtype=np.int64), dtype=np.int64)
    c.call("nh_ppc_counts", d, T.shape[0], out)
    return out.get()


@pytest.mark.parametrize("M", [1, 257, 70001])
def test_counts_are_numpys(M):
    t = table("some-mixed", nE=12)
    x = distinct(spectra(t, M, seed=M), t)
    _, T = dev_rows(x, t, 3, want_y=False)
    got = dev_counts(T)
    assert got.dtype == np.int64 and got.tolist() == R.ppc_counts(T).tolist()
    assert got[3] == 0
    # planted ties (they count in all three), NaN and inf rows (they count in none)
    rng = np.random.default_rng(M)
    P = T.copy()
    ties = rng.random(M) < 0.3
    P[ties, 1], P[ties, 3], P[ties, 5] = P[ties, 0], P[ties, 2], P[ties, 4]
    bad = rng.random(M) < 0.2
    P[bad, rng.integers(0, 6, bad.sum())] = np.nan
    P[::7, 3] = np.inf
    got = dev_counts(P)
    want = R.ppc_counts(P)
    assert got.tolist() == want.tolist()
    assert got[3] == np.count_nonzero(bad | (np.arange(M) % 7 == 0))
    assert dev_counts(np.full((M, 6), np.nan)).tolist() == [0, 0, 0, M]


# ---------------------------------------------------------------------------------------
# 3. PIT
# ---------------------------------------------------------------------------------------
def dev_pit(x, t, pad=0):
    c = ctx()
    M, nE = x.shape
    dx = c.array(padded(x, pad))
    out = c.array(np.full((2, nE), FILL))
    cols = columns(c, t)
    c.call("nh_pit_columns", dx, M, nE, nE + pad, *cols, out)
    first = out.get()
    c.call("nh_pit_columns", dx, M, nE, nE + pad, *cols, out)
    assert out.get().tobytes() == first.tobytes()
    return first


@pytest.mark.parametrize("nE", [1, 65])
@pytest.mark.parametrize("M", [1, 257, 1025, 70001])
def test_pit_against_the_restatement(M, nE):
    """1025 rows are one row past a chunk of the column tiling, 70001 many chunks"""
    t = table("some-mixed" if nE > 1 else "none-uniform", nE=nE, seed=nE)
    x = spectra(t, M, seed=M)
    t["flux"][0] = (x[:, 0] * t["conv"][0]).min() - 30.0 * t["flux_error_hi"][0]  # 30 sigma below
    t["ul"][0] = False
    got = dev_pit(x, t, pad=2)
    want = R.pit_columns(x, t["conv"], t["flux"], t["flux_error_lo"], t["flux_error_hi"], t["ul"])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    print("pit of the far point: %.6g (%.6g)" % (got[0][0], want[0][0]))
    assert 0.0 < got[0][0] < 1e-150
    assert abs(got[0][0] / want[0][0] - 1.0) <= RTOL
    if nE > 1:
        assert np.array_equal(np.isnan(got[0]), t["ul"])
        assert np.array_equal(np.isnan(got[1]), ~t["ul"])


# ---------------------------------------------------------------------------------------
# 4. the public API
# ---------------------------------------------------------------------------------------
def make_table(flux_unit, t, energy):
    from naima_amd.datatable import make_data
    return make_data(dict(energy=energy, energy_unit="TeV", flux=t["flux"], flux_unit=flux_unit,
                          flux_error_lo=t["flux_error_lo"], flux_error_hi=t["flux_error_hi"],
                          ul=t["ul"], cl=t["cl"]))


def test_ppc_sees_the_bump():
    from naima_amd import predictive as P
    from naima_amd import units as u
    p = power_law()
    model, observed = bump()
    t = dict(flux=observed, flux_error_lo=p["elo"], flux_error_hi=p["ehi"], ul=p["ul"],
             cl=np.full(BUMP_NE, 0.9), conv=np.ones(BUMP_NE))
    data = make_table("1/(s cm2 TeV)", t, np.logspace(-1, 1, BUMP_NE))
    r = P.ppc(u.Quantity(model, "1/(s cm2 TeV)"), data, seed=SEED)
    T = r["T"].get()
    want = ref_rows(model, t, SEED)[1]
    np.testing.assert_allclose(T, want, rtol=RTOL, atol=ATOL)
    c = R.ppc_counts(T)
    print("p_chi2 %.4f  p_max %.4f  p_runs %.4f" % (r["p_chi2"], r["p_max"], r["p_runs"]))
    assert (r["n_bad"], r["n_samples"], r["n_points"], r["n_ul"]) == (0, BUMP_M, BUMP_NE, 0)
    assert [r["p_chi2"], r["p_max"], r["p_runs"]] == [c[0] / BUMP_M, c[1] / BUMP_M, c[2] / BUMP_M]
    assert r["p_chi2"] > 0.5 and r["p_runs"] < 0.05
    for j, name in ((0, "chi2_obs"), (1, "chi2_rep")):
        s = r[name]
        np.testing.assert_allclose(s["mean"], T[:, j].mean(), rtol=RTOL)
        np.testing.assert_allclose([s["q16"], s["median"], s["q84"]],
                                   np.percentile(T[:, j], [16, 50, 84]), rtol=1e-12)
    pit, viol = P.pit(u.Quantity(model, "1/(s cm2 TeV)"), data)
    assert pit.tobytes() == r["pit"].tobytes() and np.all(np.isnan(viol))
    np.testing.assert_allclose(pit, R.pit_columns(model, 1.0, observed, p["elo"], p["ehi"],
                                                  p["ul"])[0], rtol=RTOL, atol=ATOL)
    # a NaN spectrum is counted and left out
    model[17, 5] = np.nan
    r2 = P.ppc(u.Quantity(model, "1/(s cm2 TeV)"), data, seed=SEED)
    c2 = R.ppc_counts(r2["T"].get())
    assert r2["n_bad"] == 1 == c2[3] and r2["p_runs"] == c2[2] / (BUMP_M - 1)
    with pytest.raises(ValueError, match="none of the 2 samples"):
        P.ppc(u.Quantity(np.full((2, BUMP_NE), np.nan), "1/(s cm2 TeV)"), data)


@pytest.mark.parametrize("model_unit,data_unit", [("erg/(s cm2)", "1/(s cm2 TeV)"),
                                                  ("1/(s cm2 TeV)", "erg/(s cm2)"),
                                                  ("1/(s cm2 eV)", "1/(s cm2 TeV)")])
def test_units(model_unit, data_unit):
    """SED model on differential data and the reverse: E^2 and the erg <-> TeV factor by hand"""
    from naima_amd import predictive as P
    from naima_amd import units as u
    nE = 21
    t = table("some-mixed", nE=nE)
    E = np.logspace(-1, 2, nE)
    t["conv"] = {"erg/(s cm2)": 1.0 / (ERG_PER_TEV * E ** 2), "1/(s cm2 TeV)": ERG_PER_TEV * E ** 2,
                 "1/(s cm2 eV)": np.full(nE, 1e12)}[model_unit]
    x = distinct(spectra(t, 50), t)
    data = make_table(data_unit, t, E)
    r = P.ppc(u.Quantity(x, model_unit), data, seed=9)
    _, T = dev_rows(x, t, 9, want_y=False)
    np.testing.assert_allclose(r["T"].get(), T, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(r["T"].get()[:, 4:], T[:, 4:])
    y = P.posterior_predictive(u.Quantity(x, model_unit), data, seed=9)
    Yd, _ = dev_rows(x, t, 9, want_t=False)
    scale = np.maximum(t["flux_error_lo"], t["flux_error_hi"])
    assert np.all(np.abs(y.get() - Yd) <= 1e-9 * np.abs(Yd) + 1e-12 * scale)
    # the same spectra already on the device, with their unit; and cut in two
    dev = (ctx().array(padded(x, 2)), 50, nE, nE + 2)
    assert P.posterior_predictive(dev, data, unit=model_unit, seed=9).get().tobytes() \
        == y.get().tobytes()
    tail = P.posterior_predictive(u.Quantity(x[20:], model_unit), data, seed=9, row0=20)
    assert tail.get().tobytes() == y.get()[20:].tobytes()
    # exact order statistics per energy
    q = [0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0]
    np.testing.assert_allclose(P.predictive_quantiles(y, q),
                               np.percentile(y.get(), 100 * np.array(q), axis=0), rtol=1e-12)
    np.testing.assert_allclose(P.predictive_quantiles(y.get(), [0.5])[0],
                               np.median(y.get(), axis=0), rtol=1e-12)


# ---------------------------------------------------------------------------------------
# 5. a whole fit
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit():
    import naima_amd as na
    from bench import build_problem
    model, p0, raw, data, prior, labels = build_problem("cfg1", na)
    s, pos = na.get_sampler(data_table=data, p0=p0, model=model, prior=None, nwalkers=32, nburn=5,
                            labels=list(labels), seed=3, verbose=False, guess=False)
    s, pos = na.run_sampler(nrun=30, sampler=s, pos=pos, verbose=False)
    return s


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "T":
            assert a[k].get().tobytes() == b[k].get().tobytes()
        elif isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_fit_ppc_is_ppc_of_the_blobs(fit):
    from naima_amd import predictive as P
    from naima_amd import units as u
    b = np.asarray(fit.get_blobs()[0], dtype=float)
    model = u.Quantity(b.reshape(-1, b.shape[2]), fit.blob_units[0])
    r = fit.ppc(seed=4)
    same(r, P.ppc(model, fit.data, seed=4))
    assert r["n_samples"] == 30 * 32 and r["n_bad"] == 0
    assert r["n_points"] + r["n_ul"] == len(fit.data["energy"])
    assert all(0.0 <= r[k] <= 1.0 for k in ("p_chi2", "p_max", "p_runs"))
    # chi2_obs is -2 x the likelihood of a table without violated upper limits
    if r["n_ul"] == 0:
        lp = np.asarray(fit.get_log_prob(flat=True))
        np.testing.assert_allclose(r["T"].get()[:, 0], -2.0 * lp, rtol=RTOL, atol=ATOL)
    y = fit.get_posterior_predictive(seed=4)
    assert y.get().tobytes() == P.posterior_predictive(model, fit.data, seed=4).get().tobytes()
    rd = fit.ppc(discard=7, thin=3, seed=4)
    bd = np.asarray(fit.get_blobs(discard=7, thin=3)[0], dtype=float)
    same(rd, P.ppc(u.Quantity(bd.reshape(-1, bd.shape[2]), fit.blob_units[0]), fit.data, seed=4))
    assert rd["n_samples"] == len(range(7, 30, 3)) * 32
    with pytest.raises(TypeError, match="Model 1 has wrong blob format"):
        fit.ppc(modelidx=1)


def test_fit_saved_read_and_tabulated(fit, tmp_path):
    import naima_amd as na
    r = fit.ppc()
    back = na.read_run(na.save_run(str(tmp_path / "run.npz"), fit))
    same(back.ppc(), r)
    assert back.get_posterior_predictive(seed=2).get().tobytes() \
        == fit.get_posterior_predictive(seed=2).get().tobytes()
    plain = na.save_results_table(str(tmp_path / "plain"), fit)
    full = na.save_results_table(str(tmp_path / "full"), fit, goodness_of_fit=True)
    off = na.save_results_table(str(tmp_path / "off"), fit, goodness_of_fit=False)
    new = ["PPC_p_chi2", "PPC_p_max", "PPC_p_runs", "PPC_chi2_obs_mean"]
    assert [k for k in full["meta"] if k not in plain["meta"]] == new
    assert {k: v for k, v in full["meta"].items() if k not in new} == plain["meta"]
    assert [full["meta"][k] for k in new] == [r["p_chi2"], r["p_max"], r["p_runs"],
                                              r["chi2_obs"]["mean"]]
    text = open(str(tmp_path / "full_results.ecsv")).read()
    assert all(k in text for k in new)
    # without the flag the file is, byte for byte, what it is with the flag off
    plain_text = open(str(tmp_path / "plain_results.ecsv"), "rb").read()
    assert plain_text == open(str(tmp_path / "off_results.ecsv"), "rb").read()
    assert b"PPC_" not in plain_text and off["meta"] == plain["meta"]


def test_plot_ppc_returns_a_figure(fit):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    from naima_amd.plot import plot_ppc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = plot_ppc(fit, seed=4)
    assert len(f.axes) == 2
    r = fit.ppc(seed=4)
    assert "%.3f" % r["p_runs"] in f.axes[0].get_title()
    assert f.axes[1].get_ylabel() == "PIT"
    import matplotlib.pyplot as plt
    plt.close(f)


# ---------------------------------------------------------------------------------------
# 6. the example
# ---------------------------------------------------------------------------------------
def test_the_example_checks_two_models():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "rxj1713_ppc", os.path.join(ROOT, "examples", "rxj1713_ppc.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ex.main(nwalkers=32, nburn=5, nrun=20, verbose=False, prefit=False)
    assert sorted(res) == ["ECPL", "PL"]
    for r in res.values():
        assert r["n_samples"] == 10 * 32 and r["n_bad"] == 0 and r["n_points"] > 0
        assert all(0.0 <= r[k] <= 1.0 for k in ("p_chi2", "p_max", "p_runs"))
        assert np.all(np.isfinite(r["pit"]) | np.isfinite(r["ul_violation"]))


# ---------------------------------------------------------------------------------------
# 7. argument errors through the C ABI
# ---------------------------------------------------------------------------------------
def test_argument_errors():
    from naima_amd import _lib
    c = ctx()
    t = table("some-mixed", nE=5)
    cols = columns(c, t)
    x, Y, T = c.array(np.ones((4, 5))), c.array(np.ones((4, 5))), c.array(np.ones((4, 6)))
    out, cnt = c.empty((2, 5)), c.empty((4,), np.int64)
    E = _lib.NaimaHipError

    def rows(M=4, nE=5, ld=5, cols=cols, x=x, Y=Y, ldY=5, T=T, row0=0):
        c.call("nh_ppc_rows", x, M, nE, ld, *cols, 1, row0, Y, ldY, T)

    rows()
    for kw, msg in ((dict(M=0), "M == 0"), (dict(M=2 ** 31), "2\\^31"), (dict(nE=0), "positive"),
                    (dict(nE=5, ld=4), "ncol > ld"), (dict(ldY=4), "nE > ldY"),
                    (dict(Y=None, T=None), "both NULL"), (dict(x=None), "null"),
                    (dict(row0=-1), "row0"),
                    (dict(cols=cols[:4] + (None,)), "null"), (dict(cols=(None,) + cols[1:]), "null")):
        with pytest.raises(E, match=msg):
            rows(**kw)
    rows(Y=None, ldY=0)  # (ldY is not looked at without Y)
    for args, msg in (((None, 4, cnt), "null"), ((T, 4, None), "null"), ((T, 0, cnt), "M == 0")):
        with pytest.raises(E, match=msg):
            c.call("nh_ppc_counts", *args)
    for args, msg in (((x, 0, 5, 5) + cols + (out,), "M == 0"),
                      ((x, 4, 5, 4) + cols + (out,), "ncol > ld"),
                      ((x, 4, 5, 5) + cols + (None,), "null"),
                      ((None, 4, 5, 5) + cols + (out,), "null")):
        with pytest.raises(E, match=msg):
            c.call("nh_pit_columns", *args)
    c.sync()
