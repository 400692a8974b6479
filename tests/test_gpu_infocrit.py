"""naima_amd.infocrit on the GPU (nh_pointwise_lnl, nh_lnl_column_stats, nh_psis_columns) against
the NumPy restatement tests/infocrit_np.py at rtol 1e-9, atol 1e-12 (DESIGN section 2's bound for
an entry point against its oracle): the pointwise terms over the wave stride's edges, units and
upper limits; the column statistics over the chunking's edges; PSIS below, at and above its
cut-in, with heavy tails and ties, deterministic and independent of the order of the rows; and a
whole fit, through save_run / read_run and save_results_table."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import infocrit_np as R  # noqa: E402
from test_infocrit_host import TABLES, normal_mean, ref_pointwise, spectra, table  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
ERG_PER_TEV = 1.602176634


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def padded(x, pad, fill=np.nan):
    host = np.full((x.shape[0], x.shape[1] + pad), fill)
    host[:, :x.shape[1]] = x
    return host


def on_device(x, pad=0):
    """x [M][ncol] inside a device matrix of ld = ncol + pad, the padding NaN"""
    M, ncol = x.shape
    return (ctx().array(padded(x, pad)), M, ncol, ncol + pad)


# ---------------------------------------------------------------------------------------
# 1. pointwise terms
# ---------------------------------------------------------------------------------------
def dev_pointwise(x, t, pad=0):
    """nh_pointwise_lnl through the C ABI: (L [M][nE], total [M], nbad), x and L inside matrices
    of ld = nE + pad whose padding must stay what it was"""
    c = ctx()
    M, nE = x.shape
    dx = c.array(padded(x, pad))
    dL = c.array(np.full((M, nE + pad), 7.0))
    tot, nbad = c.empty((M,)), c.empty((1,), np.int64)
    cl = np.concatenate([t["cl"], t["cl"][-1:]])
    c.call("nh_pointwise_lnl", dx, M, nE, nE + pad, c.array(t["conv"]), c.array(t["flux"]),
           c.array(t["flux_error_lo"]), c.array(t["flux_error_hi"]),
           c.array(t["ul"].astype(np.int32), dtype=np.int32), c.array(cl), dL, nE + pad, tot, nbad)
    L = dL.get()
    assert np.all(L[:, nE:] == 7.0)
    return L[:, :nE], tot.get(), int(nbad.get()[0])


@pytest.mark.parametrize("nE", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("M", [1, 3, 257])
def test_pointwise_against_the_restatement(nE, M):
    t = table("some-mixed", nE=nE, seed=nE)
    x = spectra(t, M, seed=M)
    want = ref_pointwise(x, t)
    for pad in (0, 3):
        L, tot, nbad = dev_pointwise(x, t, pad)
        np.testing.assert_allclose(L, want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(tot, L.sum(axis=1), rtol=RTOL, atol=ATOL)
        assert nbad == 0


@pytest.mark.parametrize("kind", TABLES)
def test_pointwise_upper_limits_and_confidence_levels(kind):
    from oracle import naima_np as O
    t = table(kind, nE=70)
    x = spectra(t, 9)
    L, tot, nbad = dev_pointwise(x, t, 1)
    np.testing.assert_allclose(L, ref_pointwise(x, t), rtol=RTOL, atol=ATOL)
    data = dict(t, cl=np.concatenate([t["cl"], t["cl"][-1:]]))
    want = [O.lnprobmodel(x[s] * t["conv"], data) for s in range(len(x))]
    np.testing.assert_allclose(tot, want, rtol=RTOL, atol=ATOL)
    assert nbad == 0


def make_table(flux_unit, t, energy):
    from naima_amd.datatable import make_data
    return make_data(dict(energy=energy, energy_unit="TeV", flux=t["flux"], flux_unit=flux_unit,
                          flux_error_lo=t["flux_error_lo"], flux_error_hi=t["flux_error_hi"],
                          ul=t["ul"], cl=t["cl"]))


@pytest.mark.parametrize("model_unit,data_unit", [("erg/(s cm2)", "1/(s cm2 TeV)"),
                                                  ("1/(s cm2 TeV)", "erg/(s cm2)"),
                                                  ("1/(s cm2 eV)", "1/(s cm2 TeV)")])
def test_pointwise_units(model_unit, data_unit):
    """SED model on differential data and the reverse: E^2 and the erg <-> TeV factor by hand"""
    from naima_amd import infocrit as IC
    from naima_amd import units as u
    nE = 21
    t = table("some-mixed", nE=nE)
    E = np.logspace(-1, 2, nE)
    conv = {"erg/(s cm2)": 1.0 / (ERG_PER_TEV * E ** 2), "1/(s cm2 TeV)": ERG_PER_TEV * E ** 2,
            "1/(s cm2 eV)": np.full(nE, 1e12)}[model_unit]
    t["conv"] = conv
    x = spectra(t, 5)
    data = make_table(data_unit, t, E)
    h, tot = IC.pointwise_log_likelihood(u.Quantity(x, model_unit), data, totals=True)
    want = ref_pointwise(x, t)
    np.testing.assert_allclose(h.get(), want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(tot.get(), want.sum(axis=1), rtol=RTOL, atol=ATOL)
    # the same spectra already on the device, with their unit
    h2 = IC.pointwise_log_likelihood(on_device(x, 2), data, unit=model_unit)
    np.testing.assert_array_equal(h2.get(), h.get())


def test_a_planted_nan_is_counted_and_raises():
    from naima_amd import infocrit as IC
    from naima_amd import units as u
    t = table("none-uniform", nE=66)
    x = spectra(t, 7)
    x[4, 65] = np.nan
    x[2, 0] = np.inf
    L, tot, nbad = dev_pointwise(x, t)
    assert nbad == 2 and np.isnan(L[4, 65]) and np.isinf(L[2, 0])
    assert np.isfinite(np.delete(L.ravel(), [4 * 66 + 65, 2 * 66])).all()
    t["conv"] = np.ones(66)
    data = make_table("1/(s cm2 TeV)", t, np.logspace(-1, 2, 66))
    with pytest.raises(ValueError, match="2 of the 462"):
        IC.pointwise_log_likelihood(u.Quantity(x, "1/(s cm2 TeV)"), data)


# ---------------------------------------------------------------------------------------
# 2. column statistics
# ---------------------------------------------------------------------------------------
def dev_stats(d):
    dev, M, ncol, ld = d
    st = ctx().empty((5, ncol))
    ctx().call("nh_lnl_column_stats", dev, M, ncol, ld, st)
    return st.get()


@pytest.mark.parametrize("ncol", [1, 5, 65])
@pytest.mark.parametrize("M", [1, 2, 1023, 1025, 4097])
def test_column_stats(M, ncol):
    """values from -700 down to -760: exp() of them is subnormal or zero unless the maximum is
    subtracted first"""
    rng = np.random.default_rng(M * 100 + ncol)
    L = -700.0 - 60.0 * rng.random((M, ncol)) ** 2
    if ncol > 1:
        L[:, 1] = -3.25  # a constant column: variance exactly 0
    d = on_device(L, 3)
    got = dev_stats(d)
    want = R.column_stats(L)
    for i, k in enumerate(("max", "mean", "var", "lse", "min")):
        np.testing.assert_allclose(got[i], want[k], rtol=RTOL, atol=ATOL, err_msg=k)
    assert np.all(np.isfinite(got[3]))
    if M == 1:
        assert np.all(np.isnan(got[2]))
    elif ncol > 1:
        assert got[2][1] == 0.0 and got[1][1] == -3.25
    assert dev_stats(d).tobytes() == got.tobytes()


def test_waic_against_the_restatement():
    from naima_amd import infocrit as IC
    L, _ = normal_mean(2, M=3001)
    got, want = IC.waic(L), R.waic(L)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v, rtol=RTOL, atol=ATOL, err_msg=k)
    assert got["n_samples"] == 3001 and got["n_data"] == 12
    # a device handle gives the same bits as the host array
    assert IC.waic(on_device(L, 1))["elpd_waic_i"].tobytes() == got["elpd_waic_i"].tobytes()


# ---------------------------------------------------------------------------------------
# 3. PSIS
# ---------------------------------------------------------------------------------------
PSIS_MS = [4, 24, 25, 100, 1000, 5000]


def psis_columns(M, seed=0):
    """[M][5]: light-tailed, heavy-tailed, constant, every value twice, ties exactly at the
    cutoff (the order statistic of rank Mt has copies above it in x: fewer than Mt tail rows)"""
    rng = np.random.default_rng(1000 + seed + M)
    light = -0.5 * (0.3 * rng.standard_normal(M) - 0.5) ** 2
    heavy = -0.5 * (8.0 * rng.standard_normal(M)) ** 2
    const = np.full(M, -3.0)
    dup = -0.5 * rng.standard_normal((M + 1) // 2) ** 2
    dup = rng.permutation(np.concatenate([dup, dup])[:M])
    ties = -0.5 * rng.standard_normal(M) ** 2
    Mt = R.tail_length(M)
    order = np.argsort(ties)
    ties[order[max(Mt - 2, 0):Mt + 1]] = ties[order[Mt]]  # L's rank-Mt value, three times
    return np.column_stack([light, heavy, const, dup, ties])


def check_loo(got, want):
    assert sorted(got) == sorted(want)
    np.testing.assert_array_equal(got["n_tail"], want["n_tail"])
    assert got["n_tail"].dtype == np.int64 and got["tail_length"] == want["tail_length"]
    np.testing.assert_array_equal(np.isposinf(got["pareto_k"]), np.isposinf(want["pareto_k"]))
    fin = np.isfinite(want["pareto_k"])
    np.testing.assert_allclose(got["pareto_k"][fin], want["pareto_k"][fin], rtol=RTOL, atol=ATOL)
    for k in ("elpd_loo_i", "lppd_i", "elpd_loo", "p_loo", "se"):
        np.testing.assert_allclose(got[k], want[k], rtol=RTOL, atol=ATOL, err_msg=k)


@pytest.mark.parametrize("M", PSIS_MS)
def test_psis_against_the_restatement(M):
    from naima_amd import infocrit as IC
    L = psis_columns(M)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = R.loo(L)
        d = on_device(L, 2)
        got = IC.loo(d)
        again = IC.loo(d)
    print("M %d: Mt %d, n_tail %s, pareto_k %s" % (M, want["tail_length"], want["n_tail"],
                                                   want["pareto_k"]))
    check_loo(got, want)
    Mt = want["tail_length"]
    assert Mt == {4: 0, 24: 4, 25: 5, 100: 20, 1000: 95, 5000: 213}[M]
    if Mt <= 4:
        assert np.all(np.isposinf(got["pareto_k"]))
    else:
        k = got["pareto_k"]
        assert np.isfinite(k[0]) and np.isposinf(k[2]) and got["n_tail"][2] == 0
        assert got["n_tail"][0] == Mt and got["n_tail"][4] < Mt
    if M >= 1000:
        assert got["pareto_k"][1] > 0.7 and got["pareto_k"][0] < 0.7
    for k in ("pareto_k", "n_tail", "elpd_loo_i"):
        assert got[k].tobytes() == again[k].tobytes(), k
    # the rows in another order: the tail's values are the same set, so k and n are the same
    # bits; elpd sums the rows below the cutoff in another order
    perm = np.random.default_rng(M).permutation(M)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        shuffled = IC.loo(L[perm])
    assert shuffled["pareto_k"].tobytes() == got["pareto_k"].tobytes()
    np.testing.assert_array_equal(shuffled["n_tail"], got["n_tail"])
    np.testing.assert_allclose(shuffled["elpd_loo_i"], got["elpd_loo_i"], rtol=1e-12, atol=1e-12)


def test_loo_warns_and_takes_reff():
    from naima_amd import infocrit as IC
    L = psis_columns(1000)
    with pytest.warns(UserWarning, match=r"of the 5 data points is above 0\.7"):
        IC.loo(L)
    light, _ = normal_mean(4, M=1000)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = IC.loo(light, reff=0.25)
        want = R.loo(light, reff=0.25)
    assert got["tail_length"] == 190
    check_loo(got, want)


def test_tail_cap_through_the_c_entry_point():
    from naima_amd import _lib
    c = ctx()
    M = 30000
    d = c.array(np.zeros((M, 1)))
    st, sel = c.empty((5, 1)), c.empty((1, 1))
    k, n, e = c.empty((1,)), c.empty((1,), np.int64), c.empty((1,))
    with pytest.raises(_lib.NaimaHipError, match="NH_PSIS_MAX_TAIL"):
        c.call("nh_psis_columns", d, M, 1, 1, 4097, st, sel, k, n, e)
    with pytest.raises(_lib.NaimaHipError, match="Mt outside"):
        c.call("nh_psis_columns", d, 10, 1, 1, 10, st, sel, k, n, e)


# ---------------------------------------------------------------------------------------
# 4. a whole fit
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


def host_pointwise(s, discard=0, thin=1):
    """the restatement on the downloaded blobs, converted by the fit's own factor"""
    from naima_amd.core import _conversion_to_data
    b = np.asarray(s.get_blobs(discard=discard, thin=thin)[0], dtype=float)
    d = s.data
    unit = d["flux"].unit
    cl = np.concatenate([d["cl"], d["cl"][-1:]])
    return R.pointwise_lnl(b.reshape(-1, b.shape[2]), _conversion_to_data(s.blob_units[0], d),
                           d["flux"].value, d["flux_error_lo"].to(unit).value,
                           d["flux_error_hi"].to(unit).value, d["ul"], cl)


def test_fit_row_sums_are_the_fits_own_likelihood(fit):
    L = fit.get_pointwise_log_likelihood().get()
    lp = np.asarray(fit.get_log_prob(flat=True))
    assert L.shape == (30 * 32, len(fit.data["energy"]))
    np.testing.assert_allclose(L.sum(axis=1), lp, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(L, host_pointwise(fit), rtol=RTOL, atol=ATOL)


def test_fit_loo_waic_discard_and_thin(fit):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        check_loo(fit.loo(), R.loo(host_pointwise(fit)))
        w, ww = fit.waic(), R.waic(host_pointwise(fit))
        for k, v in ww.items():
            np.testing.assert_allclose(w[k], v, rtol=RTOL, atol=ATOL, err_msg=k)
        Ld = fit.get_pointwise_log_likelihood(discard=7, thin=3).get()
        assert Ld.shape[0] == len(range(7, 30, 3)) * 32
        np.testing.assert_allclose(Ld, host_pointwise(fit, 7, 3), rtol=RTOL, atol=ATOL)
        lp = np.asarray(fit.get_log_prob(flat=True, discard=7, thin=3))
        np.testing.assert_allclose(Ld.sum(axis=1), lp, rtol=RTOL, atol=ATOL)
        check_loo(fit.loo(discard=7, thin=3), R.loo(host_pointwise(fit, 7, 3)))
    with pytest.raises(TypeError, match="Model 1 has wrong blob format"):
        fit.get_pointwise_log_likelihood(modelidx=1)


def test_fit_saved_read_and_tabulated(fit, tmp_path):
    import naima_amd as na
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo, w = fit.loo(), fit.waic()
        back = na.read_run(na.save_run(str(tmp_path / "run.npz"), fit))
        lb = back.loo()
        for k in ("elpd_loo_i", "pareto_k", "n_tail"):
            assert lb[k].tobytes() == lo[k].tobytes(), k
        assert back.waic()["elpd_waic_i"].tobytes() == w["elpd_waic_i"].tobytes()
        plain = na.save_results_table(str(tmp_path / "plain"), fit)
        full = na.save_results_table(str(tmp_path / "full"), fit, information_criteria=True)
    new = ["WAIC_elpd", "WAIC_p", "LOO_elpd", "LOO_p", "LOO_se", "LOO_max_pareto_k"]
    assert [k for k in full["meta"] if k not in plain["meta"]] == new
    assert {k: v for k, v in full["meta"].items() if k not in new} == plain["meta"]
    assert not set(new) & set(plain["meta"]) and "BIC" in plain["meta"]
    want = [w["elpd_waic"], w["p_waic"], lo["elpd_loo"], lo["p_loo"], lo["se"],
            float(np.max(lo["pareto_k"]))]
    assert [full["meta"][k] for k in new] == want
    text = open(str(tmp_path / "full_results.ecsv")).read()
    assert all(k in text for k in new)
    assert not any(k in open(str(tmp_path / "plain_results.ecsv")).read() for k in new)


# ---------------------------------------------------------------------------------------
# 5. the example
# ---------------------------------------------------------------------------------------
def test_the_example_compares_two_models():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "rxj1713_compare", os.path.join(ROOT, "examples", "rxj1713_compare.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        table_ = ex.main(nwalkers=32, nburn=5, nrun=20, verbose=False, prefit=False)
    assert sorted(r["name"] for r in table_) == ["ECPL", "PL"]
    assert [r["rank"] for r in table_] == [0, 1] and table_[0]["elpd_diff"] == 0.0
    assert table_[1]["elpd_diff"] <= 0.0 and table_[1]["dse"] >= 0.0
