"""naima_amd.evidence on the GPU (nh_chain_cov, nh_mvn_draw, nh_mvn_logpdf, nh_bridge_l2,
nh_bridge_sums) against the NumPy restatement tests/evidence_np.py at rtol 1e-9, atol 1e-12 (DESIGN
section 2's bound for an entry point against its oracle; integers and exact zeros exact): the
covariance and the proposal's density over the chunking's edges, for a chain's pooled rows and a
padded matrix; the draws independent of how the rows are cut into calls and apart from the
replicates' stream; the iteration's sums at +-800 and -inf, bit-identical from call to call; and
the estimator end to end -- a sampled Gaussian against its closed form, a naima fit read from the
device loop's history block against the same chain uploaded, save_results_table and the example."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import evidence_np as E  # noqa: E402
import predictive_np as R  # noqa: E402
from test_predictive_host import SEED as PPC_SEED  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
FILL = 7.0
NROWS = (1, 3, 257, 1025, 2 * 1024 + 1)  # (the last two cross PO_MIN_ROWS = 1024 rows a chunk)


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def factor(d, seed=0):
    """(mean [d], L [d][d]) of a correlated normal"""
    rng = np.random.default_rng(50 + d + seed)
    A = rng.normal(size=(d, d))
    return 10.0 * rng.normal(size=d), np.linalg.cholesky(A @ A.T + d * np.eye(d))


def block(nrows, npool, d, row0, pad, seed):
    """(flat buffer [row0 + nrows][ld], ld, cstride): correlated pooled rows far from the origin
    (the second pass has something to centre), NaN in every padding cell and in the rows in front
    of row0 (none of them may be read)"""
    rng = np.random.default_rng(seed)
    mean, L = factor(d)
    cstride = d if npool > 1 else 0
    ld = npool * d + pad
    buf = np.full((row0 + nrows, ld), np.nan)
    x = mean + rng.normal(size=(nrows, npool, d)) @ L.T
    buf[row0:, :npool * d] = x.reshape(nrows, npool * d)
    return buf, ld, cstride


def dev_cov(buf, row0, nrows, ld, cstride, npool, d):
    c = ctx()
    mean, cov = c.array(np.full(d, FILL)), c.array(np.full((d, d), FILL))
    c.call("nh_chain_cov", c.array(buf), row0, nrows, ld, cstride, npool, d, mean, cov)
    return mean.get(), cov.get()


def dev_logpdf(buf, row0, nrows, ld, cstride, npool, d, mean, L, lp=None):
    c = ctx()
    out = c.array(np.full(nrows * npool, FILL))
    c.call("nh_mvn_logpdf", c.array(buf), row0, nrows, ld, cstride, npool, d, c.array(mean),
           c.array(L), None if lp is None else c.array(lp), out)
    return out.get()


# ---------------------------------------------------------------------------------------
# 1. covariance and density
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("npool", [1, 4])
@pytest.mark.parametrize("d", [1, 2, 5, 32])
def test_cov_and_logpdf_against_the_restatement(d, npool):
    mean, L = factor(d, 1)
    for nrows in NROWS:
        row0, pad = 2, 3
        buf, ld, cs = block(nrows, npool, d, row0, pad, seed=1000 * d + nrows)
        rows = E.pooled(buf, row0, nrows, ld, cs, npool, d)
        S = nrows * npool
        m, cov = dev_cov(buf, row0, nrows, ld, cs, npool, d)
        with np.errstate(all="ignore"):
            wm, wc = E.chain_cov(rows)
        np.testing.assert_allclose(m, wm, rtol=RTOL, atol=ATOL)
        if S == 1:
            assert np.all(np.isnan(cov))  # (documented: 0 / 0)
        else:
            np.testing.assert_allclose(cov, wc, rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(cov, np.cov(rows, rowvar=False).reshape(d, d), rtol=RTOL,
                                       atol=ATOL)
        assert cov.tobytes() == cov.T.copy().tobytes()  # (exactly symmetric)
        got = dev_logpdf(buf, row0, nrows, ld, cs, npool, d, mean, L)
        np.testing.assert_allclose(got, E.mvn_logpdf(rows, mean, L), rtol=RTOL, atol=ATOL)
        lp = np.random.default_rng(nrows).normal(size=S) * 30
        got = dev_logpdf(buf, row0, nrows, ld, cs, npool, d, mean, L, lp)
        np.testing.assert_allclose(got, lp - E.mvn_logpdf(rows, mean, L), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("npool", [1, 4])
def test_cov_and_logpdf_with_one_nan_cell(npool):
    d, nrows, row0 = 5, 1025, 1
    mean, L = factor(d, 1)
    for bad in (np.nan, np.inf, -np.inf):
        buf, ld, cs = block(nrows, npool, d, row0, 2, seed=9)
        buf[row0 + 700, (npool - 1) * d + 3] = bad  # column 3 of the last walker of a row
        rows = E.pooled(buf, row0, nrows, ld, cs, npool, d)
        e = 700 * npool + npool - 1
        assert not np.isfinite(rows[e, 3]) and np.isfinite(np.delete(rows, e, 0)).all()
        m, cov = dev_cov(buf, row0, nrows, ld, cs, npool, d)
        wm, wc = E.chain_cov(rows)
        mask = np.zeros((d, d), bool)
        mask[3, :] = mask[:, 3] = True
        assert np.array_equal(np.isnan(cov), mask)
        assert np.array_equal(np.isnan(m), np.arange(d) == 3)
        np.testing.assert_allclose(m, wm, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(cov, wc, rtol=RTOL, atol=ATOL)
        got = dev_logpdf(buf, row0, nrows, ld, cs, npool, d, mean, L)
        want = E.mvn_logpdf(rows, mean, L)
        assert np.isnan(got[e]) and np.isnan(want[e]) and np.isnan(got).sum() == 1
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def test_posterior_covariance():
    from naima_amd import posterior as P
    rng = np.random.default_rng(12)
    chain = 3.0 + rng.normal(size=(40, 6, 3)) @ rng.normal(size=(3, 3))
    flat = chain[5:].reshape(-1, 3)
    for x, kw in ((chain, dict(discard=5)), (flat, {}), (chain[5:], {}),
                  ((ctx().array(chain.reshape(40, 18)), 40, 6, 3), dict(discard=5))):
        m, cov = P.covariance(x, **kw)
        np.testing.assert_allclose(m, flat.mean(axis=0), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(cov, np.cov(flat, rowvar=False), rtol=RTOL, atol=ATOL)
    m, cov = P.covariance(flat[:, 0])
    np.testing.assert_allclose(cov, [[flat[:, 0].var(ddof=1)]], rtol=RTOL)


# ---------------------------------------------------------------------------------------
# 2. the draws
# ---------------------------------------------------------------------------------------
def dev_draw(mean, L, n, seed=0, row0=0, pad=2, into=None, at=0):
    """nh_mvn_draw: (theta [n][d], z2 [n]); ``into`` = (out buffer, z2 buffer, rows) writes rows
    [at, at + n) of a larger pair instead"""
    c = ctx()
    d = len(mean)
    ld = d + pad
    if into is None:
        into = (c.array(np.full((n, ld), FILL)), c.array(np.full(n, FILL)), n)
    out, z2, rows = into
    assert at + n <= rows
    c.call("nh_mvn_draw", c.array(mean), c.array(L), d, seed, row0, n, out.ptr + 8 * at * ld, ld,
           z2.ptr + 8 * at)
    host = out.get()
    assert np.all(host[:, d:] == FILL)  # (padding is not written)
    return host[:, :d], z2.get(), into


@pytest.mark.parametrize("d", [1, 2, 5, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_draws_against_the_restatement(n, d):
    mean, L = factor(d, 2)
    seed = 1000003 * n + d
    th, z2, _ = dev_draw(mean, L, n, seed)
    wt, wz = E.mvn_draw(mean, L, n, seed)
    np.testing.assert_allclose(th, wt, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(z2, wz, rtol=RTOL, atol=ATOL)


def test_draws_do_not_depend_on_the_cut_and_do_on_the_seed():
    c = ctx()
    for d in (5, 32):
        mean, L = factor(d, 3)
        n, cut, ld = 257, 100, d + 2
        th, z2, _ = dev_draw(mean, L, n, seed=77)
        pair = (c.array(np.full((n, ld), FILL)), c.array(np.full(n, FILL)), n)
        dev_draw(mean, L, cut, seed=77, row0=0, into=pair, at=0)
        t2, y2, _ = dev_draw(mean, L, n - cut, seed=77, row0=cut, into=pair, at=cut)
        assert t2.tobytes() == th.tobytes() and y2.tobytes() == z2.tobytes()
        # a later window of the same stream, and another seed
        t3, _, _ = dev_draw(mean, L, 57, seed=77, row0=200)
        assert t3.tobytes() == th[200:].tobytes()
        t4, _, _ = dev_draw(mean, L, n, seed=78)
        assert not np.any(t4 == th)
        # rows beyond 2^32 take the counter's second word
        t5, _, _ = dev_draw(mean, L, 3, seed=77, row0=2 ** 32 + 5)
        np.testing.assert_allclose(t5, E.mvn_draw(mean, L, 3, 77, row0=2 ** 32 + 5)[0], rtol=RTOL,
                                   atol=ATOL)


def test_the_proposal_stream_is_not_the_replicates():
    n, d = 2000, 4
    z, z2, _ = dev_draw(np.zeros(d), np.eye(d), n, seed=PPC_SEED)
    np.testing.assert_allclose(z, E.normals(n, d, seed=PPC_SEED), rtol=RTOL, atol=ATOL)
    a, below = R.draw(n, d, np.ones(d), np.ones(d), seed=PPC_SEED)
    ppc = np.where(below, -a, a)
    assert not np.any(np.isclose(np.abs(z), np.abs(ppc), rtol=1e-9, atol=0))
    assert abs(np.corrcoef(z.ravel(), ppc.ravel())[0, 1]) < 4 / math.sqrt(z.size)
    assert abs(np.corrcoef(np.abs(z).ravel(), np.abs(ppc).ravel())[0, 1]) < 4 / math.sqrt(z.size)
    assert not np.any(np.isclose(z, E.normals(n, d, seed=PPC_SEED, stream=0), rtol=1e-9, atol=0))


# ---------------------------------------------------------------------------------------
# 3. the iteration's sums
# ---------------------------------------------------------------------------------------
def series(N, seed):
    l = 3.0 * np.random.default_rng(seed).normal(size=N) + 0.3
    for i, v in enumerate((800.3, -799.7, -np.inf)):
        if N > 2 * i + 1:
            l[2 * i + 1] = v
    return l


def dev_sums(l1, l2, lstar, s1, s2, r, terms=True):
    c = ctx()
    out = c.array(np.full(2, FILL))
    f1 = c.array(np.full(len(l2), FILL)) if terms else None
    f2 = c.array(np.full(len(l1), FILL)) if terms else None
    c.call("nh_bridge_sums", c.array(l1), len(l1), c.array(l2), len(l2), lstar, s1, s2, r, out,
           f1, f2)
    return out.get(), (f1.get() if terms else None), (f2.get() if terms else None)


@pytest.mark.parametrize("N2", [1, 255, 257, 2049])
@pytest.mark.parametrize("N1", [1, 255, 257, 2049])
def test_sums_against_the_restatement(N1, N2):
    l1, l2 = series(N1, N1), series(N2, 7 * N2)
    lstar, s1, s2, r = 0.3, 0.4, 0.6, 2.5
    out, f1, f2 = dev_sums(l1, l2, lstar, s1, s2, r)
    w1, w2 = E.bridge_terms(l1, l2, lstar, s1, s2, r)
    np.testing.assert_allclose(f1, w1, rtol=RTOL, atol=0)
    np.testing.assert_allclose(f2, w2, rtol=RTOL, atol=0)
    assert np.array_equal(f1 == 0.0, w1 == 0.0) and np.array_equal(f2 == 0.0, w2 == 0.0)
    assert np.all(f1[~np.isfinite(l2)] == 0.0)  # (a forbidden proposal: exactly nothing)
    if N2 > 3:
        assert f1[1] == 1.0 / s1 and f1[3] == 0.0 and f1[5] == 0.0
    if N1 > 3:
        assert f2[1] == 0.0 and f2[3] == 1.0 / (s2 * r)
    np.testing.assert_allclose(out, [w1.sum(), w2.sum()], rtol=RTOL, atol=ATOL)
    again, g1, g2 = dev_sums(l1, l2, lstar, s1, s2, r)
    assert again.tobytes() == out.tobytes() and g1.tobytes() == f1.tobytes() \
        and g2.tobytes() == f2.tobytes()
    bare, _, _ = dev_sums(l1, l2, lstar, s1, s2, r, terms=False)
    assert bare.tobytes() == out.tobytes()


def test_l2_from_the_draws_own_z2():
    c = ctx()
    for d in (1, 5, 32):
        mean, L = factor(d, 4)
        n = 300
        th, z2, _ = dev_draw(mean, L, n, seed=d)
        lp = np.random.default_rng(d).normal(size=n) * 20
        lp[::7] = -np.inf
        out = c.array(np.full(n, FILL))
        c.call("nh_bridge_l2", c.array(lp), c.array(z2), n, c.array(L), d, out)
        got = out.get()
        np.testing.assert_allclose(got, E.bridge_l2(lp, z2, L), rtol=RTOL, atol=ATOL)
        assert np.all(got[::7] == -np.inf)
        # the density |z|^2 implies is the density at the draw
        fin = np.isfinite(lp)
        np.testing.assert_allclose(got[fin], (lp - E.mvn_logpdf(th, mean, L))[fin], rtol=1e-7,
                                   atol=1e-9)


# ---------------------------------------------------------------------------------------
# 4. end to end: a sampled Gaussian
# ---------------------------------------------------------------------------------------
def test_gaussian_evidence_from_a_sampled_chain():
    from naima_amd import evidence as V
    from naima_amd.sampler import EnsembleSampler
    d, nw, steps, c0 = 3, 64, 400, -2.5
    mean, L = factor(d, 5)
    mean = mean / 10.0
    cov = L @ L.T
    prec = np.linalg.inv(cov)

    def fn(t):
        return c0 - 0.5 * np.einsum("ni,ij,nj->n", t - mean, prec, t - mean)

    exact = c0 + 0.5 * d * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(cov)[1]
    s = EnsembleSampler(nw, d, fn, seed=5)
    start = mean + np.random.default_rng(5).normal(size=(nw, d)) @ L.T  # (posterior draws)
    s.run_mcmc(start, steps)
    r = s.log_evidence(seed=3)
    print("logz %.5f exact %.5f err %.4f is %.5f it %d neff %.0f of %d" % (
        r["logz"], exact, r["logz_err"], r["logz_is"], r["iterations"], r["neff"], r["n_post"]))
    assert r["converged"] and r["n_post"] == r["n_draws"] == nw * steps // 2
    assert 1.0 <= r["neff"] <= r["n_post"] and r["forbidden_fraction"] == 0.0
    assert 0.0 < r["logz_err"] < 0.05
    assert abs(r["logz"] - exact) <= 4 * r["logz_err"]
    assert abs(r["logz_is"] - exact) < 0.1
    np.testing.assert_allclose(r["mean"], mean, atol=0.5)
    # the functional API on the downloaded chain, and on the same chain as a device block
    chain, lp = s.get_chain(), s.get_log_prob()
    h = V.bridge_sampling(chain, lp, fn, seed=3)
    c = ctx()
    blk = V.bridge_sampling((c.array(chain.reshape(steps, nw * d)), steps, nw, d), c.array(lp), fn,
                            seed=3)
    for o in (h, blk):
        for k in ("logz", "logz_err", "logz_is", "neff"):
            np.testing.assert_allclose(o[k], r[k], rtol=RTOL, atol=ATOL)
        assert o["iterations"] == r["iterations"]
    # against the restatement on the same halves (tau and neff taken from the device's result)
    # (bound: the iteration stops at a relative change of r below 1e-10, and the kernels agree
    # with the restatement to 1e-9 relative, on a logz of order 1)
    half = steps // 2
    want = E.bridge_sampling(chain[:half].reshape(-1, d), chain[half:].reshape(-1, d),
                             lp[half:].ravel(), fn, seed=3, neff=r["neff"])
    np.testing.assert_allclose(r["logz"], want["logz"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["logz_is"], want["logz_is"], rtol=1e-9, atol=1e-9)
    assert r["iterations"] == want["iterations"]
    # log_prior_norm shifts, discard and n_draws are honoured, maxiter warns
    q = s.log_evidence(seed=3, log_prior_norm=1.25, discard=100, n_draws=1000)
    assert q["n_post"] == nw * 150 and q["n_draws"] == 1000
    assert abs(q["logz"] + 1.25 - exact) <= 4 * q["logz_err"]
    with pytest.warns(UserWarning, match="did not converge"):
        w = s.log_evidence(seed=3, maxiter=1)
    assert not w["converged"] and w["iterations"] == 1
    with pytest.raises(ValueError, match="NaN"):
        V.bridge_sampling(chain, lp, lambda t: np.full(len(t), np.nan))
    with pytest.raises(ValueError, match="forbidden"):
        V.bridge_sampling(chain, lp, lambda t: np.full(len(t), -np.inf))
    bad = lp.copy()
    bad[300, 7] = -np.inf
    with pytest.raises(ValueError, match="non-finite"):
        V.bridge_sampling(chain, bad, fn)
    flatc = chain.copy()
    flatc[:, :, 2] = 1.0  # (a parameter that never moved)
    with pytest.raises(ValueError, match="positive definite"):
        V.bridge_sampling(flatc, lp, fn)


# ---------------------------------------------------------------------------------------
# 5. end to end: a naima fit on the device loop, the table, the example
# ---------------------------------------------------------------------------------------
def example():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "rxj1713_evidence", os.path.join(ROOT, "examples", "rxj1713_evidence.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


@pytest.fixture(scope="module")
def fit():
    ex = example()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (a monitored run that cannot converge before its last row: one history block in HBM)
        # from the prefit's maximum-likelihood point, so that the short chain is a stationary one
        s = ex.fit("PL", ex.make_data_table(), nwalkers=32, nburn=50, nrun=100, prefit=True,
                   converge=dict(check_every=50, tol=1e6))
    return ex, s


def test_fit_evidence_from_the_history_block(fit):
    from naima_amd import evidence as V
    ex, s = fit
    assert s._chain_block(1) is not None  # (the device loop still holds the chain in HBM)
    vol = ex.log_volume(ex.BOUNDS["PL"])
    r = s.log_evidence(log_prior_norm=vol, seed=2)
    print({k: v for k, v in r.items() if k not in ("mean", "cov")})
    assert s._chain_block(1) is not None  # (and reading it flushed nothing)
    for k in ("logz", "logz_err", "logz_is", "forbidden_fraction", "neff"):
        assert np.isfinite(r[k]), k
    assert r["n_post"] == 50 * 32 and 0.0 <= r["forbidden_fraction"] < 1.0
    assert r["cov"].shape == (3, 3) and np.all(np.linalg.eigvalsh(r["cov"]) > 0)
    # the block path against the upload path: the same chain downloaded
    chain, lp = s.get_chain(), s.get_log_prob()

    def fn(theta):
        return s.compute_log_prob(np.ascontiguousarray(theta))[0]

    h = V.bridge_sampling(chain, lp, fn, log_prior_norm=vol, seed=2)
    for k in ("logz", "logz_err", "logz_is", "neff", "forbidden_fraction"):
        np.testing.assert_allclose(h[k], r[k], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(h["cov"], r["cov"], rtol=RTOL, atol=0)
    assert s.log_evidence(seed=2)["logz"] == pytest.approx(r["logz"] + vol, rel=1e-12)


def test_fit_tabulated(fit, tmp_path):
    import naima_amd as na
    ex, s = fit
    r = s.log_evidence()
    plain = na.save_results_table(str(tmp_path / "plain"), s)
    full = na.save_results_table(str(tmp_path / "full"), s, evidence=True)
    given = na.save_results_table(str(tmp_path / "given"), s, evidence=r)
    off = na.save_results_table(str(tmp_path / "off"), s, evidence=None)
    new = ["logZ", "logZ_err", "logZ_forbidden_fraction"]
    assert [k for k in full["meta"] if k not in plain["meta"]] == new
    assert {k: v for k, v in full["meta"].items() if k not in new} == plain["meta"]
    assert [full["meta"][k] for k in new] == [r["logz"], r["logz_err"], r["forbidden_fraction"]]
    assert given["meta"] == full["meta"]
    text = open(str(tmp_path / "full_results.ecsv")).read()
    assert all(k in text for k in new)
    plain_text = open(str(tmp_path / "plain_results.ecsv"), "rb").read()
    assert plain_text == open(str(tmp_path / "off_results.ecsv"), "rb").read()
    assert b"logZ" not in plain_text and off["meta"] == plain["meta"]
    with pytest.raises(ValueError):
        na.save_results_table(str(tmp_path / "bad"), s, evidence=dict(logz=1.0))
    back = na.read_run(na.save_run(str(tmp_path / "run.npz"), s))
    assert not hasattr(back, "log_evidence")  # (no log-probability function: the functional API)
    with pytest.raises(ValueError, match="log-probability function"):
        na.save_results_table(str(tmp_path / "read"), back, evidence=True)


def test_the_example_weighs_two_models():
    ex = example()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ex.main(nwalkers=32, nburn=30, nrun=60, verbose=False, prefit=True)
    print({k: (v if k == "log_bayes_factor" else (v["logz"], v["logz_err"], v["iterations"],
                                                   v["forbidden_fraction"]))
           for k, v in res.items()})
    assert sorted(res) == ["ECPL", "PL", "log_bayes_factor"]
    for name in ("ECPL", "PL"):
        r = res[name]
        assert r["n_post"] == 30 * 32 and np.isfinite(r["logz"]) and r["logz_err"] >= 0.0
        assert r["mean"].shape == (len(ex.BOUNDS[name]),)
    lb, err = res["log_bayes_factor"]
    assert lb == res["ECPL"]["logz"] - res["PL"]["logz"] and np.isfinite(lb)


# ---------------------------------------------------------------------------------------
# 6. argument errors through the C ABI
# ---------------------------------------------------------------------------------------
def test_argument_errors():
    from naima_amd import _lib
    c = ctx()
    x, v, m = c.array(np.zeros((4, 6))), c.array(np.zeros(64)), c.array(np.zeros((33, 33)))
    for name, args in (
            ("nh_chain_cov", (None, 0, 4, 6, 3, 2, 3, v, m)),
            ("nh_chain_cov", (x, -1, 4, 6, 3, 2, 3, v, m)),
            ("nh_chain_cov", (x, 0, 0, 6, 3, 2, 3, v, m)),
            ("nh_chain_cov", (x, 0, 4, 6, 3, 2, 0, v, m)),
            ("nh_chain_cov", (x, 0, 4, 6, 2, 2, 3, v, m)),     # cstride < d
            ("nh_chain_cov", (x, 0, 4, 6, 3, 2, 4, v, m)),     # past ld
            ("nh_chain_cov", (x, 0, 4, 40, 0, 1, 33, v, m)),   # d > NH_EVID_MAX_DIM
            ("nh_mvn_logpdf", (x, 0, 4, 6, 3, 2, 3, v, None, None, v)),
            ("nh_mvn_logpdf", (x, 0, 4, 6, 3, 3, 3, v, m, None, v)),
            ("nh_mvn_draw", (v, m, 0, 1, 0, 4, x, 6, v)),
            ("nh_mvn_draw", (v, m, 33, 1, 0, 4, x, 40, v)),
            ("nh_mvn_draw", (v, m, 3, 1, 0, 0, x, 6, v)),
            ("nh_mvn_draw", (v, m, 3, 1, -1, 4, x, 6, v)),
            ("nh_mvn_draw", (v, m, 3, 1, 0, 4, x, 2, v)),      # d > ld
            ("nh_mvn_draw", (v, m, 3, 1, 0, 4, x, 6, None)),
            ("nh_bridge_l2", (v, v, 0, m, 3, v)),
            ("nh_bridge_l2", (v, v, 4, m, 0, v)),
            ("nh_bridge_sums", (v, 0, v, 4, 0.0, 0.5, 0.5, 1.0, v, None, None)),
            ("nh_bridge_sums", (v, 4, v, 0, 0.0, 0.5, 0.5, 1.0, v, None, None)),
            ("nh_bridge_sums", (v, 4, None, 4, 0.0, 0.5, 0.5, 1.0, v, None, None))):
        with pytest.raises(_lib.NaimaHipError):
            c.call(name, *args)
