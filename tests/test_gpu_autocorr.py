"""The integrated autocorrelation time on the GPU (naima_amd.autocorr, nh_autocorr_prep /
nh_autocorr_lags) against the NumPy restatement of emcee 3's estimator in test_autocorr_host.py:
the autocorrelation function, the windows and the times at many shapes, windows past the first
block of lags, AR(1) known answers, the tolerance check, NaN semantics, determinism,
EnsembleSampler.get_autocorr_time on device and host-driven runs, and the line of plot_chain."""
import logging
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_autocorr_host import PHIS, ar1, exact_tau, ref_function_1d, ref_integrated  # noqa: E402

pytestmark = pytest.mark.gpu

F_ATOL = 1e-11
TAU_RTOL = 1e-9


def check_parity(x3, c=5, has_walkers=True, x=None, tau_atol=0.0):
    """the device's f, windows and taus against the restatement's on the chain x3 (n_t, n_w, n_d);
    ``x`` is what integrated_time is given (x3 by default)"""
    from naima_amd import autocorr as A
    x = x3 if x is None else x
    tau, win, fs, n_t = A._integrated(x, c, has_walkers)
    rtau, rwin, rfs, margin = ref_integrated(x3, c)
    fin = np.isfinite(rtau)
    if c > 0:
        assert np.all(margin[fin] > 1e-6), margin  # (the window is not a near-tie)
    np.testing.assert_array_equal(win, rwin)
    np.testing.assert_allclose(tau, rtau, rtol=TAU_RTOL, atol=tau_atol)
    for d in np.flatnonzero(fin):
        f = fs[d]
        assert 1 <= f.size <= n_t and f.size > win[d]
        np.testing.assert_allclose(f, rfs[d][:f.size], rtol=0, atol=F_ATOL)
    np.testing.assert_array_equal(A.integrated_time(x, c=c, tol=0, has_walkers=has_walkers), tau)
    return tau


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 1), (50, 4, 3), (1000, 32, 5), (4097, 7, 2),
                                   (10000, 256, 6)])
def test_parity_with_the_restatement(shape):
    n_t, n_w, n_d = shape
    rng = np.random.default_rng(n_t * 31 + n_w * 7 + n_d)
    phis = np.linspace(0.0, 0.9, n_d)
    check_parity(ar1(rng, n_t, n_w, phis))


def test_parity_of_1d_and_2d_input():
    rng = np.random.default_rng(4)
    x = ar1(rng, 3000, 8, [0.7, 0.3])
    one = x[:, 0, 0]
    check_parity(one[:, None, None], x=one)
    two = x[:, :, 0]
    check_parity(two[:, :, None], x=two, has_walkers=True)
    check_parity(two[:, None, :], x=two, has_walkers=False)


def test_function_1d_is_emcee_s():
    from naima_amd import autocorr as A
    rng = np.random.default_rng(6)
    for n in (1, 2, 3, 255, 256, 257, 5000):
        x = ar1(rng, n, 1, [0.6])[:, 0, 0] + 3.0
        got, want = A.function_1d(x), ref_function_1d(x)
        assert got.shape == (n,)
        if n == 1:
            assert np.all(np.isnan(got)) and np.all(np.isnan(want))
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=F_ATOL)
    assert np.all(np.isnan(A.function_1d(np.full(10, 2.0))))


def test_windows_past_the_first_block_of_lags():
    rng = np.random.default_rng(8)
    x = ar1(rng, 3000, 8, [0.99, 0.995])
    tau = check_parity(x)
    from naima_amd import autocorr as A
    _, win, fs, _ = A._integrated(x)
    assert np.all(win > 500), win
    # c = 0: no lag satisfies m < c*tau, the window is the last lag -- every lag is computed.
    # (2 sum(f) - 1 over every lag of a centred series cancels to ~0: compared absolutely)
    tau0 = check_parity(x[:, :, :1], c=0, tau_atol=1e-8)
    _, win0, fs0, _ = A._integrated(x[:, :, :1], c=0)
    assert win0[0] == 2999 and fs0[0].size == 3000
    assert np.isfinite(tau).all() and np.isfinite(tau0).all()


def test_ar1_known_answers():
    from naima_amd import autocorr as A
    x = ar1(np.random.default_rng(11), 20000, 64, PHIS)
    tau = A.integrated_time(x)
    for d, phi in enumerate(PHIS):
        assert abs(tau[d] / exact_tau(phi) - 1) < 0.05, (phi, tau[d])


def test_short_chain_raises_and_quiet_logs(caplog):
    from naima_amd import autocorr as A
    x = ar1(np.random.default_rng(2), 200, 16, [0.9, 0.2])
    with pytest.raises(A.AutocorrError) as err:
        A.integrated_time(x)
    msg = str(err.value)
    assert msg.startswith("The chain is shorter than 50 times the integrated autocorrelation time "
                          "for 1 parameter(s). Use this estimate with caution and run a longer "
                          "chain!\nN/50 = 4;\ntau: ")
    with caplog.at_level(logging.WARNING, logger="naima_amd.autocorr"):
        tau = A.integrated_time(x, quiet=True)
    np.testing.assert_array_equal(err.value.tau, tau)
    assert [r.getMessage() for r in caplog.records if r.name == "naima_amd.autocorr"] == [msg]
    np.testing.assert_array_equal(A.integrated_time(x, tol=0), tau)
    np.testing.assert_array_equal(A.integrated_time(x[:3], tol=0),
                                  A.integrated_time(x[:3], quiet=True))


def test_nan_semantics():
    from naima_amd import autocorr as A
    x = ar1(np.random.default_rng(3), 2000, 8, [0.5, 0.6, 0.7])
    base = A.integrated_time(x, tol=0)
    assert np.isfinite(base).all()
    y = x.copy()
    y[:, 3, 1] = 2.5  # one constant walker
    got = A.integrated_time(y, tol=0)
    assert np.isnan(got[1])
    np.testing.assert_array_equal(got[[0, 2]], base[[0, 2]])
    y = x.copy()
    y[700, 5, 2] = np.inf
    got = A.integrated_time(y, tol=0)
    assert np.isnan(got[2])
    np.testing.assert_array_equal(got[:2], base[:2])
    y[9, 0, 0] = np.nan
    assert np.isnan(A.integrated_time(y, tol=0)[0])
    assert np.isnan(A.integrated_time(x[:1], tol=0)).all()  # n_t = 1: zero variance


def test_repeated_calls_are_bit_identical():
    from naima_amd import autocorr as A
    x = ar1(np.random.default_rng(12), 6000, 96, [0.95, 0.1, 0.5])
    a = A._integrated(x)
    b = A._integrated(x)
    np.testing.assert_array_equal(a[0], b[0])
    for fa, fb in zip(a[2], b[2]):
        np.testing.assert_array_equal(fa, fb)


def expect_sampler_tau(s, discard, thin):
    """get_autocorr_time(discard, thin) == thin * the restatement on get_chain(discard, thin)"""
    got = s.get_autocorr_time(discard=discard, thin=thin, quiet=True)
    chain = s.get_chain(discard=discard, thin=thin)
    rtau, _, _, margin = ref_integrated(chain)
    assert np.all(np.isfinite(rtau)) and np.all(margin > 1e-6)
    np.testing.assert_allclose(got, thin * rtau, rtol=TAU_RTOL, atol=0)
    return got


def test_device_run_get_autocorr_time():
    import naima_amd as na
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    nw = 64
    s = EnsembleSampler(nw, p0.size, na.lnprob, args=[data, model, prior], seed=5,
                        naima_style=True, device=True)
    start = p0 * (1 + 0.01 * np.random.default_rng(1).standard_normal((nw, p0.size)))
    s.run_mcmc(start, 300)
    assert s._dev is not None
    expect_sampler_tau(s, 100, 2)
    expect_sampler_tau(s, 0, 1)


def gauss(x):
    return -0.5 * np.sum((x - 1.5) ** 2 / 0.25, axis=1)


@pytest.fixture(scope="module")
def host_run():
    """a host-driven run (a plain-NumPy log-probability) long enough for tol=50"""
    from naima_amd.sampler import EnsembleSampler
    s = EnsembleSampler(32, 3, gauss, seed=7)
    s.run_mcmc(np.random.default_rng(0).normal(size=(32, 3)), 6000)
    s.labels = ["a", "b", "c"]
    return s


def test_host_driven_run_get_autocorr_time(host_run):
    s = host_run
    assert s._dev is None
    expect_sampler_tau(s, 500, 3)
    tau = s.get_autocorr_time(discard=500)  # long enough: no error
    assert np.all(np.isfinite(tau))
    np.testing.assert_array_equal(tau, s.get_autocorr_time(discard=500, quiet=True))


class ChainStub:
    def __init__(self, chain):
        self._chain = chain
        self.labels = ["p%d" % i for i in range(chain.shape[2])]
        self.acceptance_fraction = np.full(chain.shape[1], 0.4)

    def get_chain(self, flat=False):
        return self._chain.reshape(-1, self._chain.shape[-1]) if flat else self._chain


def figure_text(fig):
    return "\n".join(t.get_text() for t in fig.texts)


def test_plot_chain_prints_the_autocorrelation_time(host_run, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from naima_amd import autocorr as A
    from naima_amd import plot as P
    from naima_amd.analysis import read_run, save_run
    x = ar1(np.random.default_rng(5), 4000, 16, [0.5, 0.8])
    tau = A.integrated_time(x)
    s = ChainStub(x)
    for p in (0, 1):
        text = figure_text(P.plot_chain(s, p))
        line = "Autocorrelation time: %.1f" % tau[p]
        assert line in text
        assert text.index("Steps in chain") < text.index(line) < text.index("Mean acceptance")
    short = figure_text(P.plot_chain(ChainStub(x[:10]), 0))
    assert "Autocorrelation" not in short and "Steps in chain: 10" in short
    # a saved run read back gets the line of the live sampler
    h = host_run
    want = "Autocorrelation time: %.1f" % A.integrated_time(h.get_chain())[1]
    assert want in figure_text(P.plot_chain(h, 1))
    r = read_run(save_run(str(tmp_path / "run.npz"), h))
    assert want in figure_text(P.plot_chain(r, 1))
    plt.close("all")
