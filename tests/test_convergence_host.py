"""Running a fit until its autocorrelation time has converged, without a GPU: emcee's stopping
rule as a pure function, the argument errors of ``run_until_converged`` (raised before any device
work), the host-driven loop's books with the autocorrelation function taken in NumPy, and what
``run_sampler(converge=...)`` leaves in ``run_info``."""
import warnings

import numpy as np
import pytest

from naima_amd import autocorr
from naima_amd.autocorr import RunningAutocorr, converged
from naima_amd.sampler import EnsembleSampler, run_sampler

NW, ND = 32, 3


def gauss(x):
    return -0.5 * np.sum((x - 1.5) ** 2 / 0.25, axis=1)


def start():
    return np.random.default_rng(2).normal(size=(NW, ND))


def numpy_integrated_time(x, c=5, tol=50, quiet=False, has_walkers=True):
    """emcee's integrated_time in float64 NumPy (the FFT route of its function_1d); tol unused"""
    x = np.asarray(x, dtype=float)
    n_t, n_w, n_d = x.shape
    n = 1
    while n < n_t:
        n <<= 1
    tau = np.empty(n_d)
    for d in range(n_d):
        f = np.zeros(n_t)
        for w in range(n_w):
            y = x[:, w, d] - np.mean(x[:, w, d])
            ft = np.fft.fft(y, n=2 * n)
            acf = np.fft.ifft(ft * np.conjugate(ft))[:n_t].real
            f += acf / acf[0]
        taus = 2.0 * np.cumsum(f / n_w) - 1.0
        tau[d] = taus[autocorr.auto_window(taus, c)]
    return tau


# ------------------------------------------------------------------------------ the stopping rule
def test_rule_follows_the_tutorial():
    """converged = all(tau * tol < n) & all(|old_tau - tau| / tau < rtol), strict on both sides"""
    tau, old = np.array([10.0, 20.0]), np.array([10.05, 20.1])
    assert converged(tau, old, 1001, tol=50, rtol=0.01)
    assert not converged(tau, old, 1000, tol=50, rtol=0.01)      # 20 * 50 < 1000 is false
    assert not converged(tau, old, 999, tol=50, rtol=0.01)
    # the relative change is taken against the NEW tau, and must be strictly below rtol (numbers
    # that binary floating point holds exactly: 0.125 / 8 = 2**-6)
    r = 2.0 ** -6
    assert not converged(np.array([8.0]), np.array([8.125]), 10 ** 6, rtol=r)
    assert not converged(np.array([8.0]), np.array([7.875]), 10 ** 6, rtol=r)
    assert converged(np.array([8.0]), np.array([8.0625]), 10 ** 6, rtol=r)
    assert converged(np.array([8.0]), np.array([7.9375]), 10 ** 6, rtol=r)
    assert converged(np.array([8.125]), np.array([8.0]), 10 ** 6, rtol=r)  # 0.125 / 8.125 < 2**-6
    # every parameter has to pass both
    assert not converged(np.array([10.0, 30.0]), np.array([10.0, 30.0]), 1200, tol=50)
    assert not converged(np.array([10.0, 20.0]), np.array([10.0, 21.0]), 10 ** 6)


def test_rule_never_converges_on_the_first_check_or_on_nan():
    for rtol in (0.01, 0.5, 0.999, 1.0, 1e6):
        assert not converged(np.array([1.0, 2.0]), np.inf, 10 ** 9, tol=1, rtol=rtol)
    assert not converged(np.array([1.0, np.nan]), np.array([1.0, 1.0]), 10 ** 9, tol=1, rtol=1.0)
    assert not converged(np.array([1.0, 1.0]), np.array([1.0, np.nan]), 10 ** 9, tol=1, rtol=1.0)
    assert not converged(np.array([np.nan]), np.inf, 10 ** 9)


def test_rule_on_a_history():
    """a hand-made run checked every 100 rows: the first check that passes is the stop"""
    taus = [3.0, 6.0, 9.0, 9.5, 9.9, 9.95, 9.96]
    old, stops = np.inf, []
    for i, t in enumerate(taus):
        n = 100 * (i + 1)
        stops.append(converged(np.array([t]), old, n, tol=50, rtol=0.01))
        old = np.array([t])
    # 9.95 * 50 = 497.5 < 600 and |9.9 - 9.95| / 9.95 = 0.005 < 0.01; at 500 rows the change
    # 0.4 / 9.9 is still too large, and 9.9 * 50 = 495 < 500 alone is not enough
    assert stops == [False, False, False, False, False, True, True]


# ------------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("kw", [dict(max_steps=0), dict(max_steps=-5), dict(check_every=0),
                                dict(check_every=-1), dict(discard=50), dict(discard=60),
                                dict(discard=-1), dict(max_lag=1), dict(max_lag=0),
                                dict(thin_by=0)])
@pytest.mark.parametrize("device", [False, True])
def test_argument_errors_come_before_any_work(kw, device):
    calls = []

    def lnp(x, *a):
        calls.append(1)
        return gauss(x)

    s = EnsembleSampler(NW, ND, lnp, seed=5, device=device, naima_style=device)
    args = dict(max_steps=50)
    args.update(kw)
    with pytest.raises(ValueError):
        s.run_until_converged(start(), **args)
    assert not calls and s.steps_total == 0 and s._dev is None


def test_running_autocorr_argument_errors_need_no_gpu():
    for bad in (dict(max_lag=1), dict(max_lag=0), dict(n_w=0), dict(n_d=0)):
        kw = dict(n_w=4, n_d=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            RunningAutocorr(**kw)
    ra = RunningAutocorr(4, 2, max_lag=2)
    assert ra.rebuilds == 0 and ra.max_lag == 2
    with pytest.raises(ValueError):
        ra.tau()  # nothing has been given yet


def test_several_ranks_are_refused_before_any_step():
    class TwoRanks:
        rank, size = 0, 2

    calls = []

    def lnp(x):
        calls.append(1)
        return gauss(x)

    s = EnsembleSampler(NW, ND, lnp, seed=5, comm=TwoRanks())
    with pytest.raises(NotImplementedError):
        s.run_until_converged(start(), 50)
    assert not calls and s.steps_total == 0


# ------------------------------------------------------------------- the host-driven loop's books
@pytest.fixture
def numpy_tau(monkeypatch):
    monkeypatch.setattr(autocorr, "integrated_time", numpy_integrated_time)


def test_host_loop_stops_at_the_first_check_that_passes(numpy_tau):
    s = EnsembleSampler(NW, ND, gauss, seed=5)
    st = s.run_until_converged(start(), 600, check_every=50, tol=5, rtol=0.2)
    conv = s.convergence
    assert conv["where"] == "host" and conv["rebuilds"] == 0
    rows = [r for r, _ in conv["history"]]
    assert rows == list(range(50, conv["rows"] + 1, 50)) and s.iteration == conv["rows"]
    chain = s.get_chain()
    assert chain.shape == (conv["rows"], NW, ND) and np.array_equal(chain[-1], st.coords)
    # the history is tau of the final chain's prefixes, and the stop is the rule's first pass
    old, stop = np.inf, 600
    for r, tau in conv["history"]:
        ref = numpy_integrated_time(chain[:r])
        assert np.array_equal(tau, ref)
        if converged(ref, old, r, 5, 0.2):
            stop = r
            break
        old = ref
    assert conv["rows"] == stop < 600
    assert conv["converged"]  # (a Gaussian with 32 walkers: tau of a few steps)
    # the same seed, run plainly: the same chain
    f = EnsembleSampler(NW, ND, gauss, seed=5)
    f.run_mcmc(start(), stop)
    assert np.array_equal(f.get_chain(), chain)
    assert np.array_equal(f.acceptance_fraction, s.acceptance_fraction)


def test_host_loop_with_discard_thinning_and_a_last_short_group(numpy_tau):
    s = EnsembleSampler(NW, ND, gauss, seed=7)
    s.run_mcmc(start(), 3)  # rows of an earlier call are not part of the monitored chain
    st = s.run_until_converged(start(), 70, check_every=30, tol=10 ** 6, discard=40, thin_by=2)
    conv = s.convergence
    assert not conv["converged"] and conv["rows"] == 70
    assert [r for r, _ in conv["history"]] == [60, 70]  # (30 rows lie inside the discard)
    assert s.iteration == 73 and s.steps_total == 3 + 140
    chain = s.get_chain()
    assert np.array_equal(conv["tau"], numpy_integrated_time(chain[3 + 40:]))
    assert np.array_equal(conv["history"][0][1], numpy_integrated_time(chain[3 + 40:3 + 60]))


def test_a_nan_tau_warns_once_and_never_converges(monkeypatch):
    monkeypatch.setattr(autocorr, "integrated_time",
                        lambda x, **kw: np.array([1.0, np.nan, 1.0]))
    s = EnsembleSampler(NW, ND, gauss, seed=5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s.run_until_converged(start(), 40, check_every=10, tol=1, rtol=10.0)
    assert len([x for x in w if "NaN" in str(x.message)]) == 1
    assert not s.convergence["converged"] and s.convergence["rows"] == 40
    assert len(s.convergence["history"]) == 4


# ----------------------------------------------------------------------------------- run_sampler
def test_run_info_keys_only_with_converge_and_they_survive_save_and_read(numpy_tau, tmp_path, capsys):
    import naima_amd as na
    from naima_amd.datatable import make_data
    plain = EnsembleSampler(NW, ND, gauss, seed=4)
    plain.run_info = {}
    run_sampler(20, sampler=plain, pos=start(), verbose=False)
    assert "converged" not in plain.run_info and "autocorr_time" not in plain.run_info
    assert plain.iteration == 20

    s = EnsembleSampler(NW, ND, gauss, seed=4)
    s.labels = ["norm", "index", "cutoff"]
    s.run_info = {"n_walkers": NW, "n_burn": 0}
    s, pos = run_sampler(600, sampler=s, pos=start(), verbose=True,
                         converge=dict(check_every=50, tol=5, rtol=0.2))
    assert "Converged after %d of at most 600 steps" % s.iteration in capsys.readouterr().out
    assert s.run_info["converged"] is True and s.run_info["n_run"] == 600
    assert s.run_info["autocorr_time"] == [float(t) for t in s.convergence["tau"]]
    assert s.iteration == s.convergence["rows"] < 600
    assert np.array_equal(pos.coords, s.get_chain()[-1])
    # converge=True: the defaults (tol = 50 does not pass within 60 rows)
    s2 = EnsembleSampler(NW, ND, gauss, seed=4)
    s2.run_info = {}
    run_sampler(60, sampler=s2, pos=start(), verbose=False, converge=True)
    assert s2.run_info["converged"] is False and len(s2.run_info["autocorr_time"]) == ND
    assert s2.iteration == 60 and [r for r, _ in s2.convergence["history"]] == [60]

    k = 5
    s.data = make_data(dict(energy=np.geomspace(1, 10, k), energy_unit="TeV",
                            flux=np.ones(k), flux_error_lo=0.1 * np.ones(k),
                            flux_error_hi=0.1 * np.ones(k), ul=np.zeros(k, bool), cl=0.9,
                            flux_unit="1/(cm2 s TeV)"))
    r = na.read_run(na.save_run(str(tmp_path / "run"), s))
    assert bool(r.run_info["converged"]) is True
    assert np.array_equal(np.asarray(r.run_info["autocorr_time"], dtype=float),
                          s.run_info["autocorr_time"])
    assert np.array_equal(r.get_chain(), s.get_chain())
    table = na.save_results_table(str(tmp_path / "run"), s, include_blobs=False)
    assert table["meta"]["converged"] is True
    assert table["meta"]["autocorr_time"] == s.run_info["autocorr_time"]
    text = open(str(tmp_path / "run_results.ecsv")).read()
    assert "converged: true" in text and "autocorr_time:" in text
