"""naima_amd.autocorr on the host: the import creates no GPU context, AutocorrError, the argument
errors that come before any device work, and the NumPy restatement of emcee 3's estimator (the
yardstick of test_gpu_autocorr.py) against the known answers of AR(1) series."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- emcee 3's emcee/autocorr.py (FFT form), restated in NumPy -------------------------------
def ref_function_1d(x):
    n = 1 << max(0, int(len(x) - 1).bit_length())  # next_pow_two
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.fft.fft(x - np.mean(x), n=2 * n)
        acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
        return acf / acf[0]


def ref_auto_window(taus, c):
    m = np.arange(len(taus)) < c * taus
    return np.argmin(m) if np.any(m) else len(taus) - 1


def ref_integrated(x, c=5):
    """(tau [n_d], windows [n_d], f [n_d][n_t], margin [n_d]) of a chain (n_t, n_w, n_d); margin
    is min |m - c * taus[m]| over the lags up to the window: how far the window is from a tie"""
    n_t, n_w, n_d = x.shape
    tau, win, fs, margin = np.empty(n_d), np.empty(n_d, int), [], np.empty(n_d)
    for d in range(n_d):
        f = sum(ref_function_1d(x[:, k, d]) for k in range(n_w)) / n_w
        with np.errstate(invalid="ignore"):
            taus = 2.0 * np.cumsum(f) - 1.0
            win[d] = ref_auto_window(taus, c)
            m = np.arange(win[d] + 1)
            margin[d] = np.min(np.abs(m - c * taus[: win[d] + 1]))
        tau[d] = taus[win[d]]
        fs.append(f)
    return tau, win, fs, margin


def ar1(rng, n_t, n_w, phis):
    """AR(1) series of unit variance, one coefficient per dimension: (n_t, n_w, len(phis))"""
    phis = np.asarray(phis, dtype=float)
    e = rng.standard_normal((n_t, n_w, phis.size))
    x = np.empty_like(e)
    x[0] = e[0]
    s = np.sqrt(1 - phis ** 2)
    for t in range(1, n_t):
        x[t] = phis * x[t - 1] + s * e[t]
    return x


# (1+phi)/(1-phi): the integrated autocorrelation time of an AR(1) process
PHIS = (0.0, 0.5, 0.8, 0.9)


def exact_tau(phi):
    return (1 + phi) / (1 - phi)


def test_import_creates_no_gpu_context():
    code = ("import naima_amd.autocorr as A, naima_amd._lib as L; "
            "assert L._lib is None and not L._default, 'GPU touched'; "
            "assert A.AutocorrError and A.integrated_time; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_autocorr_error_carries_tau():
    from naima_amd.autocorr import AutocorrError
    tau = np.array([1.5, 2.5])
    e = AutocorrError(tau, "too short")
    assert e.tau is tau and str(e) == "too short"
    assert isinstance(e, Exception)


def test_bad_shapes_raise_before_device_work(monkeypatch):
    from naima_amd import _lib
    from naima_amd import autocorr as A

    def no_device(*a, **k):
        raise AssertionError("a GPU context was asked for")

    monkeypatch.setattr(_lib, "get_context", no_device)
    with pytest.raises(ValueError, match="invalid dimensions"):
        A.integrated_time(np.zeros((3, 2, 2, 2)))
    with pytest.raises(ValueError):
        A.integrated_time(np.zeros((0, 4, 2)))
    with pytest.raises(ValueError, match="invalid dimensions"):
        A.function_1d(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        A.function_1d(np.zeros(0))
    with pytest.raises(ValueError, match="invalid dimensions"):
        A.integrated_time(np.zeros((3, 2, 2, 2)), quiet=True)


def test_auto_window_is_emcee_s():
    from naima_amd.autocorr import auto_window
    taus = np.array([1.0, 1.8, 2.2, 0.5, 0.4])
    assert auto_window(taus, 5) == 3 and ref_auto_window(taus, 5) == 3
    assert auto_window(taus, 0) == 4  # no lag with m < 0: the last one
    assert auto_window(np.array([1.0, 2.0, 3.0]), 5) == 0  # every lag inside: argmin of all True


def test_restatement_meets_ar1_known_answers():
    x = ar1(np.random.default_rng(11), 20000, 64, PHIS)
    tau, win, fs, margin = ref_integrated(x)
    for d, phi in enumerate(PHIS):
        assert abs(tau[d] / exact_tau(phi) - 1) < 0.05, (phi, tau[d])
    assert np.all(margin > 1e-6)
