"""Time naima_amd.autocorr.integrated_time (the autocorrelation function on the GPU) against a
NumPy restatement of emcee 3's FFT estimator on the host, for AR(1) chains (phi = 0.5 .. 0.9 over
the dimensions).  Prints one JSON line per shape:

  device_s            integrated_time on the host chain, upload included (median of 3, warm)
  device_resident_s   the same with the chain already in device memory
  host_s              the NumPy restatement (one core); with --host-walkers W < n_w it is timed
                      on the first W walkers and scaled by n_w / W (the estimator is linear in
                      the walkers), and host_scaled says so
  tau_device, tau_host and their largest relative difference (on the walkers both saw)

    python scripts/autocorr_time.py [--host-walkers W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naima_amd import autocorr as A  # noqa: E402
from naima_amd.dview import as_chain  # noqa: E402

SHAPES = [(10000, 512, 6), (20000, 2048, 6)]


def ar1(rng, n_t, n_w, phis):
    phis = np.asarray(phis, dtype=float)
    x = np.empty((n_t, n_w, phis.size))
    x[0] = rng.standard_normal((n_w, phis.size))
    s = np.sqrt(1 - phis ** 2)
    for t in range(1, n_t):
        x[t] = phis * x[t - 1] + s * rng.standard_normal((n_w, phis.size))
    return x


def host_integrated_time(x, c=5):
    """emcee 3's integrated_time (FFT form) without the tolerance check"""
    n_t, n_w, n_d = x.shape
    n = 1 << max(0, int(n_t - 1).bit_length())
    tau = np.empty(n_d)
    for d in range(n_d):
        f = np.zeros(n_t)
        for k in range(n_w):
            y = x[:, k, d]
            g = np.fft.fft(y - np.mean(y), n=2 * n)
            acf = np.fft.ifft(g * np.conjugate(g))[:n_t].real
            f += acf / acf[0]
        f /= n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(n_t) < c * taus
        tau[d] = taus[np.argmin(m) if np.any(m) else n_t - 1]
    return tau


def median_time(fn, reps=3):
    fn()  # warm: code objects, pool buffers, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-walkers", type=int, default=512,
                    help="time the host estimator on at most this many walkers and scale")
    args = ap.parse_args()
    rng = np.random.default_rng(20261016)
    for n_t, n_w, n_d in SHAPES:
        x = ar1(rng, n_t, n_w, np.linspace(0.5, 0.9, n_d))
        dev_s = median_time(lambda: A.integrated_time(x, quiet=True))
        tau_dev = A.integrated_time(x, quiet=True)
        dx = as_chain(x)

        def resident():
            for d in range(n_d):
                A._dimension(dx, d, 5)
        res_s = median_time(resident)
        del dx
        hw = min(n_w, args.host_walkers)
        xh = np.ascontiguousarray(x[:, :hw])
        t0 = time.perf_counter()
        tau_host = host_integrated_time(xh)
        host_s = (time.perf_counter() - t0) * n_w / hw
        tau_dev_hw = A.integrated_time(xh, quiet=True)
        print(json.dumps({
            "shape": [n_t, n_w, n_d], "device_s": dev_s, "device_resident_s": res_s,
            "host_s": host_s, "host_scaled": hw < n_w, "host_walkers": hw,
            "speedup": host_s / dev_s, "tau_device": tau_dev.tolist(),
            "tau_host_on_host_walkers": tau_host.tolist(),
            "max_rel_diff_same_walkers": float(np.max(np.abs(tau_dev_hw / tau_host - 1))),
        }), flush=True)


if __name__ == "__main__":
    main()
