"""Time naima_amd.evidence at a chain's size: n_t stored steps of n_w walkers in d parameters, a
correlated normal posterior whose evidence is known.  Prints one JSON line per shape; device times
are medians of 3 warm calls that end in a download, with the chain and its log-probabilities
already on the device:

  cov_s            posterior.covariance of the first half (nh_chain_cov: two passes)
  draw_s           nh_mvn_draw of N2 = N1 proposals, then a stream synchronisation
  logpdf_s         nh_mvn_logpdf of the second half (l1), then a stream synchronisation
  iteration_s      one nh_bridge_sums launch pair and its 16-byte download
  bridge_s         bridge_sampling as a whole with neff given: the above, the median of l1, the
                   log-probability function on the host (NumPy, not timed apart), the iterations,
                   the moments and the autocorrelation time of the error
  host_bridge_s    the NumPy restatement (tests/evidence_np.py) of the same call on one core
  logz_diff        device logz minus the restatement's; logz_minus_exact, logz_err

    python scripts/evidence_rate.py
"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from naima_amd import _lib  # noqa: E402
from naima_amd import evidence as V  # noqa: E402
from naima_amd import posterior as P  # noqa: E402

SHAPES = [(256, 400, 5), (512, 2000, 5), (512, 1000, 32)]


def median_time(fn, reps=3):
    fn()  # warm: code objects, pool buffers, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    import evidence_np as E
    rng = np.random.default_rng(20261019)
    ctx = _lib.get_context()
    for n_w, n_t, d in SHAPES:
        A = rng.normal(size=(d, d))
        cov = A @ A.T + d * np.eye(d)
        L, prec = np.linalg.cholesky(cov), np.linalg.inv(cov)
        mean = rng.normal(size=d)

        def fn(t):
            return -0.5 * np.einsum("ni,ij,nj->n", t - mean, prec, t - mean)

        exact = 0.5 * d * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(cov)[1]
        chain = mean + rng.normal(size=(n_t, n_w, d)) @ L.T  # (independent draws: tau = 1)
        lp = fn(chain.reshape(-1, d)).reshape(n_t, n_w)
        block = (ctx.array(chain.reshape(n_t, n_w * d)), n_t, n_w, d)
        dlp = ctx.array(lp)
        h, N1 = n_t // 2, (n_t - n_t // 2) * n_w
        m_d, L_d = ctx.array(mean), ctx.array(L)
        th, z2, l1 = ctx.empty((N1, d)), ctx.empty((N1,)), ctx.empty((N1,))
        sums = ctx.empty((2,))

        def draw():
            ctx.call("nh_mvn_draw", m_d, L_d, d, 1, 0, N1, th, d, z2)
            ctx.sync()

        def logpdf():
            ctx.call("nh_mvn_logpdf", block[0], h, n_t - h, n_w * d, d, n_w, d, m_d, L_d,
                     dlp.ptr + 8 * h * n_w, l1)
            ctx.sync()

        def iteration():
            ctx.call("nh_bridge_sums", l1, N1, z2, N1, 0.0, 0.5, 0.5, 1.0, sums, None, None)
            return sums.get()

        def bridge():
            return V.bridge_sampling(block, dlp, fn, seed=1, neff=float(N1), batch=N1)

        r = bridge()
        out = {"shape": [n_w, n_t, d], "n_post": N1,
               "cov_s": median_time(lambda: P.covariance((block[0], h, n_w, d))),
               "draw_s": median_time(draw), "logpdf_s": median_time(logpdf),
               "iteration_s": median_time(iteration), "bridge_s": median_time(bridge),
               "iterations": r["iterations"]}
        t0 = time.perf_counter()
        w = E.bridge_sampling(chain[:h].reshape(-1, d), chain[h:].reshape(-1, d),
                              lp[h:].ravel(), fn, seed=1)
        out.update({"host_bridge_s": time.perf_counter() - t0,
                    "logz_diff": r["logz"] - w["logz"], "logz_minus_exact": r["logz"] - exact,
                    "logz_err": r["logz_err"]})
        del block, dlp, th, z2, l1
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
