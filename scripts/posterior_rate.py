"""Time the posterior reductions of naima_amd.posterior (nh_column_moments, nh_hist_columns,
nh_kde_columns) and the data pass of a whole corner figure against NumPy and scipy on one host
core, for flat chains of n_w x n_t rows and n_d columns of different scale.  Prints one JSON line
per shape; device times are medians of 3 warm calls that end in a download, with the chain already
in device memory unless the name says ``upload``:

  moments_s            column_stats
  hist1d_s             histogram, 20 bins (column_stats for the range included)
  hist2d_s             histogram_pairs, every i < j at 20 bins (the same)
  kde_s                gaussian_kde at 101 points per column (column_stats included)
  corner_s             what corner() computes: the 1-D and pair histograms in one pass and the
                       three quantiles by nh_column_select
  corner_upload_s      the same from the host chain, upload included
  host_hist1d_s        np.histogram per column
  host_hist2d_s        np.histogram2d per pair
  host_kde_s           scipy.stats.gaussian_kde per column at the same points
  host_corner_s        host_hist1d_s + host_hist2d_s + np.percentile per column
  host_rows            rows the host functions were timed on; with fewer than the chain has their
                       times are scaled by M / host_rows (all of them are linear in the rows) and
                       host_scaled says so

    python scripts/posterior_rate.py [--host-rows R] [--kde-host-rows R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naima_amd import posterior as P  # noqa: E402
from naima_amd.dview import as_matrix  # noqa: E402

SHAPES = [(512, 10000, 6), (2048, 20000, 6)]
BINS, G, Q = 20, 101, (0.16, 0.5, 0.84)


def chain(rng, M, n_d):
    """correlated columns of different scale, each within a few sigma of zero (scipy scales data
    and points by the bandwidth before it subtracts them: far from zero its own rounding shows)"""
    z = rng.standard_normal((M, n_d))
    z[:, 1:] += 0.6 * z[:, :-1]
    return (z + np.linspace(-3.0, 3.0, n_d)) * np.logspace(-3, 2, n_d)


def median_time(fn, reps=3):
    fn()  # warm: code objects, pool buffers, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-rows", type=int, default=4000000,
                    help="time the host histograms on at most this many rows and scale")
    ap.add_argument("--kde-host-rows", type=int, default=200000,
                    help="time scipy's KDE on at most this many rows and scale")
    args = ap.parse_args()
    rng = np.random.default_rng(20261017)
    from scipy import stats
    for n_w, n_t, n_d in SHAPES:
        M = n_w * n_t
        x = chain(rng, M, n_d)
        pairs = [(i, j) for i in range(n_d) for j in range(i + 1, n_d)]
        s = as_matrix(x)
        st = P.column_stats(s)
        pts = st["mean"][:, None] + np.sqrt(st["var"])[:, None] * np.linspace(-4, 4, G)

        def corner_data(m):
            return P._histograms(m, BINS, None, pairs), P._quantiles(m, Q)

        out = {"shape": [n_w, n_t, n_d], "rows": M,
               "moments_s": median_time(lambda: P.column_stats(s)),
               "hist1d_s": median_time(lambda: P.histogram(s, BINS)),
               "hist2d_s": median_time(lambda: P.histogram_pairs(s, BINS)),
               "kde_s": median_time(lambda: P.gaussian_kde(s, pts)),
               "corner_s": median_time(lambda: corner_data(s)),
               "corner_upload_s": median_time(lambda: corner_data(as_matrix(x)))}
        (h1, H, edges), q = corner_data(s)
        kde = P.gaussian_kde(s, pts)
        del s

        hr, kr = min(M, args.host_rows), min(M, args.kde_host_rows)
        xh = x[:hr]
        t1, ref1 = timed(lambda: [np.histogram(xh[:, c], bins=BINS, range=(edges[c][0], edges[c][-1]))[0]
                                  for c in range(n_d)])
        t2, ref2 = timed(lambda: [np.histogram2d(xh[:, i], xh[:, j], bins=[edges[i], edges[j]])[0]
                                  for i, j in pairs])
        tq, refq = timed(lambda: np.percentile(xh, [100 * v for v in Q], axis=0))
        xk = x[:kr]
        tk, refk = timed(lambda: [stats.gaussian_kde(xk[:, c])(pts[c]) for c in range(n_d)])
        out.update({
            "host_rows": hr, "kde_host_rows": kr, "host_scaled": hr < M or kr < M,
            "host_hist1d_s": t1 * M / hr, "host_hist2d_s": t2 * M / hr,
            "host_kde_s": tk * M / kr, "host_corner_s": (t1 + t2 + tq) * M / hr})
        # the device's results on the rows the host saw
        sh = as_matrix(xh)
        g1, gH, _ = P._histograms(sh, BINS, list(zip(edges[:, 0], edges[:, -1])), pairs)
        out["hist1d_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(g1, ref1)))
        out["hist2d_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(gH, ref2)))
        out["quantile_max_rel_diff"] = float(np.max(np.abs(P._quantiles(sh, Q) / refq - 1)))
        gk = P.gaussian_kde(as_matrix(xk), pts)
        out["kde_max_rel_diff"] = float(np.max(np.abs(gk / np.array(refk) - 1)))
        out["speedup_hist1d"] = out["host_hist1d_s"] / out["hist1d_s"]
        out["speedup_hist2d"] = out["host_hist2d_s"] / out["hist2d_s"]
        out["speedup_kde"] = out["host_kde_s"] / out["kde_s"]
        out["speedup_corner_upload"] = out["host_corner_s"] / out["corner_upload_s"]
        del h1, H, q, kde
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
