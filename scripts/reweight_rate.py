"""Time the entry points of naima_amd.reweight at a chain's size: M = n_w x n_t samples of ndim
parameters and n_E data points.  Prints one JSON line per shape; device times are medians of 3
warm calls that end in a small download, with the samples already on the device:

  drop_s        drop_points: K log-ratios from the pointwise matrix (nh_row_sums_select)
  weights_s     psis_weights of those K columns (nh_column_select + nh_psis_weights)
  stats_s       weighted_stats of the chain (nh_weighted_moments)
  quantiles_s   weighted_quantiles of the chain at 3 levels (nh_weighted_select: the radix sort)
  bands_s       weighted_quantiles of the n_E spectra columns at 4 levels
  resample_s    resample to round(ESS) rows (nh_resample_systematic + nh_gather_rows)
  host_weights_s  the NumPy restatement (tests/reweight_np.py) of the K weight columns on
                  host_rows rows, scaled by M / host_rows when it saw fewer
  lw_max_abs_diff device against restatement on the rows the host saw

    python scripts/reweight_rate.py [--host-rows R]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from naima_amd import reweight as RW  # noqa: E402
from naima_amd.dview import as_matrix  # noqa: E402

SHAPES = [(512, 500, 5, 40), (1024, 1500, 5, 40), (1024, 1500, 5, 130)]
K = 4  # groups of data points left out in turn


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
    ap.add_argument("--host-rows", type=int, default=100000,
                    help="time the NumPy restatement on at most this many rows and scale")
    args = ap.parse_args()
    import reweight_np as R
    rng = np.random.default_rng(20261020)
    warnings.simplefilter("ignore")
    for n_w, n_t, ndim, nE in SHAPES:
        M = n_w * n_t
        chain = as_matrix(rng.normal(size=(M, ndim)))
        L = as_matrix(-0.5 * rng.standard_normal((M, nE)) ** 2 * 0.2)
        spectra = as_matrix(np.exp(rng.normal(size=(M, nE))))
        groups = [list(range(g, nE, K)) for g in range(K)]
        lr = RW.drop_points(L, groups)
        w = RW.psis_weights(lr)
        out = {"shape": [n_w, n_t, ndim, nE], "rows": M, "targets": K, "tail_length": w.tail_length,
               "max_pareto_k": float(np.max(w.pareto_k)), "min_ess": float(np.min(w.ess)),
               "drop_s": median_time(lambda: RW.drop_points(L, groups).rows(0, 1).get()),
               "weights_s": median_time(lambda: RW.psis_weights(lr)),
               "stats_s": median_time(lambda: RW.weighted_stats(chain, w)),
               "quantiles_s": median_time(lambda: RW.weighted_quantiles(chain, w, [0.16, 0.5, 0.84])),
               "bands_s": median_time(lambda: RW.weighted_quantiles(spectra, w,
                                                                    [0.0013, 0.16, 0.84, 0.9987])),
               "resample_s": median_time(lambda: RW.resample(chain, w).rows(0, 1).get())}
        hr = min(M, args.host_rows)
        lrh = lr.get()[:hr]
        t0 = time.perf_counter()
        ref = R.psis_weights_np(lrh, R.tail_length(hr))
        out.update({"host_rows": hr, "host_scaled": hr < M,
                    "host_weights_s": (time.perf_counter() - t0) * M / hr})
        got = RW.psis_weights(lrh)
        out["lw_max_abs_diff"] = float(np.max(np.abs(got.lw.get() - ref["lw"])))
        out["speedup_weights"] = out["host_weights_s"] / out["weights_s"]
        del chain, L, spectra, lr, w
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
