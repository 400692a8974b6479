"""Time the three entry points of naima_amd.infocrit (nh_pointwise_lnl, nh_lnl_column_stats,
nh_psis_columns) at a chain's size: M = n_w x n_t stored spectra at n_E data points.  Prints one
JSON line per shape; device times are medians of 3 warm calls that end in a download of n_E
numbers (the pointwise matrix itself stays in device memory), with the spectra already on the
device:

  pointwise_s / _rows_per_s   pointwise_log_likelihood: M x n_E terms, the non-finite count back
  waic_s / _rows_per_s        waic: nh_lnl_column_stats
  loo_s / _rows_per_s         loo: nh_lnl_column_stats + nh_column_select + nh_psis_columns
  psis_s                      loo_s - waic_s - the selection alone
  host_loo_s                  the NumPy restatement's loo (tests/infocrit_np.py: a Python loop over
                              the data points, each sorting M values) on host_rows rows, scaled by
                              M / host_rows when it saw fewer (host_scaled says so; the sort makes
                              the scaling optimistic for the host)
  loo_max_rel_diff            device against restatement on the rows the host saw

    python scripts/infocrit_rate.py [--host-rows R]
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
from naima_amd import infocrit as IC  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402
from naima_amd.dview import as_matrix  # noqa: E402
from naima_amd.plot import column_select  # noqa: E402

SHAPES = [(512, 500, 40), (1024, 1500, 40), (1024, 1500, 130)]


def median_time(fn, reps=3):
    fn()  # warm: code objects, pool buffers, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def problem(rng, M, nE):
    """a table of nE points with 10 % errors and a few upper limits, and M spectra scattered 5 %
    round it (in the data's unit)"""
    E = np.logspace(-1, 2, nE)
    flux = 1e-11 * E ** -2.3
    ul = np.zeros(nE, bool)
    ul[-3:] = True
    data = make_data(dict(energy=E, energy_unit="TeV", flux=flux, flux_unit="1/(s cm2 TeV)",
                          flux_error_lo=0.1 * flux, flux_error_hi=0.12 * flux, ul=ul, cl=0.9))
    x = flux * (1.0 + 0.05 * rng.standard_normal((M, nE)))
    return data, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-rows", type=int, default=100000,
                    help="time the NumPy restatement on at most this many rows and scale")
    args = ap.parse_args()
    import infocrit_np as R
    rng = np.random.default_rng(20261019)
    warnings.simplefilter("ignore")
    for n_w, n_t, nE in SHAPES:
        M = n_w * n_t
        data, x = problem(rng, M, nE)
        unit = data["flux"].unit
        s = as_matrix(x)
        L = IC.pointwise_log_likelihood(s, data, unit=unit)
        Mt = IC.tail_length(M)
        out = {"shape": [n_w, n_t, nE], "rows": M, "tail_length": Mt,
               "pointwise_s": median_time(lambda: IC.pointwise_log_likelihood(s, data, unit=unit)),
               "waic_s": median_time(lambda: IC.waic(L)),
               "loo_s": median_time(lambda: IC.loo(L)),
               "select_s": median_time(lambda: column_select(L, [Mt]))}
        out["psis_s"] = out["loo_s"] - out["waic_s"] - out["select_s"]
        for k in ("pointwise", "waic", "loo"):
            out[k + "_rows_per_s"] = M / out[k + "_s"]
        hr = min(M, args.host_rows)
        Lh = L.get()[:hr]
        t0 = time.perf_counter()
        ref = R.loo(Lh)
        out.update({"host_rows": hr, "host_scaled": hr < M,
                    "host_loo_s": (time.perf_counter() - t0) * M / hr})
        got = IC.loo(Lh)
        out["loo_max_rel_diff"] = float(np.max(np.abs(got["elpd_loo_i"] / ref["elpd_loo_i"] - 1)))
        out["speedup_loo"] = out["host_loo_s"] / out["loo_s"]
        del s, L
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
