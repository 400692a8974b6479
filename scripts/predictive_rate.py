"""Time the three entry points of naima_amd.predictive (nh_ppc_rows, nh_ppc_counts,
nh_pit_columns) at a chain's size: M = n_w x n_t stored spectra at n_E data points.  Prints one
JSON line per shape; device times are medians of 3 warm calls that end in a download of a few
numbers (the replicates and the statistics stay in device memory), with the spectra already on
the device:

  replicate_s / _rows_per_s   posterior_predictive: M x n_E draws, then a stream synchronisation
  ppc_s / _rows_per_s         ppc: nh_ppc_rows (statistics only), nh_ppc_counts, the moments and
                              quantiles of T, nh_pit_columns
  pit_s / _rows_per_s         pit: nh_pit_columns alone
  bands_s                     predictive_quantiles of the replicates at 5 quantiles
  host_ppc_s                  the NumPy restatement (tests/predictive_np.py) of the rows, the
                              counts and the PIT on host_rows rows, scaled by M / host_rows when
                              it saw fewer (host_scaled says so)
  T_max_rel_diff              device against restatement on the rows the host saw

    python scripts/predictive_rate.py [--host-rows R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from naima_amd import predictive as PP  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402
from naima_amd.dview import as_matrix  # noqa: E402

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
    """a table of nE points with asymmetric errors and a few upper limits, and M spectra scattered
    5 % round it (in the data's unit)"""
    E = np.logspace(-1, 2, nE)
    flux = 1e-11 * E ** -2.3
    ul = np.zeros(nE, bool)
    ul[-3:] = True
    cols = dict(flux=flux, elo=0.1 * flux, ehi=0.25 * flux, ul=ul)
    data = make_data(dict(energy=E, energy_unit="TeV", flux=flux, flux_unit="1/(s cm2 TeV)",
                          flux_error_lo=cols["elo"], flux_error_hi=cols["ehi"], ul=ul, cl=0.9))
    x = flux * (1.0 + 0.05 * rng.standard_normal((M, nE)))
    return data, cols, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-rows", type=int, default=100000,
                    help="time the NumPy restatement on at most this many rows and scale")
    args = ap.parse_args()
    import predictive_np as R
    rng = np.random.default_rng(20261019)
    for n_w, n_t, nE in SHAPES:
        M = n_w * n_t
        data, cols, x = problem(rng, M, nE)
        unit = data["flux"].unit
        s = as_matrix(x)

        def replicate():
            y = PP.posterior_predictive(s, data, unit=unit, seed=1)
            y.ctx.sync()
            return y

        y = replicate()
        out = {"shape": [n_w, n_t, nE], "rows": M,
               "replicate_s": median_time(replicate),
               "ppc_s": median_time(lambda: PP.ppc(s, data, unit=unit, seed=1)),
               "pit_s": median_time(lambda: PP.pit(s, data, unit=unit)),
               "bands_s": median_time(lambda: PP.predictive_quantiles(
                   y, [0.025, 0.16, 0.5, 0.84, 0.975]))}
        for k in ("replicate", "ppc", "pit"):
            out[k + "_rows_per_s"] = M / out[k + "_s"]
        hr = min(M, args.host_rows)
        t0 = time.perf_counter()
        _, Th, _ = R.ppc_rows(x[:hr], 1.0, cols["flux"], cols["elo"], cols["ehi"], cols["ul"], 1)
        R.ppc_counts(Th)
        R.pit_columns(x[:hr], 1.0, cols["flux"], cols["elo"], cols["ehi"], cols["ul"])
        out.update({"host_rows": hr, "host_scaled": hr < M,
                    "host_ppc_s": (time.perf_counter() - t0) * M / hr})
        Td = PP.ppc(s, data, unit=unit, seed=1)["T"].get()[:hr]
        out["T_max_rel_diff"] = float(np.max(np.abs(Td / Th - 1)))
        out["speedup_ppc"] = out["host_ppc_s"] / out["ppc_s"]
        del s, y
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
