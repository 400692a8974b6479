"""Is either electron spectrum a GOOD fit of an RX J1713-like X-ray + TeV spectrum?  The two
synchrotron + inverse-Compton fits of examples/rxj1713_compare.py -- an exponential cut-off power
law and a plain power law -- each checked against the data by itself: the posterior predictive
check of their stored spectra (naima_amd.predictive: replicated data, discrepancy statistics and
PIT are taken on the GPU).  LOO and WAIC say which model predicts better; the Bayesian p-values
here say whether a model could have produced the data at all (small = misfit).

    python examples/rxj1713_ppc.py [nwalkers] [nburn] [nrun]

Data: the synthetic table of BASELINE workload cfg3 (naima_amd/workloads.py), generated with a
cut-off: the power law should show a misfit, most clearly in the runs of its residuals' signs."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naima_amd as naima  # noqa: E402
from naima_amd import workloads as W  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u


def _compare():
    """the models of examples/rxj1713_compare.py"""
    spec = importlib.util.spec_from_file_location(
        "rxj1713_compare", os.path.join(ROOT, "examples", "rxj1713_compare.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(nwalkers=256, nburn=100, nrun=300, verbose=True, prefit=True, seed=0):
    cmp_ = _compare()
    p0 = cmp_.MODELS["ECPL"]["p0"]
    data = make_data(W.build_data(
        "cfg3", lambda E_eV: cmp_.ECPL(p0, {"energy": E_eV * u.eV}).to("1/(s cm2 eV)").value))
    results = {}
    for name, m in cmp_.MODELS.items():
        sampler, _ = naima.run_sampler(data_table=data, p0=m["p0"], labels=m["labels"],
                                       model=m["model"], prior=m["prior"], nwalkers=nwalkers,
                                       nburn=nburn, nrun=nrun, prefit=prefit, seed=1, verbose=False)
        r = results[name] = sampler.ppc(discard=nrun // 2, seed=seed)
        if verbose:
            pit = r["pit"][np.isfinite(r["pit"])]
            print("%-5s p_chi2 %.3f  p_max %.3f  p_runs %.3f | chi2_obs %.1f (replicates %.1f) for "
                  "%d points | PIT in [%.3f, %.3f]"
                  % (name, r["p_chi2"], r["p_max"], r["p_runs"], r["chi2_obs"]["median"],
                     r["chi2_rep"]["median"], r["n_points"], pit.min(), pit.max()))
    return results


if __name__ == "__main__":
    args = [int(v) for v in sys.argv[1:4]]
    main(*args)
