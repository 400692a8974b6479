"""Which electron spectrum does an RX J1713-like X-ray + TeV spectrum ask for?  Two synchrotron +
inverse-Compton fits of the same data table -- an exponential cut-off power law and a plain power
law -- compared by PSIS leave-one-out cross-validation and WAIC of their stored spectra
(naima_amd.infocrit: the pointwise log-likelihood matrix and its reductions stay on the GPU).

    python examples/rxj1713_compare.py [nwalkers] [nburn] [nrun]

Data: the synthetic table of BASELINE workload cfg3 (naima_amd/workloads.py), generated with a
cut-off: the power law should lose.  The runs are short; for a result to quote, run until the
autocorrelation time has converged (examples/rxj1713_converged.py) and pass reff = 1 / tau."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd import infocrit  # noqa: E402
from naima_amd import workloads as W  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u


def emission(electrons, B, data):
    IC = naima.InverseCompton(electrons, seed_photon_fields=["CMB", "FIR", "NIR"],
                              Eemin=100 * u.GeV)
    SYN = naima.Synchrotron(electrons, B=B * u.uG)
    return IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)


def ECPL(pars, data):
    e = naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                        10 ** pars[2] * u.TeV, beta=pars[4])
    return emission(e, pars[3], data)


def PL(pars, data):
    e = naima.PowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1])
    return emission(e, pars[2], data)


MODELS = {
    "ECPL": dict(model=ECPL, labels=["log10(norm)", "index", "log10(cutoff)", "B", "beta"],
                 p0=np.array(W.WORKLOADS["cfg3"]["p0"], dtype=float),
                 prior=lambda p: (naima.uniform_prior(p[1], -1, 5) + naima.uniform_prior(p[2], -3, 5)
                                  + naima.uniform_prior(p[3], 0, np.inf)
                                  + naima.uniform_prior(p[4], 0.1, 5))),
    "PL": dict(model=PL, labels=["log10(norm)", "index", "B"], p0=np.array([33.0, 3.0, 12.0]),
               prior=lambda p: naima.uniform_prior(p[1], -1, 5) + naima.uniform_prior(p[2], 0, np.inf)),
}


def main(nwalkers=256, nburn=100, nrun=300, verbose=True, prefit=True):
    p0 = MODELS["ECPL"]["p0"]
    data = make_data(W.build_data(
        "cfg3", lambda E_eV: ECPL(p0, {"energy": E_eV * u.eV}).to("1/(s cm2 eV)").value))
    results = {}
    for name, m in MODELS.items():
        sampler, _ = naima.run_sampler(data_table=data, p0=m["p0"], labels=m["labels"],
                                       model=m["model"], prior=m["prior"], nwalkers=nwalkers,
                                       nburn=nburn, nrun=nrun, prefit=prefit, seed=1, verbose=False)
        L = sampler.get_pointwise_log_likelihood(discard=nrun // 2)
        results[name] = dict(loo=infocrit.loo(L), waic=infocrit.waic(L))
        if verbose:
            lo, w = results[name]["loo"], results[name]["waic"]
            print("%-5s elpd_loo %9.2f +- %.2f  p_loo %6.2f  max pareto_k %.2f | elpd_waic %9.2f  "
                  "p_waic %6.2f" % (name, lo["elpd_loo"], lo["se"], lo["p_loo"],
                                    np.max(lo["pareto_k"]), w["elpd_waic"], w["p_waic"]))
    table = infocrit.compare([r["loo"] for r in results.values()], names=list(results))
    if verbose:
        print("%-5s %4s %10s %10s %8s" % ("model", "rank", "elpd_loo", "elpd_diff", "dse"))
        for r in table:
            print("%-5s %4d %10.2f %10.2f %8.2f" % (r["name"], r["rank"], r["elpd"], r["elpd_diff"],
                                                    r["dse"]))
    return table


if __name__ == "__main__":
    args = [int(v) for v in sys.argv[1:4]]
    main(*args)
