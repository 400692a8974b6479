"""Which electron spectrum do the data prefer, by the evidence?  The two synchrotron +
inverse-Compton fits of examples/rxj1713_compare.py -- an exponential cut-off power law and a plain
power law -- with a BOUNDED uniform prior on every parameter, their marginal likelihoods by bridge
sampling (naima_amd.evidence: covariance, proposal draws and the iteration's sums on the GPU) and
the log Bayes factor between them.

    python examples/rxj1713_evidence.py [nwalkers] [nburn] [nrun]

naima's ``uniform_prior`` returns 0 inside its interval, so the volume of each model's prior box
is passed as ``log_prior_norm`` = sum log(umax - umin); without it (or with an unbounded prior, as
in rxj1713_compare.py) the numbers would mean nothing.  The likelihood's constant of the data table
cancels in the Bayes factor.  Mind that an evidence depends on the prior ranges: widening the box
of a parameter the simpler model does not have lowers the richer model's evidence (Occam's
factor), which WAIC and PSIS-LOO of rxj1713_compare.py do not see.

Data: the synthetic table of BASELINE workload cfg3 (naima_amd/workloads.py), generated with a
cut-off: the power law should lose.  The runs are short; for a result to quote, run until the
autocorrelation time has converged (examples/rxj1713_converged.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd import evidence  # noqa: E402
from naima_amd import workloads as W  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rxj1713_compare import ECPL, PL  # noqa: E402

u = naima.u

# (label, lower bound, upper bound) of every parameter.  Every walker must START inside the box: one
# that starts outside keeps lnprob = -inf until a move brings it in, and bridge_sampling refuses a
# chain with such rows.  Without a prefit the initial ball is 10 % of p0 (+-3.3 in log10(norm)).
BOUNDS = {
    "ECPL": [("log10(norm)", 13.0, 53.0), ("index", -1.0, 5.0), ("log10(cutoff)", -3.0, 5.0),
             ("B", 0.0, 100.0), ("beta", 0.1, 5.0)],
    "PL": [("log10(norm)", 13.0, 53.0), ("index", -1.0, 5.0), ("B", 0.0, 100.0)],
}
MODELS = {"ECPL": dict(model=ECPL, p0=np.array(W.WORKLOADS["cfg3"]["p0"], dtype=float)),
          "PL": dict(model=PL, p0=np.array([33.0, 3.0, 12.0]))}


def box_prior(bounds):
    def prior(p):
        out = naima.uniform_prior(p[0], bounds[0][1], bounds[0][2])
        for i, (_, lo, hi) in enumerate(bounds[1:], 1):
            out = out + naima.uniform_prior(p[i], lo, hi)
        return out
    return prior


def log_volume(bounds):
    return float(sum(np.log(hi - lo) for _, lo, hi in bounds))


def make_data_table():
    p0 = MODELS["ECPL"]["p0"]
    return make_data(W.build_data(
        "cfg3", lambda E_eV: ECPL(p0, {"energy": E_eV * u.eV}).to("1/(s cm2 eV)").value))


def fit(name, data, nwalkers=256, nburn=100, nrun=300, prefit=True, converge=None):
    """the sampler of model ``name`` after its run.  ``converge`` is run_sampler's: a monitored
    run keeps its chain in one history block in HBM, where ``log_evidence`` then reads it; after
    a plain run the chain is uploaded once instead -- the numbers are the same."""
    b, m = BOUNDS[name], MODELS[name]
    sampler, _ = naima.run_sampler(data_table=data, p0=m["p0"], labels=[v[0] for v in b],
                                   model=m["model"], prior=box_prior(b), nwalkers=nwalkers,
                                   nburn=nburn, nrun=nrun, prefit=prefit, seed=1, verbose=False,
                                   converge=converge)
    return sampler


def main(nwalkers=256, nburn=100, nrun=300, verbose=True, prefit=True):
    data = make_data_table()
    results = {}
    for name in MODELS:
        sampler = fit(name, data, nwalkers, nburn, nrun, prefit)
        results[name] = r = sampler.log_evidence(log_prior_norm=log_volume(BOUNDS[name]), seed=1)
        if verbose:
            print("%-5s logz %10.3f +- %.3f  (importance sampling %10.3f)  %d iterations, "
                  "neff %.0f of %d, %.1f %% of the proposals outside the prior"
                  % (name, r["logz"], r["logz_err"], r["logz_is"], r["iterations"], r["neff"],
                     r["n_post"], 100 * r["forbidden_fraction"]))
    lb, err = evidence.bayes_factor(results["ECPL"], results["PL"])
    results["log_bayes_factor"] = (lb, err)
    if verbose:
        print("log Bayes factor ECPL over PL: %.2f +- %.2f" % (lb, err))
    return results


if __name__ == "__main__":
    args = [int(v) for v in sys.argv[1:4]]
    main(*args)
