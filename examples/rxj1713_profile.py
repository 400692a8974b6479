"""The frequentist answer beside the Bayesian one: after the synchrotron + inverse-Compton fit of
examples/rxj1713_synic.py, refit the maximum-likelihood point by multi-start Nelder-Mead and take
the profile likelihood of every parameter (naima_amd.optimize) -- what Sherpa's ``conf`` / ``proj``
give for the reference's sherpa models.

    python examples/rxj1713_profile.py [nwalkers] [nburn] [nrun] [grid points]

All simplex searches -- 16 starts of the refit, then (parameters x grid values) searches of the
profiles, each with its parameter pinned -- advance in lock-step on the GPU: their candidate points
are one walker batch per iteration, and the simplex bookkeeping stays in HBM.  The Delta lnL = 1/2
interval of each parameter is printed beside the 16-84 % interval of its posterior; under a flat
prior and a near-Gaussian likelihood the two agree, and where they do not the posterior is
feeling a prior bound or a skewed likelihood.  ``modes`` lists the distinct optima the starts
reached: more than one says that the likelihood surface has a second maximum.

Data: the synthetic table of BASELINE workload cfg3 (naima_amd/workloads.py)."""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd import workloads as W  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u


def main(nwalkers=128, nburn=100, nrun=200, n=21, verbose=True):
    wl = W.WORKLOADS["cfg3"]
    model, p0, labels = wl["model"](naima), np.array(wl["p0"], dtype=float), wl["labels"]

    def flux_at_p0(E_eV):
        out = model(p0, {"energy": E_eV * u.eV})
        return (out[0] if isinstance(out, tuple) else out).to("1/(s cm2 eV)").value

    data = make_data(W.build_data("cfg3", flux_at_p0))
    sampler, _ = naima.run_sampler(data_table=data, p0=p0, labels=labels, model=model,
                                   prior=W.prior_for("cfg3", naima), nwalkers=nwalkers,
                                   nburn=nburn, nrun=nrun, prefit=True, seed=1, verbose=False)
    ml = sampler.fit_ml()
    best_sample = naima.find_ML(sampler)[0]
    profiles = sampler.profile_likelihood(list(range(len(labels))), ml=ml, n=n)
    chain = np.asarray(sampler.get_chain(flat=True))
    rows = []
    for p, pr in enumerate(profiles):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (a side the grid does not bracket prints as nan)
            lo, hi = pr.interval(0.683)
        q16, q84 = np.percentile(chain[:, p], [16, 84])
        rows.append((labels[p], ml.x[p], lo, hi, q16, q84))
    if verbose:
        print("maximum likelihood %.4f after the refit (best sample of the chain: log-probability "
              "%.4f); %d distinct optima from %d starts"
              % (ml.fun, best_sample, len(ml.modes), len(ml.ends)))
        print("%-15s %12s   %-27s %-27s" % ("parameter", "ML", "profile 68.3 %", "posterior 16-84 %"))
        for label, x, lo, hi, q16, q84 in rows:
            print("%-15s %12.5g   [%12.5g, %12.5g] [%12.5g, %12.5g]" % (label, x, lo, hi, q16, q84))
    return dict(ml=ml, profiles=profiles, rows=rows)


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:5]])
