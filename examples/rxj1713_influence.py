"""Which data set drives which parameter of an RX J1713-like X-ray + TeV fit, and would a new VHE
upper limit move it?  One synchrotron + inverse-Compton fit of the joint table; then the samples
already held are reweighted (naima_amd.reweight: Pareto-smoothed importance weights and weighted
reductions on the GPU) instead of fitting again:

  * ``sampler.influence()`` leaves the X-ray points and the TeV points out in turn;
  * ``sampler.reweight(new_data=...)`` adds one new upper limit at the last TeV point's energy.

A ``pareto_k`` above 0.7 means the new target is too far from the fitted one for these samples:
refit, do not reweight.  Leaving a whole instrument out of a joint fit usually is (the fit is
what ties the two together); one more point usually is not.

    python examples/rxj1713_influence.py [nwalkers] [nburn] [nrun]

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
LABELS = ["log10(norm)", "index", "log10(cutoff)", "B", "beta"]


def ECPL(pars, data):
    e = naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                        10 ** pars[2] * u.TeV, beta=pars[4])
    IC = naima.InverseCompton(e, seed_photon_fields=["CMB", "FIR", "NIR"], Eemin=100 * u.GeV)
    SYN = naima.Synchrotron(e, B=pars[3] * u.uG)
    return IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)


def prior(p):
    return (naima.uniform_prior(p[1], -1, 5) + naima.uniform_prior(p[2], -3, 5)
            + naima.uniform_prior(p[3], 0, np.inf) + naima.uniform_prior(p[4], 0.1, 5))


def new_upper_limit(sampler, discard):
    """a table of one point: an upper limit at the energy of the last measured TeV point, as deep
    as the posterior median of the model there -- half of the posterior violates it"""
    from naima_amd.core import _conversion_to_data
    data = sampler.data
    last = int(np.flatnonzero(~np.asarray(data["ul"]))[-1])
    one = slice(last, last + 1)
    spectra = np.asarray(sampler.get_blobs(discard=discard)[0], dtype=float)
    model = spectra.reshape(-1, spectra.shape[-1])[:, last] \
        * _conversion_to_data(sampler.blob_units[0], data)[last]
    return {"energy": u.Quantity(data["energy"].value[one], data["energy"].unit),
            "flux": u.Quantity(np.full(1, np.median(model)), data["flux"].unit),
            "flux_error_lo": u.Quantity(data["flux_error_lo"].value[one], data["flux"].unit),
            "flux_error_hi": u.Quantity(data["flux_error_hi"].value[one], data["flux"].unit),
            "ul": np.ones(1, bool), "cl": np.full(1, 0.95)}


def main(nwalkers=256, nburn=100, nrun=300, verbose=True, prefit=True):
    p0 = np.array(W.WORKLOADS["cfg3"]["p0"], dtype=float)
    data = make_data(W.build_data(
        "cfg3", lambda E_eV: ECPL(p0, {"energy": E_eV * u.eV}).to("1/(s cm2 eV)").value))
    data["group"] = (data["energy"].to("eV").value > 1e9).astype(int)  # 0: X-ray, 1: TeV
    sampler, _ = naima.run_sampler(data_table=data, p0=p0, labels=LABELS, model=ECPL, prior=prior,
                                   nwalkers=nwalkers, nburn=nburn, nrun=nrun, prefit=prefit, seed=1,
                                   verbose=False)
    discard = nrun // 2
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        infl = sampler.influence(discard=discard)
        added = sampler.reweight(new_data=new_upper_limit(sampler, discard), discard=discard)
    if verbose:
        names = {0: "X-ray", 1: "TeV"}
        print("%-14s %8s %9s %8s   shift of the mean, in fitted sd" % ("left out", "points",
                                                                      "pareto_k", "ESS"))
        for r in infl:
            shifts = "  ".join("%s %+.2f" % lv for lv in zip(LABELS, r["shift"]))
            print("%-14s %8d %9.2f %8.1f   %s" % (names.get(r["group"], r["group"]), r["n_points"],
                                                  r["pareto_k"], r["ess"], shifts))
        sm = added.summary()
        print("one new upper limit: pareto_k %.2f, ESS %.1f of %d, log evidence ratio %.3f"
              % (added.weights.pareto_k[0], added.weights.ess[0], added.weights.n_samples,
                 added.log_evidence_ratio))
        for i, label in enumerate(sm["labels"]):
            print("  %-14s %.4g +- %.2g  ->  %.4g +- %.2g  (%+.2f sd)"
                  % (label, sm["mean_unweighted"][i], sm["sd_unweighted"][i], sm["mean"][i],
                     sm["sd"][i], sm["shift"][i]))
        for w in caught:
            print("warning:", w.message)
    return infl, added


if __name__ == "__main__":
    args = [int(v) for v in sys.argv[1:4]]
    main(*args)
