"""Run a fit until its autocorrelation time has converged instead of guessing nrun: the RX
J1713-like synchrotron + inverse-Compton fit of examples/rxj1713_synic.py through

    run_sampler(nrun=max_steps, converge=dict(check_every=100, tol=50, rtol=0.01), ...)

which is the loop of emcee's tutorial "Autocorrelation analysis & convergence": every 100 steps
the integrated autocorrelation time tau of every parameter is estimated, and the run stops once
the chain is longer than 50 tau and tau has changed by less than 1 %.  On the device loop the chain
stays in HBM between the checks and the lag sums grow with it, so a check costs the new rows only.

    python examples/rxj1713_converged.py [nwalkers] [nburn] [max_steps]

Data: the synthetic X-ray + TeV table of BASELINE workload cfg3 (naima_amd/workloads.py)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from rxj1713_luminosity import LABELS, P0, ElectronSynIC, lnprior, synthetic_data  # noqa: E402

if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    max_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS, model=ElectronSynIC,
                                     prior=lnprior, nwalkers=nwalkers, nburn=nburn, nrun=max_steps,
                                     converge=dict(check_every=100, tol=50, rtol=0.01),
                                     prefit=True, seed=1, verbose=False)
    dt = time.time() - t0
    conv = sampler.convergence
    print("%s after %d of at most %d steps (%d walkers, %.2f s, checks on the %s, %d lags kept, "
          "%d rebuilds)" % ("converged" if conv["converged"] else "NOT converged", conv["rows"],
                            max_steps, nwalkers, dt, conv["where"], conv["max_lag"],
                            conv["rebuilds"]))
    for rows, tau in conv["history"][-5:]:
        print("  %6d rows: tau = %s" % (rows, np.array2string(tau, precision=2)))
    print("run_info:", {k: sampler.run_info[k] for k in ("n_run", "converged", "autocorr_time")})
    assert sampler.get_chain().shape[0] == conv["rows"] == sampler.iteration
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rxj1713_converged_run")
    naima.save_run(out, sampler, clobber=True)
    back = naima.read_run(out)
    assert bool(back.run_info["converged"]) == conv["converged"]
    naima.save_results_table(out, sampler, overwrite=True)
    print("saved and read back:", out + ".npz")
