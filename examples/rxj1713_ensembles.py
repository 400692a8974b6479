"""Four independent ensembles from dispersed starting points in one sampler, run until the
autocorrelation time AND the Gelman-Rubin statistic across the ensembles agree: the RX J1713-like
synchrotron + inverse-Compton fit of examples/rxj1713_synic.py through

    run_sampler(p0=starts[4][ndim], nwalkers=4 * n, nrun=max_steps,
                converge=dict(check_every=100, tol=50, rtol=0.01, rhat=1.01), ...)

The autocorrelation time of one ensemble cannot tell that the whole ensemble has settled in the
wrong place: every walker's proposal is built from another walker of the same ensemble.  Here each
walker's partner comes from its own ensemble of n, so the four are independent chains that share
every launch, and R-hat compares them on the GPU at every check.

    python examples/rxj1713_ensembles.py [walkers per ensemble] [nburn] [max_steps]

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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    max_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
    k = 4
    # dispersed starts: the point of the other examples and three others a few per cent away
    p0 = np.asarray(P0, dtype=float)
    starts = p0 * (1 + 0.03 * np.random.default_rng(7).standard_normal((k, p0.size)))
    starts[0] = p0
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=starts, labels=LABELS, model=ElectronSynIC,
                                     prior=lnprior, nwalkers=k * n, nburn=nburn, nrun=max_steps,
                                     converge=dict(check_every=100, tol=50, rtol=0.01, rhat=1.01),
                                     seed=1, verbose=False)
    dt = time.time() - t0
    conv = sampler.convergence
    print("%s after %d of at most %d steps (%d ensembles of %d walkers, seeds %s, %.2f s, checks "
          "on the %s)" % ("converged" if conv["converged"] else "NOT converged", conv["rows"],
                          max_steps, sampler.ensembles, n, sampler.seeds, dt, conv["where"]))
    for rows, tau, rhat in conv["history"][-5:]:
        print("  %6d rows: tau = %s  R-hat = %s" % (rows, np.array2string(tau, precision=2),
                                                    np.array2string(rhat, precision=4)))
    print("R-hat of the stored chain:", sampler.get_rhat())
    # every ensemble's own median, side by side
    med = np.median(sampler.split_ensembles(sampler.get_chain()), axis=(0, 2))
    for r in range(k):
        print("  ensemble %d median: %s" % (r, np.array2string(med[r], precision=4)))
    print("run_info:", {q: sampler.run_info[q] for q in ("ensembles", "seeds", "converged", "rhat")})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rxj1713_ensembles_run")
    naima.save_run(out, sampler, clobber=True)
    back = naima.read_run(out)
    assert int(back.run_info["ensembles"]) == k
    print("saved and read back:", out + ".npz")
