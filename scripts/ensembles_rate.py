"""Walker-steps per second of k independent ensembles of n walkers in one sampler
(EnsembleSampler(ensembles=k)) against ONE ensemble of n and one of k n walkers, on the device
loop, for the table-only workloads cfg1 and cfg5.  Prints one JSON line per (workload, k, n):

  one_n         one ensemble of n walkers                       (what a small fit runs at)
  k_by_n        k ensembles of n walkers, one launch per half-step for all of them
  one_kn        one ensemble of k n walkers                     (the launch shape k_by_n has)

each the median of `--reps` timed calls of `--steps` steps that end with the ensemble on the
host, after a warm-up call of as many steps; blobs are not kept, the chain is.

    python scripts/ensembles_rate.py [--n 32] [--k 4 16] [--steps 200] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as na  # noqa: E402
from bench import build_problem  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402


def rate(problem, nw, k, steps, reps):
    model, p0, raw, data, prior, labels = problem
    s = EnsembleSampler(nw, p0.size, na.lnprob, args=[data, model, prior], seed=11,
                        naima_style=True, store_blobs=False, device=True, nan_policy="reject",
                        ensembles=k)
    pos = p0 * (1 + 0.003 * np.random.default_rng(3).standard_normal((nw, p0.size)))
    with np.errstate(all="ignore"):
        st = s.run_mcmc(pos, 4)       # (settles and records the plan)
        st = s.run_mcmc(st, steps)    # warm
        np.asarray(st.coords)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            st = s.run_mcmc(st, steps)
            np.asarray(st.coords)
            ts.append(time.perf_counter() - t0)
    assert s._dev is not None and s.device
    return nw * steps / float(np.median(ts)), s._dev.resident_launches > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--k", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["cfg1", "cfg5"])
    a = ap.parse_args()
    for name in a.workloads:
        problem = build_problem(name, na)
        one_n, res = rate(problem, a.n, 1, a.steps, a.reps)
        for k in a.k:
            k_by_n, res_k = rate(problem, k * a.n, k, a.steps, a.reps)
            one_kn, _ = rate(problem, k * a.n, 1, a.steps, a.reps)
            print(json.dumps(dict(workload=name, k=k, n=a.n, steps=a.steps, reps=a.reps,
                                  one_n=round(one_n), k_by_n=round(k_by_n), one_kn=round(one_kn),
                                  speedup_over_one_n=round(k_by_n / one_n, 2),
                                  resident=bool(res and res_k))), flush=True)


if __name__ == "__main__":
    main()
