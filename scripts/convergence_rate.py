"""What watching a run's autocorrelation time costs: the headline workload (cfg3) makes --steps
ensemble steps three ways, each from a fresh warm sampler of the same seed, the stream synchronised
at both ends of the timed window, and prints one JSON line:

  a_plain_s       run_mcmc(steps)
  b_monitored_s   run_until_converged(max_steps=steps, check_every=..., tol too large to stop):
                  the chain and the lag sums stay in HBM (autocorr.RunningAutocorr)
  c_tutorial_s    the loop of emcee's tutorial on the API without it: sample(iterations=steps,
                  yield_every=check_every) with get_autocorr_time(tol=0) at every check_every-th
                  iteration (every check downloads the new rows, uploads the whole chain again
                  and recomputes every lag sum)
  c2_calls_s      the same loop as plain calls: run_mcmc(check_every) and get_autocorr_time(tol=0),
                  again and again (every call may take the resident loop; the chain still travels)
  b_minus_a_s, c_minus_a_s, c2_minus_a_s   the price of the monitoring alone
  rows_seen       the rows of the chain the last check of each loop looked at

--reps repeats (a) and (b), alternating, and reports the median and the spread; (c) runs --reps-c
times.  --no-blobs samples without keeping the blobs.

    python scripts/convergence_rate.py --steps 20000 --check-every 100
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naima_amd as na  # noqa: E402
from bench import build_problem  # noqa: E402
from naima_amd import _lib  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--check-every", type=int, default=100)
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--max-lag", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--reps-c", type=int, default=1)
    ap.add_argument("--no-blobs", action="store_true")
    args = ap.parse_args()
    nw, steps, every = args.walkers, args.steps, args.check_every
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    nd = p0.size
    ctx = _lib.get_context()

    def warm():
        s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=20261018,
                            naima_style=True, store_blobs=not args.no_blobs, device=True,
                            nan_policy="reject")
        pos = p0 + 0.1 * p0 * np.random.default_rng(20261018).normal(size=(nw, nd))
        st = s.run_mcmc(pos, 8)
        st = s.run_mcmc(st, 2 * every)  # (warm: the plan made, the resident loop created)
        s.get_autocorr_time(tol=0)      # (... and the autocorrelation kernels loaded)
        s.reset()
        ctx.sync()
        return s, st

    def plain():
        s, st = warm()
        t0 = time.perf_counter()
        s.run_mcmc(st, steps)
        ctx.sync()
        return time.perf_counter() - t0, s, None

    def monitored():
        s, st = warm()
        t0 = time.perf_counter()
        s.run_until_converged(st, steps, check_every=every, tol=1e12, max_lag=args.max_lag)
        ctx.sync()
        return time.perf_counter() - t0, s, s.convergence["tau"]

    def tutorial():
        s, st = warm()
        tau = None
        t0 = time.perf_counter()
        for _ in s.sample(st, iterations=steps, yield_every=every):
            if s.iteration % every:
                continue
            tau = s.get_autocorr_time(tol=0)
        ctx.sync()
        return time.perf_counter() - t0, s, tau

    def calls():
        s, st = warm()
        tau = None
        t0 = time.perf_counter()
        for _ in range(0, steps, every):
            st = s.run_mcmc(st, every)
            tau = s.get_autocorr_time(tol=0)
        ctx.sync()
        return time.perf_counter() - t0, s, tau

    times = dict(a=[], b=[], c=[], c2=[])
    rows_seen = {}
    taus, info, resident = {}, None, {}
    with np.errstate(all="ignore"):
        for r in range(max(args.reps, args.reps_c)):
            for key, fn, n in (("a", plain, args.reps), ("b", monitored, args.reps),
                               ("c", tutorial, args.reps_c), ("c2", calls, args.reps_c)):
                if r >= n:
                    continue
                t, s, tau = fn()
                times[key].append(t)
                resident[key] = s._dev.resident_launches
                if tau is not None:
                    taus[key] = [float(x) for x in tau]
                    rows_seen[key] = int(s.get_chain().shape[0])
                if key == "b":
                    info = {k: s.convergence[k] for k in ("where", "max_lag", "rebuilds", "rows")}
                    info["checks"] = len(s.convergence["history"])
                print("%s: %.3f s" % (key, t), file=sys.stderr, flush=True)
                del s

    def med(v):
        return float(np.median(v)) if v else None

    a, b, c, c2 = med(times["a"]), med(times["b"]), med(times["c"]), med(times["c2"])
    out = dict(steps=steps, walkers=nw, check_every=every, blobs_kept=not args.no_blobs,
               a_plain_s=a, b_monitored_s=b, c_tutorial_s=c, c2_calls_s=c2, all_times=times,
               b_minus_a_s=b - a, c_minus_a_s=(c - a) if c is not None else None,
               c2_minus_a_s=(c2 - a) if c2 is not None else None, rows_seen=rows_seen,
               plain_walker_steps_per_s=steps * nw / a,
               monitored_walker_steps_per_s=steps * nw / b,
               tau_monitored=taus.get("b"), tau_tutorial=taus.get("c"),
               tau_calls=taus.get("c2"), monitored=info,
               resident_launches=resident)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
