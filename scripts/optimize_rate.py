"""Time the lock-step simplex searches of naima_amd.optimize on the profile-likelihood batch of
workload cfg1: every parameter x 21 grid values x 4 starts = 252 searches, each with its
parameter pinned, against the same searches run one after another with the existing
neldermead.minimize_batched through lnprob on host arrays (what the package could do before).
Prints one JSON line:

  searches, ndim
  many_s             wall time of minimize_many on the whole batch (ends in the download of the
                     results), each of ``--repeats`` warm calls; many_iterations its loop trips
  sequential_s       wall time of the ``--baseline`` first searches of the same list, one after
                     another (all of them by default), each repeat; sequential_searches,
                     sequential_iterations (summed over the searches)
  speedup            sequential_s scaled to all searches over many_s, medians
  same_ends          the largest |x_many - x_sequential| / |x| over the baseline searches
  span_ms            device-event spans of an instrumented run of the same loop, summed over its
                     trips: propose (the simplex kernels that write the candidates), model (every
                     launch of the log-probability), update (the simplex kernels that take the
                     values, and the 8-byte download); simplex_share = (propose + update) / all.
                     The events add a synchronisation per phase, so this run is not the timed one.

    python scripts/optimize_rate.py [--repeats 3] [--baseline N]
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
from naima_amd import optimize as O  # noqa: E402
from naima_amd.neldermead import minimize_batched  # noqa: E402

OPTS = dict(xtol=1e-4, ftol=1e-4)


def profile_batch(mlx, sd, n=21, span=4.0, k=4, spread=0.05, seed=0):
    """(starts, frozen) of profile_likelihood's batch for every parameter"""
    rng = np.random.default_rng(seed)
    starts, frozen = [], []
    for p in range(mlx.size):
        for v in mlx[p] + span * sd[p] * np.linspace(-1.0, 1.0, n):
            for j in range(k):
                x = mlx.copy() if j == 0 else mlx + spread * mlx * rng.normal(size=mlx.size)
                x[p] = v
                f = np.zeros(mlx.size, dtype=bool)
                f[p] = True
                starts.append(x)
                frozen.append(f)
    return np.array(starts), np.array(frozen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", type=int, default=0, help="searches of the baseline (0: all)")
    a = ap.parse_args()
    ctx = _lib.get_context()
    model, p0, raw, data, prior, labels = build_problem("cfg1", na)
    rng = np.random.default_rng(1)
    ml = O.fit_ml(data, model, None, p0 + 0.05 * p0 * rng.normal(size=(8, p0.size)), **OPTS)
    sd = 0.02 * np.abs(ml.x)
    starts, frozen = profile_batch(ml.x, sd)
    S, ndim = starts.shape

    def fn(P):
        return na.lnprob(P, data, model, None)[0]

    def many():
        t0 = time.perf_counter()
        res = O.minimize_many(fn, starts, frozen, **OPTS)
        return time.perf_counter() - t0, res

    many()  # warm: code objects, pool buffers, tables
    many_s, res = [], None
    for _ in range(a.repeats):
        t, res = many()
        many_s.append(t)

    nb = S if a.baseline <= 0 else min(a.baseline, S)

    def sequential():
        t0 = time.perf_counter()
        ends, its = [], 0
        for x0, fz in zip(starts[:nb], frozen[:nb]):
            free = np.flatnonzero(~fz)

            def nll(Y, x0=x0, free=free):
                X = np.tile(x0, (len(Y), 1))
                X[:, free] = Y
                return -np.asarray(na.lnprob(np.ascontiguousarray(X.T), data, model, None)[0],
                                   dtype=float).reshape(-1)

            r = minimize_batched(nll, x0[free], **OPTS)
            x = x0.copy()
            x[free] = r["x"]
            ends.append(x)
            its += r["nit"]
        return time.perf_counter() - t0, np.array(ends), its

    sequential()
    seq_s, ends, seq_its = [], None, 0
    for _ in range(a.repeats):
        t, ends, seq_its = sequential()
        seq_s.append(t)

    # the instrumented loop: device-event spans per phase
    sb = O.SimplexBatch(ctx, starts, frozen, logp=True, **OPTS)
    span = dict(propose=0.0, model=0.0, update=0.0)
    trips = 0
    while trips == 0 or sb.active:
        ctx.timer_start()
        P = sb.propose()
        span["propose"] += ctx.timer_stop()
        ctx.timer_start()
        f = fn(P)
        ctx.flush()
        span["model"] += ctx.timer_stop()
        ctx.timer_start()
        sb.update(f)
        span["update"] += ctx.timer_stop()
        trips += 1
    total = sum(span.values())
    print(json.dumps(dict(
        workload="cfg1", searches=S, ndim=ndim, many_s=many_s,
        many_iterations=res["iterations"], many_status=np.bincount(res["status"]).tolist(),
        sequential_s=seq_s, sequential_searches=nb, sequential_iterations=int(seq_its),
        speedup=float(np.median(seq_s) * S / nb / np.median(many_s)),
        same_ends=float(np.max(np.abs(res["x"][:nb] - ends) / np.abs(ends))),
        span_ms=span, span_trips=trips, simplex_share=(span["propose"] + span["update"]) / total,
        device=ctx.info()["name"])))


if __name__ == "__main__":
    main()
