"""Time the rank-normalised statistics of naima_amd.posterior on a chain of 1000 rows x 512 walkers
x 4 parameters held in device memory: two ensembles of 256 walkers, every walker an AR(1) series
(phi = 0.5) in which every third row repeats the one before, as a rejected move does.  Prints one
JSON line; times are medians of 3 warm calls, each of which ends in a download of ndim numbers
(``rank_normalize``: in a device synchronisation through the download of one status word):

  rank_normalize_s     nh_rank_columns + nh_rank_normal_scores, the scores left in device memory
  rhat_rank_s          rhat(method="rank"): the chain and its folded values ranked, split moments
  rhat_moments_s       rhat(method="moments") on the same chain: nh_group_moments alone
  ess_bulk_s           ess(kind="bulk"): ranks, scores, emcee's tau of every parameter
  ess_tail_s           ess(kind="tail"): two quantiles, two indicator chains, their taus
  summary_s            summary(ensembles=2)
  values_per_s         rows x walkers x parameters / rank_normalize_s
  ndtri_max_rel_err    the largest relative difference between the device's scores of this chain
                       and scipy.special.ndtri of the same ranks

    python scripts/rank_rate.py
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naima_amd import _lib, posterior as P  # noqa: E402

ROWS, NW, ND, K = 1000, 512, 4, 2


def chain(rng):
    n = ROWS * 3 // 4 + 1
    e = rng.standard_normal((n, NW, ND))
    x = np.empty_like(e)
    x[0] = e[0]
    for t in range(1, n):
        x[t] = 0.5 * x[t - 1] + np.sqrt(0.75) * e[t]
    keep = np.sort(np.concatenate([np.arange(n), np.arange(0, n, 3)]))[:ROWS]
    return x[keep] * np.logspace(-2, 2, ND)


def median_time(fn, reps=3):
    fn()  # warm: code objects, pool buffers, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    x = chain(np.random.default_rng(20261019))
    assert x.shape == (ROWS, NW, ND)
    ctx = _lib.get_context()
    block = (ctx.array(x.reshape(ROWS, NW * ND)), ROWS, NW, ND)

    def normalize():
        z = P.rank_normalize(block, K, device=True)
        ctx.call("nh_copy", one, z[0], 8)  # (a download orders the host behind the stream)
        return one.get()

    one = ctx.empty((1,))
    out = {"shape": [ROWS, NW, ND], "ensembles": K, "device": ctx.info(),
           "rank_normalize_s": median_time(normalize),
           "rhat_rank_s": median_time(lambda: P.rhat(block, K, method="rank")),
           "rhat_moments_s": median_time(lambda: P.rhat(block, K)),
           "ess_bulk_s": median_time(lambda: P.ess(block, "bulk")),
           "ess_tail_s": median_time(lambda: P.ess(block, "tail")),
           "summary_s": median_time(lambda: P.summary(block, K))}
    out["values_per_s"] = x.size / out["rank_normalize_s"]
    out["rhat_rank"] = P.rhat(block, K, method="rank").tolist()
    out["rhat_moments"] = P.rhat(block, K).tolist()
    out["ess_bulk"] = P.ess(block, "bulk").tolist()
    out["ess_tail"] = P.ess(block, "tail").tolist()
    from scipy.special import ndtri
    r, z = P.rank_columns(x), P.rank_normalize(x)
    want = ndtri((r - 0.375) / (ROWS * NW + 0.25))
    nz = want != 0
    out["ndtri_max_rel_err"] = float(np.max(np.abs(z[nz] - want[nz]) / np.abs(want[nz])))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
