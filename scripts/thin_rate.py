"""What thinning a run on the GPU costs and saves: the headline workload (cfg3, blobs kept) makes
--steps ensemble steps as ``run_mcmc(pos, steps / t, thin_by=t)`` and prints one JSON line:

  walker_steps_per_s   up to the end of the last launch (the stream synchronised), the sampler
                       warm (plan made, resident loop created) and reset before the timed call
  get_chain_s          the get_chain() that follows: download of the kept block + the host's lists
  thin_info            what the device loop did (staging rows and bytes, internal calls)
  compaction_us        one chunk's nh_hist_thin launch, timed alone: the median over --reps of 20
                       launches queued back to back on blocks of the run's own shapes

With --thin-by 1 the thin_by argument is not passed at all, so the same script measures a tree
that does not have it: NAIMA_AMD_TREE=<another checkout, built> makes the script import
naima_amd and bench from there.

    python scripts/thin_rate.py --steps 12800 --thin-by 8
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("NAIMA_AMD_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naima_amd as na  # noqa: E402
from bench import build_problem  # noqa: E402
from naima_amd import _lib  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12800)
    ap.add_argument("--thin-by", type=int, default=1)
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    t, nw = args.thin_by, args.walkers
    assert args.steps % t == 0
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    nd = p0.size
    s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=20260929,
                        naima_style=True, store_blobs=True, device=True, nan_policy="reject")
    pos = p0 + 0.1 * p0 * np.random.default_rng(20260929).normal(size=(nw, nd))
    ctx = _lib.get_context()
    kw = dict(thin_by=t) if t != 1 else {}
    with np.errstate(all="ignore"):
        st = s.run_mcmc(pos, 8)
        st = s.run_mcmc(st, 64 // t if t <= 64 else 1, **kw)  # (warm: every path the timed call takes)
        s.reset()
        ctx.sync()
        t0 = time.perf_counter()
        st = s.run_mcmc(st, args.steps // t, **kw)
        ctx.sync()
        t1 = time.perf_counter()
    dev = s._dev
    info = getattr(dev, "thin_info", None)
    kept_rows = sum(b.coords.shape[0] for b in dev.hist)
    t2 = time.perf_counter()
    chain = s.get_chain()
    t3 = time.perf_counter()
    out = dict(tree=ROOT, steps=args.steps, thin_by=t, walkers=nw,
               walker_steps_per_s=args.steps * nw / (t1 - t0), run_s=t1 - t0,
               get_chain_s=t3 - t2, chain_shape=list(chain.shape), kept_rows_in_hbm=kept_rows,
               resident_launches=dev.resident_launches,
               acceptance=float(np.mean(s.acceptance_fraction)))
    if info is not None and t != 1:
        out["thin_info"] = dict(info, calls=len(info["calls"]), first_call=list(info["calls"][0]))
        if info["where"] == "device" and info["stage_rows"] >= t:
            c = info["stage_rows"] // t
            stage, compact = dev._new_block(info["stage_rows"]), dev._new_block(c)
            times = []
            for _ in range(args.reps + 1):
                ctx.sync()
                a = time.perf_counter()
                for _ in range(20):
                    compact.n = 0
                    dev._compact(stage, compact, t - 1, t, c)
                ctx.sync()
                times.append((time.perf_counter() - a) / 20 * 1e6)
            row = 8 * nw * (nd + 1 + sum(b.m for b in dev.cur_blobs))
            out["compaction_us"] = float(np.median(times[1:]))
            out["compaction_rows"] = c
            out["compaction_gb_per_s"] = 2 * c * row / (out["compaction_us"] * 1e-6) / 1e9
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
