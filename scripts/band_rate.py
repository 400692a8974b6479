"""Walker-steps per second of the Syn+IC model of examples/rxj1713_luminosity.py with and
without its two band-integral blobs (1-100 TeV IC luminosity, 2-10 keV synchrotron flux).

With the blobs the model runs the per-launch fused device loop (nh_step_front and captured
graphs): the one-launch half-step and the resident loop do not know nh_trapz_loglog_comps.
Without them it is measured twice: on the loop it takes by default (resident), and on the same
per-launch loop (NAIMA_AMD_RESIDENT=0 NAIMA_AMD_MEGA=0), which isolates what the extra launches
cost.  The three are timed in turn, ``--repeat`` times over, and one JSON line is printed per
model and turn.

    python scripts/band_rate.py [--walkers 512] [--steps 200] [--warmup 20] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import naima_amd as naima  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402
from rxj1713_luminosity import (P0, ElectronSynIC, ElectronSynICBands, lnprior,  # noqa: E402
                                synthetic_data)


def rate(model, data, nw, steps, warmup, per_launch):
    for k in ("NAIMA_AMD_RESIDENT", "NAIMA_AMD_MEGA"):
        if per_launch:
            os.environ[k] = "0"
        else:
            os.environ.pop(k, None)
    s = EnsembleSampler(nw, P0.size, naima.lnprob, args=[data, model, lnprior], seed=3,
                        naima_style=True, store_blobs=True, device=True)
    pos = P0 * (1 + 1e-3 * np.random.default_rng(4).standard_normal((nw, P0.size)))
    st = s.run_mcmc(pos, warmup)
    s._dev.ctx.sync()
    t0 = time.perf_counter()
    s.run_mcmc(st, steps)
    s._dev.ctx.sync()
    dt = time.perf_counter() - t0
    d = s._dev
    plan = getattr(d, "_plan", None)
    return dict(walker_steps_per_s=nw * steps / dt, seconds=dt, device=bool(s.device),
                fused=bool(d.fused), mega=bool(d.mega),
                launches_per_half_step=list(plan.calls) if plan else None,
                acceptance=float(np.mean(s.acceptance_fraction)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    data = synthetic_data()
    cases = (("with_band_blobs", ElectronSynICBands, False),
             ("without_per_launch_loop", ElectronSynIC, True),
             ("without_default_loop", ElectronSynIC, False))
    for turn in range(a.repeat):
        for name, model, per_launch in cases:
            r = rate(model, data, a.walkers, a.steps, a.warmup, per_launch)
            print(json.dumps(dict(model=name, turn=turn, walkers=a.walkers, steps=a.steps, **r)),
                  flush=True)
