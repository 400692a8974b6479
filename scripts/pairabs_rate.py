"""Times of the pair-absorption kernels and walker-steps per second of the absorbed PeVatron
fit (examples/pevatron_absorbed.py) with and without the factor, both on the per-launch fused
device loop (nh_step_front and captured graphs; NAIMA_AMD_RESIDENT=0 NAIMA_AMD_MEGA=0, which
the absorbed model takes anyway: the one-launch half-step does not know nh_pairabs_apply).

  nh_pairabs_rows   one shared row (a cached table build) and one row per walker (a thermal
                    field with a free temperature), device events around `reps` launches
  nh_pairabs_apply  two fields times a one-term flux, device events around `reps` launches
  the fit           host clock around run_mcmc, ending in a device synchronise

Prints one JSON line per measurement.

    python scripts/pairabs_rate.py [--walkers 512] [--energies 20] [--steps 2000] [--warmup 200]
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
os.environ["NAIMA_AMD_RESIDENT"] = "0"
os.environ["NAIMA_AMD_MEGA"] = "0"

import naima_amd as naima  # noqa: E402
import pevatron_absorbed as PA  # noqa: E402
from naima_amd import _lib  # noqa: E402
from naima_amd.darray import DMat, DPairAbs, DVec  # noqa: E402
from naima_amd.models import PairAbsorptionModel  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402

u = naima.u


def timed(ctx, fn, reps, rounds=5):
    """median over `rounds` of the device time of one call, from `reps` calls between two events"""
    fn()
    ctx.sync()
    ms = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps):
            fn()
        ms.append(ctx.timer_stop() / reps)
    return dict(us_median=1e3 * float(np.median(ms)), us_min=1e3 * float(np.min(ms)),
                us_max=1e3 * float(np.max(ms)), reps=reps, rounds=rounds)


def kernels(nw, nE, reps):
    ctx = _lib.get_context()
    x = np.geomspace(1e12, 2.5e15, nE) / 510998.9499961643
    xd = ctx.const(x)
    out = []
    one = ctx.empty((1, nE))
    r = timed(ctx, lambda: PairAbsorptionModel._rows_launch(
        ctx, True, _lib.NH_PAIR_THERMAL, 2.72548, None, None, None, 0, xd, nE, 1, one), reps)
    out.append(dict(what="nh_pairabs_rows shared row", rows=1, energies=nE, **r))
    Td = ctx.array(np.random.default_rng(1).uniform(20, 60, nw))
    T = DVec(ctx, Td, Td.ptr, nw)
    per = ctx.empty((nw, nE))
    for theta, tag in ((None, "isotropic"), (1.0, "at an angle")):
        r = timed(ctx, lambda: PairAbsorptionModel._rows_launch(
            ctx, True, _lib.NH_PAIR_THERMAL, T, theta, None, None, 0, xd, nE, nw, per), reps)
        out.append(dict(what="nh_pairabs_rows per-walker rows, " + tag, rows=nw, energies=nE,
                        integrals_per_s=nw * nE / (r["us_median"] * 1e-6), **r))
    Ld = ctx.array(np.random.default_rng(2).uniform(1, 10, nw) * 3.0856775814913673e21)
    L = DVec(ctx, Ld, Ld.ptr, nw)
    fac = DPairAbs(ctx, [(one, False, L, 4.17e-13, 2.72548), (per, True, L, 8e-13, T)], nw, nE)
    flux = DMat.from_buffer(ctx, ctx.array(np.random.default_rng(3).uniform(1, 2, (nw, nE))), nw, nE)
    r = timed(ctx, lambda: fac.apply(flux), reps)
    out.append(dict(what="nh_pairabs_apply, 2 fields x 1 term", rows=nw, energies=nE,
                    bytes=8 * nw * nE * 3 + 8 * nE, **r))
    return out


def rate(absorb, nw, steps, warmup):
    PA.ABSORB = absorb
    data = PA.synthetic_data()
    nd = 4 if absorb else 3
    prior = PA.lnprior if absorb else (lambda p: naima.uniform_prior(p[0], 25, 40)
                                       + naima.uniform_prior(p[1], 1, 4)
                                       + naima.uniform_prior(p[2], 1, 5))
    s = EnsembleSampler(nw, nd, naima.lnprob, args=[data, PA.AbsorbedPeVatron, prior], seed=3,
                        naima_style=True, store_blobs=True, device=True)
    pos = PA.P0[:nd] * (1 + 1e-3 * np.random.default_rng(4).standard_normal((nw, nd)))
    st = s.run_mcmc(pos, warmup)
    s._dev.ctx.sync()
    t0 = time.perf_counter()
    s.run_mcmc(st, steps)
    s._dev.ctx.sync()
    dt = time.perf_counter() - t0
    d = s._dev
    return dict(walker_steps_per_s=nw * steps / dt, seconds=dt, device=bool(s.device),
                fused=bool(d.fused), mega=bool(d.mega),
                launches_per_half_step=list(d._plan.calls),
                acceptance=float(np.mean(s.acceptance_fraction)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--energies", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    for r in kernels(a.walkers, a.energies, a.reps):
        print(json.dumps(r), flush=True)
    # alternating, twice each: the spread between equal runs stands beside the difference
    for rnd in range(2):
        for name, absorb in (("absorbed", True), ("unabsorbed", False)):
            r = rate(absorb, a.walkers, a.steps, a.warmup)
            print(json.dumps(dict(model=name, round=rnd, walkers=a.walkers, steps=a.steps, **r)),
                  flush=True)
