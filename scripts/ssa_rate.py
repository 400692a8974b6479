"""Times of the self-absorption kernels beside nh_synchrotron at the same shape, and walker-steps
per second of the compact synchrotron + SSC fit (examples/blob_ssc.py) with and without the
factor, both on the per-launch fused device loop (nh_step_front and captured graphs;
NAIMA_AMD_RESIDENT=0 NAIMA_AMD_MEGA=0, which the absorbed model takes anyway: the one-launch
half-step does not know nh_syn_absorption or nh_ssa_apply).

  nh_synchrotron, nh_syn_absorption   512 walkers x 32 energies on naima's default electron
                    grid (1 GeV .. 1e9 m_e c^2, 100 nodes per decade), exponential cutoff power
                    laws, device events around `reps` launches of each
  nh_ssa_apply      the sphere's factor times a one-term flux, device events around `reps` launches
  the fit           host clock around run_mcmc, ending in a device synchronise

Prints one JSON line per measurement.

    python scripts/ssa_rate.py [--walkers 512] [--energies 32] [--steps 1000] [--warmup 100]
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

import blob_ssc as BS  # noqa: E402
import naima_amd as naima  # noqa: E402
from naima_amd import _lib  # noqa: E402
from naima_amd.constants import MEC2_EV  # noqa: E402
from naima_amd.darray import DMat, DSsa, DVec  # noqa: E402
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
    rng = np.random.default_rng(1)
    gam = naima.Synchrotron(naima.PowerLaw(1 / u.eV, 1 * u.TeV, 2.0))._gam
    nG = gam.size
    rows = np.zeros((nw, 8))
    rows[:, 0] = 10 ** rng.normal(33, 0.1, nw)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = 1e13, rng.uniform(2, 3, nw), 5e13, 1.0
    gd, ed, rd = ctx.array(gam), ctx.array(gam * MEC2_EV), ctx.array(rows)
    w, dlw, lx = ctx.empty((nw, nG)), ctx.empty((nw, nG)), ctx.empty((nG - 1,))
    ctx.call("nh_particle_weights", 1, rd, nw, ed, gd, nG, MEC2_EV, w, dlw, None)
    ctx.call("nh_grid_logratio", gd, nG, lx)
    B = ctx.array(10 ** rng.uniform(-5.3, -4.3, nw))
    E = ctx.array(np.geomspace(1e-7, 1e4, nE))
    out = []
    spec, kap = ctx.empty((nw, nE)), ctx.empty((nw, nE))
    args = (w, dlw, B, 1, nw, gd, lx, nG, E, nE)
    for name, buf in (("nh_synchrotron", spec), ("nh_syn_absorption", kap)):
        r = timed(ctx, lambda: ctx.call(name, *args, buf, nE), reps)
        out.append(dict(what=name, walkers=nw, energies=nE, nodes=nG,
                        integrals_per_s=nw * nE / (r["us_median"] * 1e-6), **r))
    Rd = ctx.array(10 ** rng.uniform(15, 17, nw))
    fac = DSsa(ctx, kap, True, DVec(ctx, Rd, Rd.ptr, nw), "sphere", nw, nE)
    flux = DMat.from_buffer(ctx, spec, nw, nE)
    r = timed(ctx, lambda: fac.apply(flux), reps)
    out.append(dict(what="nh_ssa_apply, sphere x 1 term", walkers=nw, energies=nE,
                    bytes=8 * nw * nE * 3, **r))
    return out


def rate(absorb, nw, steps, warmup):
    BS.ABSORB = True
    data = BS.synthetic_data()
    BS.ABSORB = absorb
    nd = BS.P0.size
    s = EnsembleSampler(nw, nd, naima.lnprob, args=[data, BS.BlobSSC, BS.lnprior], seed=3,
                        naima_style=True, store_blobs=False, device=True)
    pos = BS.P0 * (1 + 1e-3 * np.random.default_rng(4).standard_normal((nw, nd)))
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
    ap.add_argument("--energies", type=int, default=32)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    for r in kernels(a.walkers, a.energies, a.reps):
        print(json.dumps(r), flush=True)
    # alternating, twice each: the spread between equal runs stands beside the difference
    for rnd in range(2):
        for name, absorb in (("absorbed", True), ("thin", False)):
            r = rate(absorb, a.walkers, a.steps, a.warmup)
            print(json.dumps(dict(model=name, round=rnd, walkers=a.walkers, steps=a.steps, **r)),
                  flush=True)
