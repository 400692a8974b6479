"""Times of the cooling kernels and walker-steps per second of the cooled pulsar wind nebula fit
(examples/pwn_cooled.py) with the cooling solve and with a plain power law in its place.

  nh_cooled_electrons   the solve of `walkers` walkers on `nodes` nodes with two photon fields,
                        device events around `reps` launches
  nh_cooled_weights     its rows resampled onto a particle grid of the same size
  the loss table        its build for two fields on that grid, host clock ending in a synchronise
  the fit               host clock around run_mcmc, ending in a device synchronise; with cooling
                        the model runs on the piecewise device loop, without it on the loop the
                        sampler picks for a PowerLaw model

Prints one JSON line per measurement.

    python scripts/cooling_rate.py [--walkers 512] [--nodes 570] [--steps 400] [--warmup 50]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import naima_amd as naima  # noqa: E402
import pwn_cooled as PWN  # noqa: E402
from naima_amd import _lib  # noqa: E402
from naima_amd.darray import DVec, nh_lazy  # noqa: E402
from naima_amd.models import cool_status  # noqa: E402
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


def kernels(nw, nC, reps):
    ctx = _lib.get_context()
    rng = np.random.default_rng(1)
    e = np.geomspace(1e9, 510.998e12, nC)
    model = naima.CooledElectrons((e * u.eV, np.ones(nC) / u.eV / u.s), 10 * u.uG, 1e3 * u.yr,
                                  ["CMB", "FIR"])
    ed = ctx.const(e)
    out = []
    # the loss table's build (two fields: nh_cooled_ic_rows + nh_trapz_loglog_comps each, and a
    # synchronise), host clock, with the cache entry dropped before each of five builds
    key = [k for k in ctx._tables if k[0] == "cool-loss" and k[1] == ed.ptr]
    ms = []
    for _ in range(5):
        for k in key:
            del ctx._tables[k]
        ctx.sync()
        t0 = time.perf_counter()
        loss = model._loss_table(ctx, ed)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    out.append(dict(what="loss table build (host clock)", nodes=nC, fields=2,
                    ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                    ms_max=float(np.max(ms))))
    Q = ctx.array(1e36 * (e[None, :] / 1e12) ** -rng.uniform(1.8, 2.6, (nw, 1)))
    keep = [ctx.array(v) for v in (10 ** rng.uniform(-6, -4, nw), 10 ** rng.uniform(9, 14, nw),
                                   np.full(nw, 4.2e-13), rng.uniform(2e-13, 2e-12, nw))]
    lz = [DVec(ctx, d, d.ptr, nw).lazy() for d in keep]
    ul = (nh_lazy * 2)(lz[2], lz[3])
    n = ctx.empty((nw, nC))
    st = cool_status(ctx)
    r = timed(ctx, lambda: ctx.call("nh_cooled_electrons", Q, nC, nw, ed, nC, C.addressof(lz[0]),
                                    loss, 2, ul, C.addressof(lz[1]), n, st), reps)
    out.append(dict(what="nh_cooled_electrons", walkers=nw, nodes=nC, fields=2,
                    nodes_per_s=nw * nC / (r["us_median"] * 1e-6), **r))
    xg = ctx.const(e / 510998.9499961643)
    w, lw = ctx.empty((nw, nC)), ctx.empty((nw, nC))
    eg = ctx.const(np.geomspace(1e9, 400e12, nC))
    r = timed(ctx, lambda: ctx.call("nh_cooled_weights", n, ed, nC, nw, eg, xg, nC,
                                    510998.9499961643, w, lw), reps)
    out.append(dict(what="nh_cooled_weights", walkers=nw, nodes=nC, target_nodes=nC,
                    bytes=8 * nw * nC * 3, **r))
    assert int(st.get()[0]) == 0 and np.all(np.isfinite(n.get()))
    return out


def rate(cooling, nw, steps, warmup):
    PWN.COOLING = True
    data = PWN.synthetic_data()
    PWN.COOLING = cooling
    s = EnsembleSampler(nw, 2, naima.lnprob, args=[data, PWN.CooledPWN, PWN.lnprior], seed=3,
                        naima_style=True, store_blobs=False, device=True)
    pos = PWN.P0 * (1 + 1e-3 * np.random.default_rng(4).standard_normal((nw, 2)))
    st = s.run_mcmc(pos, warmup)
    s._dev.ctx.sync()
    t0 = time.perf_counter()
    s.run_mcmc(st, steps)
    s._dev.ctx.sync()
    dt = time.perf_counter() - t0
    d = s._dev
    return dict(walker_steps_per_s=nw * steps / dt, seconds=dt, device=bool(s.device),
                fused=bool(d.fused), mega=bool(d.mega), graph=d.graph is not None,
                acceptance=float(np.mean(s.acceptance_fraction)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--nodes", type=int, default=570)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    for r in kernels(a.walkers, a.nodes, a.reps):
        print(json.dumps(r), flush=True)
    # alternating, twice each: the spread between equal runs stands beside the difference
    for rnd in range(2):
        for name, cooling in (("cooled", True), ("power law", False)):
            r = rate(cooling, a.walkers, a.steps, a.warmup)
            print(json.dumps(dict(model=name, round=rnd, walkers=a.walkers, steps=a.steps, **r)),
                  flush=True)
