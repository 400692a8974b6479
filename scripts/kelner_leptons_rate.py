"""Device time of nh_pp_leptons_kelner06 (neutrinos and secondary electrons of pp collisions)
beside nh_pion_kelner06 (the gamma rays of the same collisions) at the same shape: device events
around `reps` launches, median of five rounds, one JSON line per measurement.

The energies are log-spaced from 1 GeV to 1 PeV, a third of them below Etrans = 0.1 TeV, so both
calls also form the two integrals at Etrans.  The lepton kernel walks one set of panels per
energy and accumulates two (full branch) or up to three (delta branch) components on it, the
gamma-ray kernel one.

    python scripts/kelner_leptons_rate.py [--walkers 512] [--energies 32] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import naima_amd as naima  # noqa: E402
from naima_amd import _lib  # noqa: E402

u = naima.u
PRODUCTS = naima.SecondaryLeptonsKelner06.products


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


def main(nw, nE, reps):
    ctx = _lib.get_context()
    rng = np.random.default_rng(1)
    pd = naima.ExponentialCutoffBrokenPowerLaw(
        10 ** rng.uniform(34, 36, nw) / u.eV, 1 * u.TeV, 10 ** rng.uniform(-1, 1, nw) * u.TeV,
        rng.uniform(1.8, 2.2, nw), rng.uniform(2.3, 3.0, nw), 10 ** rng.uniform(1, 3, nw) * u.TeV)
    rows = pd.device_rows(ctx, nw, amplitude_to=u.Unit("1/eV"))
    kind = _lib.PD_KIND[pd.kind]
    E = ctx.array(np.geomspace(1e9, 1e15, nE))
    out, nhat, nhat3 = ctx.empty((nw, nE)), ctx.empty((nw,)), ctx.empty((nw, 3))
    r = timed(ctx, lambda: ctx.call("nh_pion_kelner06", kind, rows, nw, E, nE, 1e11, 1, out, nE,
                                    nhat, None), reps)
    base = r["us_median"]
    print(json.dumps(dict(what="nh_pion_kelner06", walkers=nw, energies=nE,
                          integrals_per_s=nw * (nE + 2) / (base * 1e-6), **r)), flush=True)
    for k, product in enumerate(PRODUCTS):
        r = timed(ctx, lambda: ctx.call("nh_pp_leptons_kelner06", kind, rows, nw, E, nE, 1e11, 1,
                                        k, out, nE, nhat3), reps)
        print(json.dumps(dict(what="nh_pp_leptons_kelner06 " + product, walkers=nw, energies=nE,
                              tasks_per_s=nw * (nE + 2) / (r["us_median"] * 1e-6),
                              over_gamma=r["us_median"] / base, **r)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--energies", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    main(a.walkers, a.energies, a.reps)
