"""Walker-steps per second of the free-redshift Syn+IC model (examples/absorbed_synic.py) and of
the same model without absorption, both on the per-launch fused device loop (nh_step_front and
captured graphs; NAIMA_AMD_RESIDENT=0 NAIMA_AMD_MEGA=0, which the absorbed model takes anyway:
the one-launch half-step does not know nh_ebl_apply).  Prints one JSON line per model.

    python scripts/ebl_rate.py [--walkers 512] [--steps 200] [--warmup 20]
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
from absorbed_synic import P0, ElectronEblAbsorbedSynIC, lnprior, synthetic_data  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402

u = naima.u


def ElectronSynIC(pars, data):
    """ElectronEblAbsorbedSynIC without the absorption (pars[5] unused)"""
    BPL = naima.BrokenPowerLaw(10 ** pars[0] / u.eV, 1.0 * u.TeV, (10 ** pars[1]) * u.TeV,
                               pars[2], pars[3])
    IC = naima.InverseCompton(BPL, seed_photon_fields=["CMB"], Eemin=10 * u.GeV)
    SYN = naima.Synchrotron(BPL, B=pars[4] * u.uG)
    model = IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)
    return model, IC.compute_We(Eemin=1 * u.TeV)


def rate(model, data, nw, steps, warmup):
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
    return dict(walker_steps_per_s=nw * steps / dt, seconds=dt, fused=bool(d.fused),
                mega=bool(d.mega), launches_per_half_step=list(d._plan.calls),
                acceptance=float(np.mean(s.acceptance_fraction)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    data = synthetic_data()
    for name, model in (("free_z_absorbed", ElectronEblAbsorbedSynIC), ("unabsorbed", ElectronSynIC)):
        r = rate(model, data, a.walkers, a.steps, a.warmup)
        print(json.dumps(dict(model=name, walkers=a.walkers, steps=a.steps, **r)), flush=True)
