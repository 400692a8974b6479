"""A pulsar wind nebula whose spectral break is not a free parameter: electrons injected as a
power law at a constant rate cool by synchrotron and inverse-Compton losses for the age of the
nebula, and the population that is left radiates synchrotron X-rays and inverse-Compton gamma
rays.  The magnetic field and the age are the fit parameters; the break energy, where the
cooling time equals the age, follows from them.  Every walker's cooling solve comes from the GPU
(nh_cooled_electrons / nh_cooled_weights) inside the device-resident step loop.

    python examples/pwn_cooled.py [nwalkers] [nburn] [nrun]

Data: a seeded synthetic table made here from the model itself at the known parameters
(B, age, injection index, injection rate) -- radio to X-rays and 1 GeV to 100 TeV, 12 % errors and
Gaussian scatter.  Printed: the posteriors of B and the age and of the derived break energy."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u

ALPHA, L_INJ = 2.2, 3e35  # injection index, injection rate at 1 TeV [1/(eV s)]
P0 = np.array((40.0, 3.5))
LABELS = ["B [uG]", "log10(age/yr)"]
FIELDS = ["CMB", "FIR"]
DISTANCE = 2.0 * u.kpc
COOLING = True


def cooled(B_uG, log_age):
    inj = naima.PowerLaw(L_INJ / u.eV / u.s, 1 * u.TeV, ALPHA)
    return naima.CooledElectrons(inj, B_uG * u.uG, 10 ** log_age * u.yr, FIELDS, n_per_decade=40)


def CooledPWN(pars, data):
    if COOLING:
        electrons = cooled(pars[0], pars[1])
    else:  # (the timing comparison of scripts/cooling_rate.py: the same emission, no solve)
        electrons = naima.PowerLaw(10 ** pars[1] * 1e43 / u.eV, 1 * u.TeV, ALPHA + 1)
    SYN = naima.Synchrotron(electrons, B=pars[0] * u.uG, Eemax=400 * u.TeV, nEed=40)
    IC = naima.InverseCompton(electrons, seed_photon_fields=FIELDS, Eemax=400 * u.TeV, nEed=40)
    return SYN.flux(data, distance=DISTANCE) + IC.flux(data, distance=DISTANCE)


def lnprior(pars):
    return naima.uniform_prior(pars[0], 1, 500) + naima.uniform_prior(pars[1], 1, 7)


def synthetic_data(seed=11):
    E = np.concatenate([np.geomspace(1e-5, 1e4, 14), np.geomspace(1e9, 1e14, 14)])
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    true = CooledPWN(P0, make_data(raw))
    sed = (true * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    rng = np.random.default_rng(seed)
    raw["flux"] = sed * (1 + 0.12 * rng.standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.12 * sed
    return make_data(raw)


def run(nwalkers, nburn, nrun, seed=1):
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS, model=CooledPWN,
                                     prior=lnprior, nwalkers=nwalkers, nburn=nburn, nrun=nrun,
                                     guess=False, seed=seed, verbose=False)
    return sampler, time.time() - t0


if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    nrun = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    sampler, dt = run(nwalkers, nburn, nrun)
    chain = sampler.get_chain()
    print("%d walkers x (%d + %d) steps in %.2f s; acceptance %.2f" % (
        nwalkers, nburn, nrun, dt, np.mean(sampler.acceptance_fraction)))
    print("device loop: %s" % bool(getattr(sampler, "device", False)))
    flat = chain[nrun // 2:].reshape(-1, chain.shape[-1])
    for lab, med, lo, hi, t in zip(LABELS, np.median(flat, 0),
                                   *np.percentile(flat, [16, 84], 0), P0):
        print("  %-16s %8.3f  (+%.3f -%.3f)   generated with %.3f" % (lab, med, hi - med,
                                                                   med - lo, t))
    # the derived break energy of every sample: one host batch through the same model
    sub = flat[::max(1, len(flat) // 2048)]
    eb = cooled(sub[:, 0], sub[:, 1]).break_energy().to("TeV").value
    lo, med, hi = np.nanpercentile(eb, [16, 50, 84])
    true = float(cooled(P0[0], P0[1]).break_energy().to("TeV").value)
    print("break energy [TeV]: %.3f (+%.3f -%.3f), generated with %.3f" % (
        med, hi - med, med - lo, true))
