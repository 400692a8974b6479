"""A compact one-zone synchrotron + synchrotron-self-Compton source (a blazar zone, a radio
supernova, a microquasar knot) whose radio points lie below the self-absorption turnover: the
source radius R is a fit parameter, and it enters three times -- as the optical depth of the
synchrotron spectrum (nu^(5/2) below the turnover), as the volume that turns the escaping
synchrotron luminosity into the SSC seed photon density, and through that as the level of the
inverse-Compton component.  The absorbed synchrotron spectrum is both the radio-to-X-ray
component and the seed field of the SSC emission.  The escape fraction of every walker comes from
the GPU (nh_syn_absorption / nh_ssa_apply) inside the device-resident step loop, which runs this
model piecewise (the one-launch half-step does not know the two launches).

    python examples/blob_ssc.py [nwalkers] [nburn] [nrun]

Data: a seeded synthetic table made here from the known parameters P0 -- 2.4 GHz to 10 GeV,
10 % errors and Gaussian scatter.  R is walked in log10 under a normal prior (a size from the
variability time scale), B under a uniform one."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u

P0 = np.array((42.0, 2.2, 1.0, 0.3, 16.0))
LABELS = ["log10(norm)", "index", "log10(cutoff/GeV)", "B [G]", "log10(R/cm)"]
LOGR_MEAN, LOGR_SIGMA = 16.0, 0.3  # the prior on log10(R / cm)
C_CGS = 29979245800.0
ESY = np.logspace(-6, 4, 60) * u.eV  # the seed photon grid of the SSC component
EOPTS = {"Eemin": 5 * u.MeV, "Eemax": 1 * u.TeV, "nEed": 50}
DISTANCE = 100 * u.Mpc
ABSORB = True


def _rows(x):
    """a per-walker factor of an (N, n_e) host batch: walkers on axis 0"""
    return x[:, None] if isinstance(x, np.ndarray) and x.ndim == 1 else x


def BlobSSC(pars, data):
    ECPL = naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 1 * u.GeV, pars[1],
                                           10 ** pars[2] * u.GeV)
    SYN = naima.Synchrotron(ECPL, B=pars[3] * u.G, **EOPTS)
    R = 10 ** pars[4] * u.cm if ABSORB else None
    # photon density of the synchrotron emission that escapes a homogeneous sphere of radius R
    # (2.24: the mean over its volume, as in naima's examples/CrabNebula_SynSSC.py)
    Lsy = SYN.flux(ESY, distance=0 * u.cm, radius=R)
    phn_sy = Lsy * _rows(10 ** (-2 * pars[4])) * (2.24 / (4 * np.pi * C_CGS)) / (u.cm ** 3 / u.s)
    IC = naima.InverseCompton(ECPL, seed_photon_fields=[["SSC", ESY, phn_sy]], **EOPTS)
    return IC.flux(data, distance=DISTANCE) + SYN.flux(data, distance=DISTANCE, radius=R)


def lnprior(pars):
    return (naima.uniform_prior(pars[0], 35, 50) + naima.uniform_prior(pars[1], 1, 4)
            + naima.uniform_prior(pars[2], -1, 3) + naima.uniform_prior(pars[3], 0.01, 10)
            + naima.uniform_prior(pars[4], 14, 18)
            + naima.normal_prior(pars[4], LOGR_MEAN, LOGR_SIGMA))


def synthetic_data(seed=11):
    E = np.concatenate([np.geomspace(1e-5, 1e-3, 8), np.geomspace(3e-3, 1e4, 12),
                        np.geomspace(1e6, 1e10, 8)])
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    true = BlobSSC(P0, make_data(raw))
    sed = (true * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    rng = np.random.default_rng(seed)
    raw["flux"] = sed * (1 + 0.10 * rng.standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.10 * sed
    return make_data(raw)


def turnover_GHz(B_G, log10_R, pars):
    """the frequency at which tau = 1 along a diameter, for each sample: the opacity of every
    sample at once on a fine grid, one host batch through the GPU"""
    E = np.geomspace(1e-6, 1e-1, 200)
    ECPL = naima.ExponentialCutoffPowerLaw(10 ** pars[:, 0] / u.eV, 1 * u.GeV, pars[:, 1],
                                           10 ** pars[:, 2] * u.GeV)
    SYN = naima.Synchrotron(ECPL, B=B_G * u.G, **EOPTS)
    tau = SYN.self_absorption(10 ** log10_R * u.cm).opacity(E * u.eV)
    thin = tau <= 1.0
    return np.where(thin.any(axis=1), E[np.argmax(thin, axis=1)], np.nan) / 4.135667696e-15 * 1e-9


def run(nwalkers, nburn, nrun, seed=1):
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS, model=BlobSSC,
                                     prior=lnprior, nwalkers=nwalkers, nburn=nburn, nrun=nrun,
                                     guess=False, prefit=False, seed=seed, verbose=False)
    return sampler, time.time() - t0


if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    nrun = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    sampler, dt = run(nwalkers, nburn, nrun)
    chain = sampler.get_chain()
    print("%d walkers x (%d + %d) steps in %.2f s (%.0f walker-steps/s); acceptance %.2f" % (
        nwalkers, nburn, nrun, dt, nwalkers * (nburn + nrun) / dt,
        np.mean(sampler.acceptance_fraction)))
    print("device loop: %s" % bool(getattr(sampler, "device", False)))
    dev = getattr(sampler, "_dev", None)
    if dev is not None and dev._plan is not None:
        print("launches of a step: %s" % list(dev._plan.calls))
    flat = chain[nrun // 2:].reshape(-1, chain.shape[-1])
    for lab, med, lo, hi, t in zip(LABELS, np.median(flat, 0),
                                   *np.percentile(flat, [16, 84], 0), P0):
        print("  %-20s %8.3f  (+%.3f -%.3f)   generated with %.3f" % (lab, med, hi - med,
                                                                       med - lo, t))
    some = flat[::max(1, len(flat) // 1024)]
    nu = turnover_GHz(some[:, 3], some[:, 4], some)
    lo, med, hi = np.nanpercentile(nu, [16, 50, 84])
    print("self-absorption turnover (tau = 1): %.1f GHz (16th %.1f, 84th %.1f)" % (med, lo, hi))
