"""A leptonic PeVatron behind a few kiloparsecs of Galactic photon fields: inverse Compton
emission on the CMB up to the PeV range, absorbed by pair production on the CMB and on the
far-infrared dust field along the line of sight, with the path length a fit parameter under a
normal prior (the distance estimate).  Above ~300 TeV the spectrum bends twice: at the
electrons' own cut-off and where the Galaxy becomes opaque (tau = 1 on the CMB near 1 PeV for
~7 kpc).  The transmission of every walker comes from the GPU (nh_pairabs_rows /
nh_pairabs_apply) inside the device-resident step loop.

    python examples/pevatron_absorbed.py [nwalkers] [nburn] [nrun]

Data: a seeded synthetic table made here from the known parameters P0 -- 1 TeV to 2.5 PeV,
12 % errors and Gaussian scatter.  Printed: the posterior of the intrinsic cut-off (of the
electrons) and of the absorbed cut-off, the photon energy at which the transmission has fallen
to 1/2 for each sample's path length."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u

P0 = np.array((33.3, 2.2, 3.3, 7.0))
LABELS = ["log10(norm)", "index", "log10(cutoff/TeV)", "path length [kpc]"]
FIELDS = ["CMB", "FIR"]
L_MEAN, L_SIGMA = 7.0, 1.0  # kpc: the prior on the path length
ABSORB = True


def AbsorbedPeVatron(pars, data):
    ECPL = naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                           10 ** pars[2] * u.TeV)
    IC = naima.InverseCompton(ECPL, seed_photon_fields=["CMB"], Eemin=100 * u.GeV,
                              Eemax=50 * u.PeV, nEed=40)
    flux = IC.flux(data, distance=3.0 * u.kpc)
    if not ABSORB:
        return flux
    # one path length per walker: a per-walker, per-energy factor from the GPU
    absorb = naima.PairAbsorptionModel(FIELDS, pars[3] * u.kpc)
    T = absorb.transmission(data)
    return flux * T, T


def lnprior(pars):
    return (naima.uniform_prior(pars[0], 25, 40) + naima.uniform_prior(pars[1], 1, 4)
            + naima.uniform_prior(pars[2], 1, 5) + naima.uniform_prior(pars[3], 0, 30)
            + naima.normal_prior(pars[3], L_MEAN, L_SIGMA))


def synthetic_data(seed=11):
    E = np.geomspace(1e12, 2.5e15, 20)
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    true = AbsorbedPeVatron(P0, make_data(raw))
    true = true[0] if ABSORB else true
    sed = (true * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    rng = np.random.default_rng(seed)
    raw["flux"] = sed * (1 + 0.12 * rng.standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.12 * sed
    return make_data(raw)


def absorbed_cutoff_TeV(lengths_kpc):
    """the lowest photon energy at which the transmission is 1/2 for each path length (inf where
    it never falls that far): the opacity of every sample at once on a fine grid, one host
    batch through the GPU"""
    E = np.geomspace(1e14, 1e17, 240)
    tau = naima.PairAbsorptionModel(FIELDS, lengths_kpc * u.kpc).opacity(E * u.eV)
    half = tau >= np.log(2.0)
    return np.where(half.any(axis=1), E[np.argmax(half, axis=1)], np.inf) * 1e-12


def run(nwalkers, nburn, nrun, seed=1):
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0 if ABSORB else P0[:3],
                                     labels=LABELS if ABSORB else LABELS[:3],
                                     model=AbsorbedPeVatron, prior=lnprior if ABSORB else (
                                         lambda p: naima.uniform_prior(p[0], 25, 40)
                                         + naima.uniform_prior(p[1], 1, 4)
                                         + naima.uniform_prior(p[2], 1, 5)),
                                     nwalkers=nwalkers, nburn=nburn, nrun=nrun, guess=False,
                                     seed=seed, verbose=False)
    return sampler, time.time() - t0


if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    nrun = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    sampler, dt = run(nwalkers, nburn, nrun)
    chain = sampler.get_chain()
    print("%d walkers x (%d + %d) steps in %.2f s; acceptance %.2f" % (
        nwalkers, nburn, nrun, dt, np.mean(sampler.acceptance_fraction)))
    print("device loop: %s" % bool(getattr(sampler, "device", False)))
    flat = chain[nrun // 2:].reshape(-1, chain.shape[-1])
    for lab, med, lo, hi, t in zip(LABELS, np.median(flat, 0),
                                   *np.percentile(flat, [16, 84], 0), P0):
        print("  %-20s %8.3f  (+%.3f -%.3f)   generated with %.3f" % (lab, med, hi - med,
                                                                       med - lo, t))
    intrinsic = 10 ** flat[:, 2]
    absorbed = absorbed_cutoff_TeV(flat[::max(1, len(flat) // 4096), 3])
    for name, v in (("intrinsic cut-off", intrinsic), ("absorbed cut-off", absorbed)):
        lo, med, hi = np.percentile(v, [16, 50, 84], method="nearest")
        print("%s [TeV]: %.0f (16th %.0f, 84th %.0f)" % (name, med, lo, hi))
    lo, med, hi = np.percentile(flat[:, 3], [16, 50, 84])
    print("path length [kpc]: %.2f (+%.2f -%.2f), prior %.1f +- %.1f, generated with %.1f" % (
        med, hi - med, med - lo, L_MEAN, L_SIGMA, P0[3]))
    T = np.asarray(sampler.get_blobs()[1], dtype=float)
    print("transmission at the highest energy: %.3f .. %.3f" % (T[..., -1].min(), T[..., -1].max()))
