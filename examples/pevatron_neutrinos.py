"""The neutrinos of a hadronic PeVatron: the fit of examples/pevatron_absorbed.py with protons in
place of electrons -- gamma rays of pp collisions (PionDecayKelner06) absorbed by pair production
on the CMB and the far-infrared dust field, the path length a fit parameter under the same normal
prior -- and, as a blob of every sample, the neutrino flux the same protons predict
(SecondaryLeptonsKelner06, Kelner, Aharonian & Bugayov 2006).  Neutrinos are not absorbed, so the
blob is the unattenuated all-flavour spectrum at a handful of energies; after averaged
oscillations each flavour arrives with about a third of it, which is what a muon-neutrino
telescope (IceCube, KM3NeT, Baikal-GVD) is compared with.  The chain and the blob stay in HBM.

    python examples/pevatron_neutrinos.py [nwalkers] [nburn] [nrun]

Data: a seeded synthetic table made here from the known parameters P0 -- 1 TeV to 2.5 PeV,
12 % errors and Gaussian scatter.  Printed: the posterior of the parameters, and the median and
68 % band of E^2 Phi of nu_mu + anti-nu_mu at Earth at 100 TeV beside the value of P0."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402
from pevatron_absorbed import FIELDS, L_MEAN, L_SIGMA, lnprior  # noqa: E402

u = naima.u

P0 = np.array((36.0, 2.1, 3.5, 7.0))
LABELS = ["log10(norm)", "index", "log10(cutoff/TeV)", "path length [kpc]"]
DISTANCE = 3.0 * u.kpc
NH = 10 / u.cm ** 3
NU_E = np.array([1e12, 1e13, 1e14, 3e14, 1e15]) * u.eV  # the blob's energies; 100 TeV is [2]


def protons(pars):
    return naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                           10 ** pars[2] * u.TeV)


def HadronicPeVatron(pars, data):
    gamma = naima.PionDecayKelner06(protons(pars), nh=NH)
    T = naima.PairAbsorptionModel(FIELDS, pars[3] * u.kpc).transmission(data)
    nu = gamma.secondaries("nu_all").flux(NU_E, distance=DISTANCE)
    return gamma.flux(data, distance=DISTANCE) * T, nu


def synthetic_data(seed=11):
    E = np.geomspace(1e12, 2.5e15, 20)
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    true = HadronicPeVatron(P0, make_data(raw))[0]
    sed = (true * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    rng = np.random.default_rng(seed)
    raw["flux"] = sed * (1 + 0.12 * rng.standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.12 * sed
    return make_data(raw)


def numu_at_earth(nu_all):
    """E^2 Phi [TeV / (cm2 s)] of nu_mu + anti-nu_mu at Earth from the all-flavour flux
    [1/(s cm2 eV)] at NU_E: a third of it after averaged oscillations"""
    E = NU_E.to("eV").value
    return np.asarray(nu_all, dtype=float) / 3.0 * E ** 2 * 1e-12


def run(nwalkers, nburn, nrun, seed=1):
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS,
                                     model=HadronicPeVatron, prior=lnprior, nwalkers=nwalkers,
                                     nburn=nburn, nrun=nrun, guess=False, seed=seed,
                                     verbose=False)
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
    print("path length prior: %.1f +- %.1f kpc" % (L_MEAN, L_SIGMA))
    nu = numu_at_earth(sampler.get_blobs()[1])[nrun // 2:].reshape(-1, NU_E.size)
    true = numu_at_earth(HadronicPeVatron(P0, synthetic_data())[1].to("1/(s cm2 eV)").value)
    lo, med, hi = np.percentile(nu[:, 2], [16, 50, 84])
    print("E^2 Phi(nu_mu + anti-nu_mu) at Earth at 100 TeV: %.3e TeV/(cm2 s) "
          "(68 %%: %.3e .. %.3e), generated with %.3e" % (med, lo, hi, true[2]))
    for e, col, t in zip(NU_E.to("TeV").value, nu.T, true):
        print("  %7.0f TeV: median %.3e  (16th %.3e, 84th %.3e)  generated with %.3e" % (
            e, np.median(col), *np.percentile(col, [16, 84]), t))
