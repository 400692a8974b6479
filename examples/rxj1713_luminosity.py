"""Posterior of band-integrated quantities in a fit: the RX J1713-like synchrotron +
inverse-Compton fit of examples/rxj1713_synic.py with two extra blobs, each one line of
ordinary naima in the model function,

    trapz_loglog(IC.flux(E, 0 * u.cm) * E, E).to("erg/s")           1-100 TeV IC luminosity
    trapz_loglog(SYN.flux(E, 1 * u.kpc) * E, E).to("erg/(cm2 s)")   2-10 keV energy flux

On device parameters ``trapz_loglog`` integrates the spectrum where it lies in HBM (one launch
per integral, nothing downloaded), so the fit stays on the device step loop and the two numbers
are kept per step and walker like We.

    python examples/rxj1713_luminosity.py [nwalkers] [nburn] [nrun]

Data: the synthetic X-ray + TeV table of BASELINE workload cfg3 (naima_amd/workloads.py)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd import workloads as W  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402
from naima_amd.utils import trapz_loglog  # noqa: E402

u = naima.u
E_TEV = np.logspace(0, 2, 30) * u.TeV
E_KEV = np.logspace(np.log10(2.0), 1, 20) * u.keV
P0 = np.array(W.WORKLOADS["cfg3"]["p0"], dtype=float)
LABELS = ["log10(norm)", "index", "log10(cutoff)", "B", "beta"]


def _components(pars):
    ECPL = naima.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                           10 ** pars[2] * u.TeV, beta=pars[4])
    IC = naima.InverseCompton(ECPL, seed_photon_fields=["CMB", "FIR", "NIR"], Eemin=100 * u.GeV)
    SYN = naima.Synchrotron(ECPL, B=pars[3] * u.uG)
    return IC, SYN


def ElectronSynIC(pars, data):
    """the model of examples/rxj1713_synic.py (blobs: the model, We)"""
    IC, SYN = _components(pars)
    model = IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)
    return model, IC.compute_We(Eemin=1 * u.TeV)


def ElectronSynICBands(pars, data):
    """... with the 1-100 TeV inverse-Compton luminosity and the 2-10 keV synchrotron energy
    flux as blobs 2 and 3"""
    IC, SYN = _components(pars)
    model = IC.flux(data, distance=1.0 * u.kpc) + SYN.flux(data, distance=1.0 * u.kpc)
    We = IC.compute_We(Eemin=1 * u.TeV)
    L_ic = trapz_loglog(IC.flux(E_TEV, 0 * u.cm) * E_TEV, E_TEV).to("erg/s")
    F_x = trapz_loglog(SYN.flux(E_KEV, 1.0 * u.kpc) * E_KEV, E_KEV).to("erg/(cm2 s)")
    return model, We, L_ic, F_x


def lnprior(pars):
    return (naima.uniform_prior(pars[1], -1, 5) + naima.uniform_prior(pars[3], 0, np.inf)
            + naima.uniform_prior(pars[4], 0.3, 3))


def synthetic_data():
    def flux_at_p0(E_eV):
        return ElectronSynIC(P0, {"energy": E_eV * u.eV})[0].to("1/(s cm2 eV)").value

    return make_data(W.build_data("cfg3", flux_at_p0))


if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    nrun = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS,
                                     model=ElectronSynICBands, prior=lnprior, nwalkers=nwalkers,
                                     nburn=nburn, nrun=nrun, prefit=True, seed=1, verbose=False)
    dt = time.time() - t0
    chain, blobs = sampler.get_chain(), sampler.get_blobs()
    print("chain", chain.shape, "blobs", [np.shape(b) for b in blobs])
    print("%d walkers x (%d + %d) steps in %.2f s; device loop: %s; acceptance %.2f" % (
        nwalkers, nburn, nrun, dt, sampler.device, np.mean(sampler.acceptance_fraction)))
    truth = ElectronSynICBands(P0, data)
    for name, j in (("L_IC(1-100 TeV)", 2), ("F_syn(2-10 keV)", 3)):
        v = np.asarray(blobs[j], dtype=float)[nrun // 2:].ravel()
        lo, med, hi = np.percentile(v, [16, 50, 84])
        print("  %-16s median %.4e  16%% %.4e  84%% %.4e %s   (at the generating parameters "
              "%.4e)" % (name, med, lo, hi, sampler.blob_units[j].name,
                         float(truth[j].to(sampler.blob_units[j]).value)))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rxj1713_luminosity_run")
    naima.save_run(out, sampler, clobber=True)
    back = naima.read_run(out)
    assert np.array_equal(np.asarray(back.get_blobs()[2], dtype=float),
                          np.asarray(blobs[2], dtype=float))
    naima.save_results_table(out, sampler, overwrite=True)
    print("saved and read back:", out + ".npz")
