"""Synchrotron + EBL-absorbed inverse Compton with the source redshift a free parameter: the
reference's examples/absorbed_SynIC.py (ElectronEblAbsorbedSynIC) fitted with naima_amd.  The
absorption cutoff of the GeV-TeV points constrains z; the transmission at each walker's
redshift is one gathered row of a table of every tabulated redshift at the data's energies,
made on the GPU (nh_ebl_table / nh_ebl_apply), inside the device-resident step loop.

    python examples/absorbed_synic.py [nwalkers] [nburn] [nrun]

Data: a seeded synthetic table made here from the known parameters P0 -- X-ray points and
10 GeV - 20 TeV points with 10 % errors and Gaussian scatter.  The reference's
InteractiveModelFitter call is left out."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from naima_amd.datatable import make_data  # noqa: E402

u = naima.u

P0 = np.array((31.0, 1.0, 0.35, 1.5, 2.3, 0.06))  # the reference's p0
LABELS = ["log10(norm)", "log10(Energy_Break)", "index1", "index2", "B", "redshift"]


def ElectronEblAbsorbedSynIC(pars, data):
    amplitude = 10 ** pars[0] / u.eV
    e_break = (10 ** pars[1]) * u.TeV
    alpha1 = pars[2]
    alpha2 = pars[3]
    B = pars[4] * u.uG

    # one redshift per walker: a per-walker factor from the GPU
    redshift = pars[5] * u.dimensionless_unscaled
    EBL_transmitance = naima.EblAbsorptionModel(redshift, "Dominguez")

    BPL = naima.BrokenPowerLaw(amplitude, 1.0 * u.TeV, e_break, alpha1, alpha2)
    IC = naima.InverseCompton(BPL, seed_photon_fields=["CMB"], Eemin=10 * u.GeV)
    SYN = naima.Synchrotron(BPL, B=B)

    model = EBL_transmitance.transmission(data) * IC.flux(data, distance=1.0 * u.kpc) + \
        SYN.flux(data, distance=1.0 * u.kpc)
    return model, IC.compute_We(Eemin=1 * u.TeV)


def lnprior(pars):
    # (bounded normalisation and break: naima's 10 % ball spreads log10(norm) by decades, and
    # a flux that overflows makes a NaN log-probability)
    return (naima.uniform_prior(pars[0], 25, 40) + naima.uniform_prior(pars[1], -2, 3)
            + naima.uniform_prior(pars[2], -1, 5) + naima.uniform_prior(pars[3], -1, 5)
            + naima.uniform_prior(pars[4], 0, np.inf) + naima.uniform_prior(pars[5], 0, np.inf))


def synthetic_data(seed=7):
    E = np.concatenate([np.geomspace(0.5e3, 1e4, 8), np.geomspace(1e10, 2e13, 16)])
    raw = dict(energy=E, energy_unit="eV", flux=np.ones_like(E), flux_error_lo=np.ones_like(E),
               flux_error_hi=np.ones_like(E), ul=np.zeros(E.size, dtype=bool), cl=0.9,
               flux_unit="erg/(cm2 s)")
    true = ElectronEblAbsorbedSynIC(P0, make_data(raw))[0]
    sed = (true * (E * u.eV) ** 2).to("erg/(cm2 s)").value
    rng = np.random.default_rng(seed)
    raw["flux"] = sed * (1 + 0.1 * rng.standard_normal(E.size))
    raw["flux_error_lo"] = raw["flux_error_hi"] = 0.1 * sed
    return make_data(raw)


if __name__ == "__main__":
    nwalkers = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    nburn = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    nrun = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    data = synthetic_data()
    t0 = time.time()
    sampler, pos = naima.run_sampler(data_table=data, p0=P0, labels=LABELS,
                                     model=ElectronEblAbsorbedSynIC, prior=lnprior,
                                     nwalkers=nwalkers, nburn=nburn, nrun=nrun, guess=False,
                                     seed=1, verbose=False)
    dt = time.time() - t0
    chain = sampler.get_chain()
    print("%d walkers x (%d + %d) steps in %.2f s; acceptance %.2f" % (
        nwalkers, nburn, nrun, dt, np.mean(sampler.acceptance_fraction)))
    flat = chain[nrun // 2:].reshape(-1, chain.shape[-1])
    for lab, med, lo, hi, t in zip(LABELS, np.median(flat, 0),
                                   *np.percentile(flat, [16, 84], 0), P0):
        print("  %-20s %8.3f  (+%.3f -%.3f)   generated with %.3f" % (lab, med, hi - med,
                                                                       med - lo, t))
    z1, z99 = np.percentile(flat[:, 5], [1, 99])
    print("z percentiles (1st, 99th) and injected: %.4f %.4f %.4f" % (z1, z99, P0[5]))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "absorbed_synic_run")
    naima.save_run(out, sampler, clobber=True)
    back = naima.read_run(out)
    assert np.array_equal(back.get_chain(), chain)
    print("saved and read back:", out + ".npz")
