"""The synchrotron emission of a hadronic PeVatron's secondary electrons beside the gamma rays
of the same protons.  pp collisions make neutral pions (gamma rays, PionDecayKelner06) and charged
pions, whose decay leaves electrons and positrons (SecondaryLeptonsKelner06, product="electron").
That is an injection RATE; cooled for the age of the source in its magnetic field and photon
fields (CooledElectrons) it becomes a population, whose synchrotron emission is what X-ray upper
limits constrain in hadronic models of PeVatrons.  The protons are those examples/
pevatron_neutrinos.py generates its data with; nothing is fitted here.

    python examples/pevatron_secondaries.py

Printed: E^2 dN/dE of the pi0 gamma rays and of the secondaries' synchrotron emission for a
few magnetic fields (one host batch through the GPU), and the break energy of each population."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naima_amd as naima  # noqa: E402
from pevatron_neutrinos import DISTANCE, NH, P0, protons  # noqa: E402

u = naima.u

AGE = 1e4 * u.yr
B_UG = np.array([3.0, 10.0, 30.0, 100.0])
FIELDS = ["CMB", "FIR"]


def secondaries_synchrotron(B_uG, age=AGE):
    """(Synchrotron of the cooled secondary electrons, their CooledElectrons), one walker per
    magnetic field"""
    gamma = naima.PionDecayKelner06(protons(P0), nh=NH)
    rate = gamma.secondaries("electron")  # 1/(s eV) at the source: an injection rate
    electrons = naima.CooledElectrons(rate, B_uG * u.uG, age, FIELDS, Emin=1 * u.GeV,
                                      Emax=2 * u.PeV, n_per_decade=40)
    return naima.Synchrotron(electrons, B=B_uG * u.uG, Eemax=2 * u.PeV, nEed=40), electrons


if __name__ == "__main__":
    gamma = naima.PionDecayKelner06(protons(P0), nh=NH)
    Eg = np.geomspace(1e11, 1e15, 9) * u.eV
    sed = gamma.sed(Eg, distance=DISTANCE).to("erg/(cm2 s)").value
    print("pi0 gamma rays, E^2 dN/dE [erg/(cm2 s)]:")
    for e, v in zip(Eg.to("TeV").value, sed):
        print("  %10.2f TeV  %.3e" % (e, v))
    syn, electrons = secondaries_synchrotron(B_UG)
    Ex = np.geomspace(1e-1, 1e5, 7) * u.eV
    sx = syn.sed(Ex, distance=DISTANCE).to("erg/(cm2 s)").value
    eb = electrons.break_energy().to("TeV").value
    We = syn.compute_We(Eemin=1 * u.GeV).to("erg").value
    print("synchrotron of the cooled secondaries after %.0e yr, E^2 dN/dE [erg/(cm2 s)]:"
          % AGE.to("yr").value)
    print("  %12s" % "E [eV]" + "".join("  B = %5.0f uG" % b for b in B_UG))
    for e, row in zip(Ex.to("eV").value, sx.T):
        print("  %12.3g" % e + "".join("  %12.3e" % v for v in row))
    for b, e_b, w in zip(B_UG, eb, We):
        print("B = %5.0f uG: break energy %.3g TeV, energy in secondaries above 1 GeV %.3e erg"
              % (b, e_b, w))
