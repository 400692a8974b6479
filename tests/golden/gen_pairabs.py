"""Writes tests/golden/pairabs.npz: pair-production opacities from their definitions
(tests/pairabs_cases.py), evaluated with mpmath at 30 digits and rounded to doubles.

    python tests/golden/gen_pairabs.py

On the grid ``eta`` (pairabs_cases.eta_grid), in units of sigma_T:
    iso       int x^2/(e^x - 1) sbar(eta x) dx             thermal, isotropic (a double integral)
    ang30/90/180  mu int x^2/(e^x - 1) sigma(eta x mu/2) dx    thermal at theta
    mono      sbar(eta)                                    monochromatic, eta = E E0 / m^2
    sigma_peak_s, sigma_peak  where sigma / sigma_T is largest, and that value
A value below the smallest double is stored as 0."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]


def main():
    import mpmath as mp

    import pairabs_cases as PC
    mp.mp.dps = 30
    eta = PC.eta_grid()
    out = dict(eta=eta)
    out["iso"] = np.array([float(PC.iso_mp(mp.mpf(float(e)))) for e in eta])
    for deg in PC.ANGLES_DEG:
        mu = PC.mu_of_deg_mp(deg)
        out["ang%d" % deg] = np.array([float(PC.ang_mp(mp.mpf(float(e)), mu)) for e in eta])
    out["mono"] = np.array([float(PC.sigma_bar_mp(mp.mpf(float(e)))) for e in eta])
    s_peak = mp.findroot(lambda s: mp.diff(PC.sigma_mp, s), 2.0)
    out["sigma_peak_s"] = np.array(float(s_peak))
    out["sigma_peak"] = np.array(float(PC.sigma_mp(s_peak)))
    np.savez(os.path.join(HERE, "pairabs.npz"), **out)
    for k, v in out.items():
        print(k, np.asarray(v).ravel()[:3], "...", np.asarray(v).ravel()[-2:])


if __name__ == "__main__":
    main()
