#!/opt/conda/bin/python3.9
"""Golden vectors for the likelihood (core.py:64-94) where units.npz is silent: asymmetric
errors whose larger side alternates, upper limits spread through the table, a DISTINCT
confidence level per point (so the quirk of core.py:89-92, cl indexed by the number of violated
limits, is pinned to a value) and models that violate 0, 1, 2, 3 and 4 limits.  Produced by
running THE REFERENCE in the build container (same loader as gen_golden.py):

    /opt/conda/bin/python3.9 tests/golden/gen_golden_lnprob.py

Writes tests/golden/lnprob.npz (inputs + expected outputs; data only)."""
import importlib
import os
import sys
import types
import warnings

import numpy as np

for n, f in (("asscalar", lambda a: a.item()), ("alen", len), ("rank", np.ndim)):
    if not hasattr(np, n):
        setattr(np, n, f)
SRC = "/root/reference/src/naima"
pkg = types.ModuleType("naima")
pkg.__path__ = [SRC]
pkg.__file__ = SRC + "/__init__.py"
pkg.__package__ = "naima"
sys.modules["naima"] = pkg
sys.modules.setdefault("emcee", types.ModuleType("emcee"))
for m in ("extern", "extern.validator", "utils", "model_utils", "radiative", "models", "core"):
    importlib.import_module("naima." + m)
warnings.simplefilter("ignore")
import astropy.units as u  # noqa: E402

import naima.core as ncore  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(20261015)
out = {}

n = 30
en = np.geomspace(0.4, 80.0, n)  # TeV
true = 2e-11 * en ** -2.4
flux = true * (1 + 0.2 * rng.standard_normal(n))
lo = np.where(np.arange(n) % 2 == 0, 0.08, 0.25) * true   # the larger side alternates
hi = np.where(np.arange(n) % 2 == 0, 0.25, 0.08) * true
ul = np.zeros(n, bool)
uls = np.array([2, 9, 15, 22, 29])
ul[uls] = True
flux[uls] = 1.5 * true[uls]
lo[uls] = hi[uls] = 0.0
cl = 0.5 + 0.013 * np.arange(n)
fu = u.Unit("1/(cm2 s TeV)")
d = dict(energy=en * u.TeV, flux=flux * fu, flux_error_lo=lo * fu, flux_error_hi=hi * fu,
         ul=ul, cl=cl)
# models scattered around the data; the first k upper limits (in a shuffled order) violated
models, nviol = [], []
order = rng.permutation(uls)
for k in (0, 1, 2, 3, 4, 2, 1, 3):
    m = true * (1 + 0.3 * rng.standard_normal(n))
    m[uls] = 0.5 * flux[uls]
    m[order[:k]] = 1.3 * flux[order[:k]]
    models.append(m)
    nviol.append(k)
out["energy_TeV"], out["flux"], out["flux_error_lo"], out["flux_error_hi"] = en, flux, lo, hi
out["ul"], out["cl"] = ul, cl
out["models"], out["nviol"] = np.array(models), np.array(nviol)
out["lnprobmodel"] = np.array([float(ncore.lnprobmodel(m * fu, d)) for m in models])
np.savez_compressed(os.path.join(HERE, "lnprob.npz"), **out)
