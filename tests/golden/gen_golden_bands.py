#!/opt/conda/bin/python3.9
"""Golden vectors for the confidence bands and ML model of naima's plots (plot.py:273-343,
396-501, 667-702): stub samplers with emcee-style object blob arrays (one (spectrum, scalar)
tuple per step and walker) fed to THE REFERENCE's _process_blob, _calc_CI, find_ML and _calc_ML
in the build container (same loader as gen_golden.py, plus a stand-in for emcee.autocorr so
that naima.plot imports):

    /opt/conda/bin/python3.9 tests/golden/gen_golden_bands.py

Writes tests/golden/bands.npz (blob histories + expected outputs; data only)."""
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
emcee = sys.modules.setdefault("emcee", types.ModuleType("emcee"))
autocorr = types.ModuleType("emcee.autocorr")


class AutocorrError(Exception):
    pass


def integrated_time(*a, **k):
    raise AutocorrError("not available")


autocorr.AutocorrError, autocorr.integrated_time = AutocorrError, integrated_time
emcee.autocorr = autocorr
sys.modules["emcee.autocorr"] = autocorr
for m in ("extern", "extern.validator", "utils", "model_utils", "radiative", "models", "core",
          "plot"):
    importlib.import_module("naima." + m)
warnings.simplefilter("ignore")
import astropy.units as u  # noqa: E402

import naima.plot as nplot  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(20261016)
FU, SU = u.Unit("1/(cm2 s eV)"), u.Unit("erg")


class Stub:
    """what the reference reads of an emcee sampler"""

    def __init__(self, chain, lp, spec, scal, energy):
        S, W = lp.shape
        self._chain, self._lp = chain, lp
        self._blobs = np.empty((S, W), dtype=object)
        for s in range(S):
            for w in range(W):
                self._blobs[s, w] = (spec[s, w] * FU, scal[s, w] * SU)
        self.data = {"energy": energy * u.TeV, "flux": np.ones(energy.size) * FU}

    def get_chain(self, flat=False):
        return self._chain.reshape(-1, self._chain.shape[-1]) if flat else self._chain

    def get_log_prob(self):
        return self._lp

    def get_blobs(self):
        return self._blobs


def history(S, W, m, kind):
    base = np.exp(rng.normal(-25.0, 1.5, size=(S, W, m)))  # lognormal columns
    if kind == "edge":
        base[:, :, 0] = 3.5e-12                                      # all equal
        base[:, :, 1] = np.round(base[:, :, 1] / base[:, :, 1].max() * 6) * 1e-12  # heavy ties
        base[:, :, 2] = np.where(rng.random((S, W)) < 0.4, 0.0, base[:, :, 2])     # exact zeros
        base[:, :, 3] = rng.normal(0.0, 1e-300, (S, W))              # tiny negatives (LUT lobes)
        nan = rng.random((S, W, m)) < 0.01
        nan[:, :, :4] = False
        base[nan] = np.nan                                            # a few NaNs
    return base


out = {}
cases = []
for name, (S, W, m, kind) in {"logn": (30, 24, 9, "plain"), "edge": (25, 32, 7, "edge")}.items():
    ndim = 3
    chain = rng.normal(size=(S, W, ndim)) * [0.3, 0.1, 0.05] + [1.0, 2.2, 0.7]
    lp = -0.5 * ((chain - [1.0, 2.2, 0.7]) ** 2).sum(-1) + rng.normal(0, 1e-3, (S, W))
    spec = history(S, W, m, kind)
    scal = np.exp(rng.normal(110.0, 0.5, (S, W)))
    energy = np.geomspace(0.3, 70.0, m)
    sp = Stub(chain, lp, spec, scal, energy)
    out[name + "__chain"], out[name + "__log_prob"] = chain, lp
    out[name + "__blob0"], out[name + "__blob1"], out[name + "__energy_TeV"] = spec, scal, energy
    for last in (False, True):
        tag = "%s__last%d" % (name, int(last))
        mx, model = nplot._process_blob(sp, 0, last_step=last)
        out[tag + "__pb0_x"] = mx.to(u.TeV).value
        # (the whole history is blob0 flattened over steps x walkers: checked, not stored again)
        want = spec[-1] if last else spec.reshape(-1, m)
        assert np.array_equal(model.to(FU).value, want, equal_nan=True)
        mx, model = nplot._process_blob(sp, 1, last_step=last)
        assert mx is None
        out[tag + "__pb1"] = model.to(SU).value
        for ci, confs in enumerate(([3, 1], [3, 1, 0.5], [2])):
            mx, CI = nplot._calc_CI(sp, 0, confs=list(confs), last_step=last)
            out["%s__ci%d" % (tag, ci)] = np.array([[lo.to(FU).value, hi.to(FU).value]
                                                    for lo, hi in CI])
    ML, MLp, MLerr, (mx, my) = nplot.find_ML(sp, 0)
    out[name + "__ML"], out[name + "__MLp"], out[name + "__MLerr"] = ML, MLp, np.array(MLerr)
    out[name + "__ML_x"], out[name + "__ML_model"] = mx.to(u.TeV).value, my.to(FU).value
    ML2, MLp2, MLerr2, (mx2, my2) = nplot._calc_ML(sp, 0)
    assert ML2 == ML and np.array_equal(my2.value, my.value)
    cases.append(name)
out["cases"] = np.array(cases)
out["confs"] = np.array(["3,1", "3,1,0.5", "2"])
np.savez_compressed(os.path.join(HERE, "bands.npz"), **out)
