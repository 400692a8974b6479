"""The resident loop's log-domain synchrotron items with a chunk count per energy (csrc/nh_syn2.h:
hs_s2_spread -- every lane of a slice's planned items carries a chunk, the longest ranges one
chunk more) against the per-launch kernel, which keeps one chunk count for all energies.

The number of live photon energies and the spread of their ranges follow from the magnetic field:
an energy E is live where E / Ec(gamma) <= 746 somewhere on the electron grid, Ec = 3 e hbar B
gamma^2 / (2 m_e c) (radiative.py:331-334), and its range starts at the first such node.  cfg3's
64 photon energies (36 X-ray points, 28 TeV points) on small ensembles:
  * one live energy (746 Ec at the grid's last node lies between the two lowest energies): the
    whole item is that energy's chunks, capped by the partial sums' room;
  * every energy live, the ranges very unequal (the TeV points' ranges are a fraction of the X-ray
    points'): 64 energies, one chunk each or two, the extra chunks on the long ranges;
  * none live: no synchrotron item at all, the component an exact zero;
  * the benchmark's field: 36 live energies, ranges of 170 ... 234 nodes (tests/test_item_lanes_host.py).
Resident loop == per-launch loop at 1e-10 on chain and blobs (the same tolerance as
tests/test_gpu_loops.py::test_resident_loop_equals_per_launch_loop)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

SEED = 20260929
EC_PER_GAUSS = 1.7366e-8          # eV: 3 e hbar / (2 m_e c), times B [G] gamma^2
GAMMA_MAX = 510e12 / 510998.95    # Synchrotron's default Eemax = 510 TeV


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def _field_for(E_eV):
    """B [uG] at which 746 Ec(gamma_max) = E_eV"""
    return E_eV / (746.0 * EC_PER_GAUSS * GAMMA_MAX ** 2) * 1e6


@pytest.mark.parametrize("split", ["1", "8"], ids=["one-workgroup-per-walker", "eight-per-walker"])
@pytest.mark.parametrize("case", ["one-live", "all-live-unequal", "none-live", "benchmark-field"])
def test_resident_equals_per_launch_over_the_field_range(na, monkeypatch, case, split):
    # (NH_HS_SPLIT: workgroups per walker at most -- 1 is the headline's shape, 8 what 32 walkers get)
    monkeypatch.setenv("NH_HS_SPLIT", split)
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    E = np.sort(np.asarray(raw["energy"], dtype=float)) * {"eV": 1.0, "keV": 1e3, "MeV": 1e6, "GeV": 1e9,
                                                           "TeV": 1e12}[raw["energy_unit"]]
    assert E.size == 64
    B = {"one-live": _field_for(np.sqrt(E[0] * E[1])),       # (E[0] live, E[1] not: the ball below keeps it so)
         "all-live-unequal": _field_for(E[-1] * 30.0),
         "none-live": _field_for(E[0] / 30.0),
         "benchmark-field": p0[3]}[case]
    nw, nd = 32, p0.size
    start = np.array(p0, dtype=float)
    start[3] = B
    rng = np.random.default_rng(SEED)
    pos = start * (1 + 0.01 * rng.normal(size=(nw, nd)))
    if case == "one-live":
        # (the two lowest energies are 9 % apart: a 0.3 % ball in B starts every walker between them)
        assert E[1] / E[0] > 1.05
        pos[:, 3] = B * (1 + 0.003 * rng.normal(size=nw))
    kw = dict(args=[data, model, prior], seed=SEED, naima_style=True, store_blobs=True, nan_policy="reject")
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("NAIMA_AMD_RESIDENT", mode)
        d = EnsembleSampler(nw, nd, na.lnprob, device=True, **kw)
        with np.errstate(all="ignore"):
            st = d.run_mcmc(pos, 4)
            st = d.run_mcmc(st, 36)
        assert (d._dev.resident_launches > 0) == (mode == "1"), getattr(d._dev, "resident_reason", "")
        if mode == "1":
            info = d._dev.resident_info
            assert info["syn_log_domain"] and info["workgroups_per_walker"] == int(split), info
        runs[mode] = (d.get_chain(), d.get_log_prob(), [np.asarray(b, dtype=float) for b in d.get_blobs()],
                      d.acceptance_fraction)
    a, b = runs["0"], runs["1"]
    assert a[0].shape == (40, nw, nd)
    assert_allclose(b[0], a[0], rtol=1e-10)
    fin = np.isfinite(a[1])
    assert np.array_equal(fin, np.isfinite(b[1]))
    assert_allclose(b[1][fin], a[1][fin], rtol=1e-9)
    for x, y in zip(b[2], a[2]):
        assert x.shape == y.shape
        assert_allclose(x, y, rtol=1e-10, atol=1e-300, equal_nan=True)
    assert_allclose(b[3], a[3])
    spec = a[2][0]
    print("%s: B = %.3g uG, model spectra finite: %.2f, positive: %.2f" %
          (case, B, np.isfinite(spec).mean(), (spec > 0).mean()))
