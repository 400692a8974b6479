"""What the reference's arithmetic makes of scalars outside their physical domain, pinned on the
oracle (no GPU): tests/domain_cases.py is the table test_gpu_domain.py holds the kernels to, and
this file holds that table to the reference's behaviour, read from its source:

  theta     1 - cos(theta) for an angle of any sign (radiative.py:597): theta and -theta give
            identical bits, 2 pi - theta the same to rounding, theta = 0 NaN at every energy;
  T         T < 0 NaN at every energy, isotropic or not; T = 0 passes validate_scalar's
            "positive" (validator.py:33-35), uf = u / (ar T^4) is array arithmetic
            (radiative.py:666-667: a division warning and inf) and the row is NaN -- the oracle's
            ic_seed_spectrum follows those lines, it used to raise ZeroDivisionError;
  B         B < 0 and B = 0 NaN at every energy of the table's cases;
  limits    int(nEed * decades) (radiative.py:152-154; protons 1002-1009): inverted limits give
            10 nodes, a descending grid, a finite spectrum and We of the opposite sign; equal
            limits 10 equal nodes and an exact 0; a negative limit ValueError (int(nan)), a
            limit of 0 OverflowError (int(inf));
  nEed      -5, 0.3, 0: 10 nodes, finite;
  n0, nh    the spectrum of |n0| with its sign flipped."""
import numpy as np
import pytest

import domain_cases as D
from oracle import naima_np as O


def _rows(cid, size="small"):
    c = D.CASES[D.IDS.index(cid)]
    # (0.0 and -0.0 are one key: the first wins; test_negative_zero looks at the other)
    return dict(reversed(list(zip(c[3], D.expected(cid, size)))))


def test_case_table_is_well_formed():
    """8 walkers per case, walker 0 and the last one legal with an entirely finite oracle row,
    every scalar of every class in the table, and the scalars given per walker beside the one
    under test are grid limits of that class"""
    seen = set()
    for cid, cls, name, values, legal, also in D.CASES:
        assert len(values) == len(legal) == D.NW, cid
        assert legal[0] and legal[-1], cid
        assert name in D.DEFAULTS[cls] and all(a in D.DEFAULTS[cls] for a in also), cid
        assert values[0] == D.DEFAULTS[cls][name], cid
        for size in D.SIZES:
            rows = D.expected(cid, size)
            for v, r, lg in zip(values, rows, legal):
                if lg:
                    assert D.outcome(r, True) == "legal", (cid, v)
        seen.add((cls, name))
    assert seen == {(cls, n) for cls, d in D.DEFAULTS.items() for n in d}
    assert D.energies("InverseCompton", "tiles").size == 70 > 64
    g = O.electron_grid(1e9, 1e14, 20)
    assert g.size == 100


@pytest.mark.parametrize("size", D.SIZES)
def test_every_scalar_has_the_outcomes_the_reference_can_give(size):
    """per scalar, the illegal walkers' oracle rows cover exactly the kinds domain_cases.OUTCOMES
    lists -- entirely finite and unphysical, non-finite, raising -- and the table as a whole has
    all three"""
    got = {}
    for cid, cls, name, values, legal, _ in D.CASES:
        for r, lg in zip(D.expected(cid, size), legal):
            if not lg:
                got.setdefault(name, set()).add(D.outcome(r, False))
    assert got == D.OUTCOMES
    assert {"unphysical", "nonfinite", "raises"} <= set().union(*got.values())


def test_theta_is_even_and_periodic():
    r = _rows("ic-theta")
    for key in ("flux", "seed"):
        assert np.array_equal(r[0.7][key], r[-0.7][key])  # (identical bits)
        # (2 pi - 0.7 is rounded to 4.4e-16: 1.2e-15 of 1 - cos(theta), which the kernel's
        # exp(-x), x ~ 1 / (1 - cos(theta)) up to ~40 where it still counts, turns into 5e-14)
        np.testing.assert_allclose(r[D.TWO_PI - 0.7][key], r[0.7][key], rtol=1e-13)
        assert np.all(np.isnan(r[0.0][key])) and np.all(np.isnan(r[1e-8][key]))
        for th in (np.pi, 4.0, -3.0):
            assert np.all(np.isfinite(r[th][key])) and np.all(r[th][key] > 0)
    # the isotropic spectrum of the same seed is another model (here 12.6 .. 13.2 times larger)
    E = D.energies("InverseCompton", "small")
    g = O.electron_grid(1e9, 1e14, 20)
    ne = O.nelec_on(D.particle_distribution(), g)
    par = dict(D.DEFAULTS["InverseCompton"])
    iso = O.ic_seed_spectrum(E, g, ne, dict(D.seeds(par)[1], theta=None))
    ratio = iso / r[0.7]["seed"]
    assert np.all(ratio > 2), ratio


def test_temperature_below_and_at_zero():
    r = _rows("ic-T")
    for T in (-30.0, -1e-30, 0.0):
        assert np.all(np.isnan(r[T]["flux"])) and np.all(np.isnan(r[T]["seed"]))
    for T in (1e-30, 3e4):
        assert np.all(np.isfinite(r[T]["flux"]))
    E = D.energies("InverseCompton", "small")
    g = O.electron_grid(1e9, 1e14, 20)
    ne = O.nelec_on(D.particle_distribution(), g)
    for T in (-30.0, 0.0):  # (isotropic as well)
        with np.errstate(all="ignore"):
            s = O.ic_seed_spectrum(E, g, ne, dict(type="thermal", T=T, u=0.5 * O.ERG_PER_EV, theta=None))
        assert np.all(np.isnan(s)), T
    # the legal values did not move with the oracle's T = 0 lines: Python's own arithmetic
    T, uu = 30.0, 0.5 * O.ERG_PER_EV
    K = O.ic_planck_kernel(g, T, E / O.MEC2_EV, 0.7)
    want = (uu / (O.AR_CGS * T ** 4)) * (E / O.MEC2_EV) * O.trapz_loglog(ne[None, :] * K, g) / E
    assert np.array_equal(r[30.0]["seed"], want)


def test_field_at_and_below_zero():
    for cid in ("syn-B", "syn-B-general"):
        for size in D.SIZES:
            r = _rows(cid, size)
            assert np.all(np.isnan(r[-1e-5]["flux"])) and np.all(np.isnan(r[0.0]["flux"]))
            assert np.any(np.isnan(r[-3e-4]["flux"]))
            assert np.all(r[1e-30]["flux"] == 0.0)  # (legal, and beyond every node's cut-off)


@pytest.mark.parametrize("cid", ["syn-Eemin", "ic-Eemin", "br-Eemin"])
def test_electron_grid_limits(cid):
    r = _rows(cid)
    assert r[-1e9] is ValueError and r[0.0] is OverflowError
    g = O.electron_grid(2e14, 1e14, 20)
    assert g.size == 10 and np.all(np.diff(g) < 0)
    back = O.electron_energy_content(D.particle_distribution(), O.electron_grid(1e14, 2e14, 20))
    assert np.all(np.isfinite(r[2e14]["flux"])) and np.any(r[2e14]["flux"] != 0)
    assert r[2e14]["W"] < 0 < back
    np.testing.assert_allclose(r[2e14]["W"], -back, rtol=1e-12)
    g = O.electron_grid(1e14, 1e14, 20)
    assert g.size == 10 and np.all(g == g[0])
    assert np.all(r[1e14]["flux"] == 0.0) and r[1e14]["W"] == 0.0
    hi = _rows(cid.replace("Eemin", "Eemax"))
    assert hi[-1e13] is ValueError and hi[0.0] is OverflowError


def test_proton_grid_limits():
    r = _rows("pp-Epmin")
    assert r[-2.0] is ValueError and r[0.0] is OverflowError
    assert O.proton_grid(2e5, 1e5, 20).size == 10
    assert np.all(np.isfinite(r[2e5]["flux"])) and r[2e5]["W"] < 0
    assert np.all(r[1e5]["flux"] == 0.0) and r[1e5]["W"] == 0.0
    for below in (0.5, 1.0):  # (below the threshold m_p + T_th = 1.218 GeV)
        assert below < O.M_P_GEV + O.T_TH_GEV and np.all(np.isnan(r[below]["flux"]))
    hi = _rows("pp-Epmax")
    assert hi[-1e5] is ValueError and hi[0.0] is OverflowError


@pytest.mark.parametrize("cid", ["syn-nEed", "ic-nEed", "br-nEed", "pp-nEpd"])
def test_node_density(cid):
    r = _rows(cid)
    for n in (-5, 0.3, 0):
        assert max(10, int(n * 5)) == 10
        assert np.all(np.isfinite(r[n]["flux"])) and np.array_equal(r[n]["flux"], r[-5]["flux"])
    assert O.electron_grid(1e9, 1e14, -5).size == 10


@pytest.mark.parametrize("cid", ["br-n0", "pp-nh"])
def test_negative_target_density(cid):
    c = D.CASES[D.IDS.index(cid)]
    r = _rows(cid)
    assert np.array_equal(r[-1.0]["flux"], -r[1.0]["flux"]) and np.any(r[1.0]["flux"] > 0)
    assert np.all(r[0.0]["flux"] == 0.0)
    assert r[-1.0]["W"] == r[1.0]["W"]
    assert c[2] in ("n0", "nh")


def test_negative_seed_energy_density():
    """u enters as the factor uf alone (radiative.py:667, 684): the second seed's part flips"""
    r = _rows("ic-u")
    assert np.array_equal(r[-0.5]["seed"], -r[0.5]["seed"])
    assert np.all(r[0.0]["seed"] == 0.0) and np.all(r[0.0]["flux"] > 0)  # (the CMB is left)


@pytest.mark.parametrize("cid", [c[0] for c in D.CASES if any(np.signbit(v) and v == 0 for v in c[3])])
def test_negative_zero(cid):
    """-0.0 is 0: a node density of -0.0 gives the 10 nodes of 0, a density of -0.0 a spectrum of
    zeros (of either sign), by walker index -- a dict keyed by value cannot tell the two apart"""
    c = D.CASES[D.IDS.index(cid)]
    rows = D.expected(cid, "small")
    neg = [i for i, v in enumerate(c[3]) if v == 0 and np.signbit(v)]
    pos = [i for i, v in enumerate(c[3]) if v == 0 and not np.signbit(v)]
    assert neg and pos
    for key in rows[pos[0]]:
        a, b = np.asarray(rows[neg[0]][key]), np.asarray(rows[pos[0]][key])
        assert np.array_equal(np.abs(a), np.abs(b)), (cid, key)
