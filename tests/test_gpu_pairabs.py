"""Pair-production absorption on photon fields (nh_pairabs_rows / nh_pairabs_apply,
PairAbsorptionModel): the opacity rows against the mpmath golden file for every field kind, the
apply kernel's indexing, scalar / host batch / device agreement, the domain, linearity, the
factor in a model on the device loop, EblAbsorptionModel beside it, and the example."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import pairabs_cases as PC
from test_gpu_shapes import KPC, RT_MODEL, _sigma, make_raw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# nh_pairabs_rows against mpmath, per field kind: ten times the largest relative error measured
# on an MI355X (profiles/NOTES_pairabs.md: 5.5e-15, 2.2e-13, 1.1e-15, 1.4e-15), for other boxes
# and compiler versions, and far below the 1e-8 that is allowed at most (RTOL of
# tests/test_gpu_kelner.py).  The angle's figure is the rounding of eta itself, 3 * 2^-53, times
# 1/eta' <= 645 where the reference is still >= 1e-280.
RTOL_ROWS = {"thermal": 1e-13, "angle": 3e-12, "mono": 2e-14, "table": 2e-14}
TINY = 1e-280


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "pairabs.npz")))


def rows(na, kind, x, T=None, theta=None, se=None, sn=None, nrows=1):
    """kappa[nrows][x.size] of one nh_pairabs_rows launch; T, theta floats or DVecs"""
    from naima_amd import _lib
    from naima_amd.models import PairAbsorptionModel
    ctx = _lib.get_context()
    xd = ctx.array(np.asarray(x, dtype=float))
    sed = ctx.array(np.atleast_1d(se)) if se is not None else None
    snd = ctx.array(np.atleast_1d(sn)) if sn is not None else None
    out = ctx.empty((nrows, xd.shape[0]))
    PairAbsorptionModel._rows_launch(ctx, True, kind, T, theta, sed, snd,
                                     0 if sed is None else sed.shape[0], xd, xd.shape[0], nrows,
                                     out)
    return out.get()


def check_rows(got, ref, rtol, what):
    """relative wherever the reference is >= 1e-280, elsewhere a non-negative value <= 1e-280;
    returns the largest relative error"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape and not np.any(np.isnan(got)), what
    big = ref >= TINY
    assert np.all(got[~big] >= 0.0) and np.all(got[~big] <= TINY), (what, got[~big])
    err = np.abs(got[big] - ref[big]) / ref[big]
    print("%s: max relative error %.3g over %d values (%d below 1e-280)"
          % (what, err.max() if err.size else 0.0, big.sum(), (~big).sum()))
    assert np.all(err <= rtol), (what, err.max(), np.nonzero(err > rtol)[0])
    return err.max() if err.size else 0.0


# ------------------------------------------------------------------------- 1. rows vs golden
@pytest.mark.parametrize("T_K", [2.72548, 3.0e4])
def test_rows_thermal_isotropic_against_golden(na, golden, T_K):
    from naima_amd._lib import NH_PAIR_THERMAL
    eta = golden["eta"]
    x = eta / (T_K * PC.K_TO_MEC2)
    got = rows(na, NH_PAIR_THERMAL, x, T=T_K)[0]
    # (x * T k/m rounds eta by 2^-53: times 1/eta <= 50 on the Wien side, far below the bound)
    check_rows(got, PC.thermal_prefactor(T_K) * golden["iso"], RTOL_ROWS["thermal"],
               "thermal isotropic T=%g" % T_K)


@pytest.mark.parametrize("deg", PC.ANGLES_DEG)
def test_rows_thermal_at_an_angle_against_golden(na, golden, deg):
    from naima_amd._lib import NH_PAIR_THERMAL
    eta, T_K = golden["eta"], 30.0
    x = eta / (T_K * PC.K_TO_MEC2)
    got = rows(na, NH_PAIR_THERMAL, x, T=T_K, theta=float(np.deg2rad(deg)))[0]
    ref = PC.thermal_prefactor(T_K) * golden["ang%d" % deg]
    assert np.sum(ref >= TINY) >= 30 and (deg != 30.0 or np.sum(ref < TINY) >= 1)
    check_rows(got, ref, RTOL_ROWS["angle"], "thermal at %g deg" % deg)


def test_rows_monochromatic_against_golden(na, golden):
    from naima_amd._lib import NH_PAIR_MONO
    eta = golden["eta"]
    # E0 = m_e c^2 exactly: s0 = x, so the two neighbours of the threshold are met exactly
    got = rows(na, NH_PAIR_MONO, eta, se=PC.MEC2_EV)[0]
    ref = PC.SIGMA_T * golden["mono"]
    assert np.all(got[eta <= 1.0] == 0.0) and got[eta == np.nextafter(1.0, 2.0)][0] > 0.0
    check_rows(got[eta > 1.0], ref[eta > 1.0], RTOL_ROWS["mono"], "monochromatic")
    # from one direction: the closed form mu sigma(s0 mu / 2)
    for deg in (60.0, 180.0):
        th = float(np.deg2rad(deg))
        mu = 1.0 - np.cos(th)
        got = rows(na, NH_PAIR_MONO, eta, se=PC.MEC2_EV, theta=th)[0]
        refa = PC.SIGMA_T * mu * PC.sigma_np(eta * mu / 2.0)
        assert np.all(got[refa == 0.0] == 0.0)
        assert_allclose(got, refa, rtol=1e-12, atol=0)


def test_rows_tabulated_field(na):
    from naima_amd._lib import NH_PAIR_TABLE
    # a grey body's shape on 24 nodes with a zero node and nodes below the threshold of the
    # lower energies; the restatement's sbar is held to the golden file by test_pairabs_host
    eps = np.geomspace(1e-4, 1.0, 24)
    n = 1e3 * eps ** 2 / np.expm1(eps / 0.01)
    n[9] = 0.0
    E = np.geomspace(1e12, 5e16, 13)
    got = rows(na, NH_PAIR_TABLE, E / PC.MEC2_EV, se=eps, sn=n)[0]
    ref = PC.dtau_dl_table(E, eps, n)
    assert np.all(ref > 0.0)
    check_rows(got, ref, RTOL_ROWS["table"], "tabulated")
    # below every node's threshold: exactly 0
    assert rows(na, NH_PAIR_TABLE, np.array([1e9 / PC.MEC2_EV]), se=eps, sn=n)[0, 0] == 0.0


def test_rows_out_of_range_inputs(na):
    from naima_amd._lib import NH_PAIR_THERMAL
    x = np.array([0.0, 1e-30, 1e3, 1e9, 1e300])
    for theta in (None, 1.0):
        got = rows(na, NH_PAIR_THERMAL, x, T=2.7, theta=theta)[0]
        assert np.all(got[:2] == 0.0) and np.all(np.isfinite(got)) and np.all(got >= 0.0), got
    assert np.all(rows(na, NH_PAIR_THERMAL, x, T=2.7, theta=0.0)[0] == 0.0)


# --------------------------------------------------------------------- 2. the apply's indexing
@pytest.mark.parametrize("N", [1, 3, 5, 67])
@pytest.mark.parametrize("nE", [1, 63, 64, 65])
def test_apply_shapes(na, N, nE):
    """random kappa rows, shared and per walker, through DPairAbs: 1, 2 and 8 fields, terms with
    ld > n_e, a colfac, and the opacity itself"""
    from naima_amd import _lib
    from naima_amd.darray import DMat, DPairAbs, DVec
    ctx = _lib.get_context()
    rng = np.random.default_rng(1000 * N + nE)

    def dvec(v):
        d = ctx.array(v)
        return DVec(ctx, d, d.ptr, N)

    for nf in (1, 2, 8):
        fields, tau = [], np.zeros((N, nE))
        for f in range(nf):
            per_walker = f % 2 == 1 if nf > 1 else N == 3  # (mixed shared and per-walker rows)
            k = rng.uniform(0.0, 1.0, (N if per_walker else 1, nE))
            L, a = rng.uniform(0.5, 2.0, N), rng.uniform(0.1, 1.0, N)
            T = rng.uniform(1.0, 3.0, N) if f % 3 == 0 else None  # (a thermal field)
            dens = a * PC.AR_CGS * T ** 4 if T is not None else a
            # a path length as a plain device vector, a scaled one, or one number for all
            if f % 4 == 3:
                L = np.full(N, 1.25)
                Ld = 1.25
            elif f % 2 == 0:
                Ld = dvec(L)
            else:
                Ld, L = dvec(L / 3.0) * 3.0, (L / 3.0) * 3.0
            fields.append((ctx.array(k), per_walker, Ld, dvec(dens),
                           dvec(T) if T is not None else None))
            coef = L * (dens / (PC.AR_CGS * (T * T) ** 2) if T is not None else dens)
            tau = tau + coef[:, None] * k
        fac = DPairAbs(ctx, fields, N, nE)
        assert_allclose(fac.get(), np.exp(-tau), rtol=1e-14, atol=0)
        assert_allclose(DPairAbs(ctx, fields, N, nE, tau=True).get(), tau, rtol=1e-14, atol=0)
        ld = nE + 3
        b1, b2 = rng.standard_normal((N, ld)), rng.standard_normal((N, nE))
        d1, d2 = ctx.array(b1), ctx.array(b2)
        m = DMat(ctx, [(d1, d1.ptr + 8 * 2, ld, 0.5), (d2, d2.ptr, nE, -2.0)], (N, nE))
        cf = rng.uniform(0.5, 1.5, nE)
        want = np.exp(-tau) * (cf * (0.5 * b1[:, 2:2 + nE] - 2.0 * b2))
        for prod in (fac * (m * cf), (m * cf) * fac):
            assert isinstance(prod, DMat) and prod.shape == (N, nE)
            assert_allclose(prod.get(), want, rtol=1e-13, atol=1e-300)
    with pytest.raises(ValueError):
        fac.apply(DMat.from_buffer(ctx, d2, N, nE + 1))


# -------------------------------------------------------- 3. scalar, host batch, device values
def _fields(u, T, uu, th, n, L1, L2, L3):
    return ([["dust", T * u.K, uu * u.eV / u.cm ** 3], "CMB",
             ["star", 2e4 * u.K, 5.0 * u.erg / u.cm ** 3, th * u.deg],
             ["line", 2.0 * u.eV, n * u.eV / u.cm ** 3]],
            [L1 * u.kpc, L1 * u.kpc, L2 * u.au, L3 * u.pc])


ENERGIES_EV = np.geomspace(1e10, 3e15, 23)


@pytest.fixture(scope="module")
def batch(na):
    """per-walker values of every kind, the host batch's transmission and opacity"""
    N = 9
    rng = np.random.default_rng(7)
    v = dict(T=rng.uniform(20, 60, N), uu=rng.uniform(0.2, 2, N), th=rng.uniform(-170, 170, N),
             n=rng.uniform(1e3, 1e5, N), L1=rng.uniform(1, 20, N), L2=rng.uniform(0.5, 3, N),
             L3=rng.uniform(0.1, 2, N))
    e = ENERGIES_EV * na.u.eV
    m = na.PairAbsorptionModel(*_fields(na.u, **v))
    assert m.batch_size == N and not m.on_device
    return v, e, m.transmission(e), m.opacity(e)


def test_host_batch_rows_are_their_scalar_models(na, batch):
    v, e, tr, tau = batch
    assert isinstance(tr, np.ndarray) and tr.shape == tau.shape == (9, e.size)
    assert np.all((tr > 0) & (tr <= 1)) and tr.min() < 0.5 and tr.max() == 1.0
    assert_allclose(tr, np.exp(-tau), rtol=1e-15)
    for w in range(9):
        m = na.PairAbsorptionModel(*_fields(na.u, **{k: float(x[w]) for k, x in v.items()}))
        assert m.batch_size is None
        t1, o1 = m.transmission(e), m.opacity(e)
        assert t1.shape == o1.shape == (e.size,)
        assert_allclose(tr[w], t1, rtol=1e-12, atol=0)
        assert_allclose(tau[w], o1, rtol=1e-12, atol=0)
    # and the restatement
    w = 4
    ref = (PC.dtau_dl_thermal(ENERGIES_EV, v["T"][w], v["uu"][w] * 1.602176634e-12)
           * v["L1"][w] * KPC
           + PC.dtau_dl_thermal(ENERGIES_EV, 2.72548, PC.AR_CGS * 2.72548 ** 4) * v["L1"][w] * KPC
           + PC.dtau_dl_thermal(ENERGIES_EV, 2e4, 5.0, np.deg2rad(v["th"][w]))
           * v["L2"][w] * 1.495978707e13
           + PC.dtau_dl_mono(ENERGIES_EV, 2.0, v["n"][w] / 2.0) * v["L3"][w] * KPC * 1e-3)
    assert_allclose(tau[w], ref, rtol=1e-8, atol=0)


def test_device_values_are_bit_identical_to_the_host_batch(na, batch):
    from naima_amd import _lib
    from naima_amd.darray import DPairAbs, DPars
    v, e, tr, tau = batch
    ctx = _lib.get_context()
    names = list(v)
    pars = DPars(ctx, ctx.array(np.stack([v[k] for k in names])), len(names), 9)
    m = na.PairAbsorptionModel(*_fields(na.u, **{k: pars[i] for i, k in enumerate(names)}))
    assert m.on_device and m.batch_size == 9
    t = m.transmission(e)
    assert isinstance(t, DPairAbs) and t.shape == (9, e.size)
    assert_array_equal(t.get(), tr)
    assert_array_equal(np.asarray(t), tr)
    assert_array_equal(m.opacity(e).get(), tau)
    # one device value among scalars
    one = dict({k: float(x[2]) for k, x in v.items()}, L1=pars[names.index("L1")])
    t = na.PairAbsorptionModel(*_fields(na.u, **one)).transmission(e).get()
    host = na.PairAbsorptionModel(*_fields(na.u, **dict(one, L1=v["L1"]))).transmission(e)
    assert_array_equal(t, host)
    assert_allclose(t[2], tr[2], rtol=1e-12)


def test_per_walker_T_equal_to_the_shared_T_gives_the_shared_rows_bits(na):
    u = na.u
    e = ENERGIES_EV * u.eV
    shared = na.PairAbsorptionModel([["d", 35.0 * u.K, 0.7 * u.eV / u.cm ** 3],
                                     ["s", 9e3 * u.K, 2.0 * u.erg / u.cm ** 3, 75 * u.deg]],
                                    [4 * u.kpc, 2 * u.au])
    per = na.PairAbsorptionModel([["d", np.full(5, 35.0) * u.K, 0.7 * u.eV / u.cm ** 3],
                                  ["s", 9e3 * u.K, 2.0 * u.erg / u.cm ** 3,
                                   np.full(5, 75.0) * u.deg]], [4 * u.kpc, 2 * u.au])
    a, b = shared.transmission(e), per.transmission(e)
    assert b.shape == (5, e.size)
    for w in range(5):
        assert_array_equal(b[w], a)


# ------------------------------------------------------------------------------- 4. the domain
def test_domain(na):
    u = na.u
    e = ENERGIES_EV * u.eV
    ok = dict(L=3.0, uu=0.5, n=4e4, T=30.0)
    cases = [("L", x) for x in (-1.0, np.nan, np.inf, -np.inf)] + \
            [("uu", x) for x in (-1.0, np.nan, np.inf, -np.inf)] + \
            [("n", x) for x in (-1.0, np.nan, np.inf, -np.inf)] + \
            [("T", x) for x in (0.0, -1.0, np.nan, np.inf)]
    N = 2 * len(cases) + 1
    v = {k: np.full(N, x) for k, x in ok.items()}
    bad = np.zeros(N, dtype=bool)
    for i, (k, x) in enumerate(cases):
        v[k][2 * i + 1] = x
        bad[2 * i + 1] = True
    m = na.PairAbsorptionModel([["d", v["T"] * u.K, v["uu"] * u.eV / u.cm ** 3],
                                ["line", 2.0 * u.eV, v["n"] * u.eV / u.cm ** 3]],
                               [v["L"] * u.kpc, 1 * u.pc])
    with np.errstate(all="ignore"):
        tr, tau = m.transmission(e), m.opacity(e)
    for r in (tr, tau):
        assert np.all(np.isnan(r[bad])) and np.all(np.isfinite(r[~bad]))
    assert_array_equal(tr[~bad], np.broadcast_to(tr[0], tr[~bad].shape))
    assert tr[0].min() < 0.95

    # L = 0, u = 0, n = 0 and theta = 0: exactly 1
    zero = na.PairAbsorptionModel(["CMB", ["d", 30 * u.K, np.array([0.0, 1.0]) * u.eV / u.cm ** 3],
                                   ["line", 2.0 * u.eV, np.array([0.0, 1.0]) * u.eV / u.cm ** 3]],
                                  [np.array([0.0, 1.0]) * u.kpc, 1 * u.kpc, 1 * u.kpc])
    tz = zero.transmission(e)
    assert np.all(tz[0] == 1.0) and tz[1].min() < 1.0
    assert np.all(na.PairAbsorptionModel("CMB-FIR", 0 * u.kpc).transmission(e) == 1.0)
    th = np.array([0.0, 40.0, -40.0, -0.0, 180.0, -180.0])
    star = na.PairAbsorptionModel([["s", 9e3 * u.K, 2.0 * u.erg / u.cm ** 3, th * u.deg]],
                                  5 * u.au).transmission(e)
    assert np.all(star[0] == 1.0) and np.all(star[3] == 1.0) and star[1].min() < 1.0
    assert_array_equal(star[1], star[2])
    assert_array_equal(star[4], star[5])
    assert np.all(na.PairAbsorptionModel([["s", 9e3 * u.K, 2.0 * u.erg / u.cm ** 3, 0 * u.deg]],
                                         5 * u.au).transmission(e) == 1.0)


# ---------------------------------------------------------------------------- 5. linearity
def test_linearity(na):
    u = na.u
    e = ENERGIES_EV * u.eV
    d1 = ["d1", 35.0 * u.K, 0.7 * u.eV / u.cm ** 3]
    d2 = ["d2", 35.0 * u.K, 0.7 * u.eV / u.cm ** 3]
    twice = ["d", 35.0 * u.K, 1.4 * u.eV / u.cm ** 3]
    a = na.PairAbsorptionModel([d1, d2], 6 * u.kpc).transmission(e)
    b = na.PairAbsorptionModel([twice], 6 * u.kpc).transmission(e)
    assert a.min() < 0.9
    assert_array_equal(a, b)
    whole = na.PairAbsorptionModel(["CMB", d1], 6 * u.kpc).transmission(e)
    p1 = na.PairAbsorptionModel(["CMB", d1], 2.5 * u.kpc).transmission(e)
    p2 = na.PairAbsorptionModel(["CMB", d1], 3.5 * u.kpc).transmission(e)
    assert_allclose(p1 * p2, whole, rtol=1e-15, atol=0)


# -------------------------------------------------------------------------------- 6. in a fit
IGRID = (1e11, 3e16, 40)
FIT_E = np.geomspace(3e11, 2e15, 18)
VARIANTS = {
    # name: (extra start values, their widths)
    "fixed": ((), ()),
    "length": ((6.0,), (0.5,)),
    "T_u": ((32.0, 0.6), (1.5, 0.05)),
}


def fit_models(na, variant):
    """IC on the CMB from a hard electron spectrum, absorbed on the CMB and a dust field;
    pars: log10 amplitude, alpha, log10(cutoff / TeV) [, L / kpc | , T / K, u / (eV/cm3)]"""
    u = na.u

    def absorber(pars):
        if variant == "fixed":
            return na.PairAbsorptionModel(["CMB", "FIR"], 6.0 * u.kpc)
        if variant == "length":
            return na.PairAbsorptionModel(["CMB", "FIR"], pars[3] * u.kpc)
        return na.PairAbsorptionModel(["CMB", ["dust", pars[3] * u.K, pars[4] * u.eV / u.cm ** 3]],
                                      6.0 * u.kpc)

    def emission(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV)
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=IGRID[0] * u.eV,
                               Eemax=IGRID[1] * u.eV, nEed=IGRID[2])
        return IC.flux(data, distance=2 * u.kpc)

    def model(pars, data):
        T = absorber(pars).transmission(data)
        return emission(pars, data) * T, T

    def both(pars, data, L=None):  # (7: the EBL factor beside it)
        T = (absorber(pars) if L is None else
             na.PairAbsorptionModel(["CMB", "FIR"], L * u.kpc)).transmission(data)
        Z = na.EblAbsorptionModel(pars[1] * 0.01 * u.dimensionless_unscaled).transmission(data)
        return emission(pars, data) * Z * T, Z

    def ebl_only(pars, data):
        Z = na.EblAbsorptionModel(pars[1] * 0.01 * u.dimensionless_unscaled).transmission(data)
        return emission(pars, data) * Z, Z

    def tau_restated(p):
        if variant == "T_u":
            T, uu, L = p[3], p[4], 6.0
        else:
            T, uu, L = 30.0, 0.5, (p[3] if variant == "length" else 6.0)
        Tc = 2.72548
        return L * KPC * (PC.dtau_dl_thermal(FIT_E, Tc, PC.AR_CGS * Tc ** 4)
                          + PC.dtau_dl_thermal(FIT_E, T, uu * 1.602176634e-12))

    return model, emission, tau_restated, both, ebl_only


def fit_prior(na, variant):
    ex = VARIANTS[variant][0]

    def prior(pars):
        lp = (na.uniform_prior(pars[0], 20, 45) + na.uniform_prior(pars[1], 1, 4)
              + na.uniform_prior(pars[2], 0, 5))
        if variant == "length":
            lp = lp + na.normal_prior(pars[3], 6.0, 1.0) + na.uniform_prior(pars[3], 0, 30)
        elif variant == "T_u":
            lp = lp + na.uniform_prior(pars[3], 5, 100) + na.uniform_prior(pars[4], 0, 10)
        return lp

    def oprior(p):
        from oracle import naima_np as O
        lp = sum(O.uniform_prior(p[i], lo, hi) for i, (lo, hi) in
                 enumerate([(20, 45), (1, 4), (0, 5)]))
        if variant == "length":
            lp += O.normal_prior(p[3], 6.0, 1.0) + O.uniform_prior(p[3], 0, 30)
        elif variant == "T_u":
            lp += O.uniform_prior(p[3], 5, 100) + O.uniform_prior(p[4], 0, 10)
        return float(lp)

    return prior, oprior, np.array((33.5, 2.1, 3.0) + ex), np.array((0.05, 0.01, 0.02) + VARIANTS[variant][1])


def fit_raw(na, variant):
    from naima_amd.datatable import make_data
    model = fit_models(na, variant)[0]
    p0 = fit_prior(na, variant)[2]
    e = FIT_E * na.u.eV
    true = model(np.repeat(p0[:, None], 2, axis=1), dict(energy=e))[0]
    true = true.to("1/(s cm2 eV)").value[0] * FIT_E ** 2 * 1.602176634e-12
    raw = make_raw(FIT_E, true, "erg/(cm2 s)", np.random.default_rng(12), uls=(16,),
                   ul_factor=(1.7,))
    return raw, make_data(raw)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_in_a_fit(na, monkeypatch, variant):
    from naima_amd.sampler import EnsembleSampler
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    model, emission, tau_restated, _, _ = fit_models(na, variant)
    prior, oprior, p0, width = fit_prior(na, variant)
    raw, data = fit_raw(na, variant)
    nw, steps = 16, 6
    pos = p0 + width * np.random.default_rng(3).standard_normal((nw, p0.size))
    k = dict(args=[data, model, prior], seed=31, naima_style=True, store_blobs=True)
    h = EnsembleSampler(nw, p0.size, na.lnprob, device=False, **k)
    d = EnsembleSampler(nw, p0.size, na.lnprob, device=True, **k)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no "host-driven loop" warning)
        h.run_mcmc(pos, steps)
        d.run_mcmc(pos, steps)
    assert d.device is True and d._dev is not None
    # the rtol of tests/test_gpu_ebl.py for the free redshift
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-8)
    assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-6)
    chain = d.get_chain()
    bd = [np.asarray(b, dtype=float) for b in d.get_blobs()]
    assert bd[1].shape == (steps, nw, FIT_E.size)
    for s in (0, steps - 1):
        again = np.asarray(model(np.ascontiguousarray(chain[s].T), data)[1])
        assert_allclose(bd[1][s], np.broadcast_to(again, bd[1][s].shape), rtol=1e-13, atol=0)
    assert bd[1].min() < 0.7 and bd[1].max() <= 1.0
    calls = list(d._dev._plan.calls)
    print("\n%s: launches of a step: %s" % (variant, calls))
    assert "nh_pairabs_apply" in calls
    assert ("nh_pairabs_rows" in calls) == (variant == "T_u")
    if variant == "length":
        assert len(np.unique(chain[..., 3])) > nw  # (the length moved)
    # the first ensemble against the restatement applied to the unabsorbed device flux
    flux0 = emission(np.ascontiguousarray(chain[0].T), data).to("1/(s cm2 eV)").value
    lp = d.get_log_prob()[0]
    ul = np.asarray(raw["ul"], dtype=bool)
    for w in range(nw):
        rep = WN.to_data_repr(flux0[w] * np.exp(-tau_restated(chain[0, w])), raw)
        lp_o = O.lnprobmodel(rep, raw) + oprior(chain[0, w])
        dd, sg = _sigma(raw, rep)
        bound = np.sum(np.abs(dd[~ul]) * RT_MODEL * np.abs(rep[~ul]) / sg[~ul] ** 2) \
            + 1e-12 * abs(lp_o)
        assert abs(lp[w] - lp_o) <= bound, (variant, w, lp[w], lp_o, bound)
    assert np.all(np.isfinite(bd[0]))


# ------------------------------------------------------------------- 7. DEbl beside the factor
def test_ebl_factor_is_unchanged_beside_it(na, monkeypatch):
    from naima_amd.sampler import EnsembleSampler
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    _, _, _, both, ebl_only = fit_models(na, "length")
    prior, _, p0, width = fit_prior(na, "length")
    raw, data = fit_raw(na, "length")
    nw = 16
    pos = p0 + width * np.random.default_rng(3).standard_normal((nw, p0.size))

    def run(model, steps):
        d = EnsembleSampler(nw, p0.size, na.lnprob, device=True, args=[data, model, prior],
                            seed=31, naima_style=True, store_blobs=True)
        d.run_mcmc(pos, steps)
        assert d.device is True
        return d, d.get_chain(), np.asarray(d.get_blobs()[1], dtype=float)

    # a path length of 0 makes the new factor exactly 1: the same fit, bit for bit, with the
    # factor's launches in every step
    _, c0, z0 = run(ebl_only, 6)
    d1, c1, z1 = run(lambda pars, data: both(pars, data, L=0.0), 6)
    assert "nh_pairabs_apply" in d1._dev._plan.calls and "nh_ebl_apply" in d1._dev._plan.calls
    assert_array_equal(c1, c0)
    assert_array_equal(z1, z0)
    assert len(np.unique(np.round(c0[..., 1], 2))) > 1  # (several redshift rows were gathered)
    # with real absorption the likelihood is another one, and the EBL blob stays the bits of the
    # model's own factor at the stored positions
    _, c2, z2 = run(both, 2)
    for s in range(2):
        for c, z in ((c0, z0), (c2, z2)):
            assert_array_equal(z[s], na.EblAbsorptionModel(c[s][:, 1] * 0.01).transmission(data))


# ------------------------------------------------------------------------------ 8. the example
def test_pevatron_absorbed_example():
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "pevatron_absorbed.py"),
                        "32", "30", "60"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device loop: True" in r.stdout, r.stdout
    for key in ("intrinsic cut-off", "absorbed cut-off", "path length"):
        assert any(ln.startswith(key) for ln in r.stdout.splitlines()), r.stdout
