"""Synchrotron self-absorption (nh_syn_absorption / nh_ssa_apply, SynchrotronSelfAbsorption):
kappa against the long double reference of tests/ssa_np.py at every launch shape the planner
picks (tests/ssa_cases.py: each case asks the planner first), the escape fractions against
mpmath, the entry points' refusals, scalar / host batch / device agreement of the model on an
analytic distribution and on CooledElectrons, Synchrotron.flux(radius=...), and a fit with a free
radius on the device loop.

nh_syn_absorption's bound: |out - ref| <= C0 S + C1 SX per element, S = pref sum |term|, SX =
pref sum |term| x.  It is test_gpu_synchrotron.py's derivation (which see: errors that the nodes
and dl share cost their own size, errors in which they disagree are amplified by A = 1 + 2^10, the
reciprocal of the series threshold) with the absorption kernel's own pieces, eps = 2^-53:
  shared, per node   Q = P (1 + x - Dp): P as syn_P1, 2e-14 + 14 eps; 3 Dp = num / den with
                     Bn gt3 and Cn gt2 each four times gt2 gt3 and five roundings in either: 40 eps
                     absolute, and 3e-14 of nh_rcp1f on 3 Dp <= 1: Dp to 13 eps + 1e-14, on
                     1 + x - Dp >= 2/3, with the sum's two roundings: 1.5e-14 + 23 eps; the
                     rounding of x in 1 + x: 10 eps; the product: 2 eps.  exp: 4 eps;
                     w / gamma = w (ig2 gam): 5 eps; (w/gamma) (Q ev): 2 eps       -> 4.2e-14
                     x = q ig2 under the exponential, as there                       -> 10 eps x
  disagreeing        dlw against the weights, rounded twice where a segment was planted
                     (ssa_cases.make_inputs): 4 eps; lx against ln of the two computed 1/gamma:
                     11 eps; the two exponentials: 8 eps; the four products of the two nodes:
                     4 eps; the sum (dlw - lx) + dlnQ - q dig2: 2 eps                -> A 29 eps
                     syn_dlnP1 on Q against ln(Q2/Q1) of the computed Q: D(grid) as there, at
                     the largest s^2 of Q the reference finds in each form's range   -> A D
                     x2 - x1 against q dig2, as there                                -> A 10 eps x
  the term           nh_rcp1f: 3e-14; the subtraction and two products: 3 eps
  the sums           400 eps, as there (the cases' longest chunk is the same)
  the prefactor      CS1's ten roundings and eight more: 18 eps
C0 = 4.2e-14 + 3e-14 + 421 eps + A (29 eps + D),  C1 = 10 eps + A 10 eps.
The prefactor 2 pi^2 hbar^3 CS1 / (m_e E) is small (hbar^3 / m_e = 1.3e-54) where the emission's
CS1 is large, so kappa itself may be a denormal float64 although its sum is not: each of the at
most 64 partial sums times the prefactor, and their sum, is then a multiple of 2^-1074.  The bound
carries that as the absolute term 65 * 2^-1074.
Underflow elements -- the sum before the prefactor below 2^-960 -- are held to
0 <= out <= 2 ref + 2^-1000 pref (test_ssa_host.py: at most 5 % of any case's live elements).

nh_ssa_apply's bound against mpmath, relative, for positive terms:
  tau                the area (2 pi / 3 or pi) R R: 3 eps, the division: 1, kappa's place in it:
                     none -- 5 eps with pi's own rounding, and |dln f / dln tau| <= 1      -> 5 eps
  sphere, tau < 1    20 coefficients rounded once and 19 fma: 20 eps sum |a_n| tau^(n-2) <=
                     30 eps, of f >= f(1) = 0.707; the first term left out is 2.6e-21      -> 43 eps
  sphere, tau >= 1   exp: 1 ulp; u = 1/2 + r (e - (1 - e) r) is 5 eps of 0.64 on u(1) = 0.236,
                     less beyond; 3 u r: 3 eps                                             -> 25 eps
  slab               expm1: 2 eps, the division: 1                                         -> 3 eps
  the terms          ncomp products and sums, colfac, the last product        -> (2 ncomp + 2) eps
"""
import ctypes as C
import warnings

import mpmath
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import ssa_cases as AC
import ssa_np as ANP
import synchrotron_np as SNP
from test_gpu_shapes import make_raw

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
AMP = 1 + 2.0 ** 10
C1 = 10 * EPS + AMP * 10 * EPS
UNDER = 2.0 ** -960
DENORMAL = 65 * SNP.LD(2) ** -1074  # kappa's own place in a float64 (see above)
SENTINEL = -7.25e77
F_BOUND = {"sphere": 48 * EPS, "slab": 8 * EPS}


def c0_of(s2):
    s3, s5, sl = np.sqrt(s2)
    rcp = 3e-14 + 3 * EPS
    D = max(2 * s3 ** 7 / 7 + rcp * 2 * s3, 2 * s5 ** 11 / 11 + rcp * 2 * s5,
            (2 * EPS + EPS * np.log((1 + sl) / (1 - sl))) if sl > 0 else 0.0)
    return 4.2e-14 + 3e-14 + 421 * EPS + AMP * (29 * EPS + D)


@pytest.fixture(scope="module")
def ctx():
    from naima_amd import _lib
    return _lib.get_context()


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


# ------------------------------------------------------------------------ 1. nh_syn_absorption
def _hold(got, ref, nE, what):
    assert np.all(got[:, nE:] == SENTINEL), what
    g = got[:, :nE]
    C0 = c0_of(ref["s2"])
    kap, S, SX = ref["kappa"], ref["S"], ref["SX"]
    nan = np.isnan(kap)
    assert np.array_equal(np.isnan(g), nan), (what, np.argwhere(np.isnan(g) != nan)[:8].tolist())
    dead = ~nan & (S == 0)
    assert np.all(g[dead] == 0.0), what
    live = ~nan & (S > 0)
    under = live & (ref["S_raw"] < UNDER)
    gl = g.astype(SNP.LD)
    cap = 2 * kap + SNP.LD(2) ** -1000 * ref["pref"]
    assert np.all((gl[under] >= 0) & (gl[under] <= cap[under])), what
    held = live & ~under
    with np.errstate(all="ignore"):
        frac = np.where(held, np.abs(gl - kap) / (C0 * S + C1 * SX + DENORMAL), 0)
    at = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[at])
    print("%-22s C0 = %.3g: max |out - ref| / (C0 S + C1 SX) = %.3g at walker %d, energy %d: %.3g "
          "of S (%d held, %d under the cap, %d dead, %d NaN)"
          % (what, C0, worst, at[0], at[1],
             float(np.abs(gl[at] - kap[at]) / S[at]) if held[at] else 0.0, held.sum(),
             under.sum(), dead.sum(), nan.sum()))
    assert worst <= 1.0, (what, worst, np.argwhere(frac > 1)[:8].tolist())


@pytest.mark.parametrize("case", AC.CASES, ids=AC.CASE_IDS)
def test_syn_absorption_variant(ctx, case):
    """one shape, on every grid of synchrotron_cases.grids_of: B read with ldB = 3, ldo = nE + 3
    with a sentinel in the padding.  Walkers 3..6 have B = 0, < 0, NaN, +inf (NaN rows); walker 7
    has a NaN weight at an interior node m: NaN exactly where i0 <= m"""
    cid, N, nG, nE, label, _ = case
    rc, p = AC.plan(N, nG, nE)
    assert rc == 0 and p[:3] == label, "the planner picks %r for %s" % (p, cid)
    for gname in AC.grids_of(nG):
        d = AC.make_case(cid, gname)
        ref = AC.case_reference(cid, gname)
        ldo = nE + 3
        out = ctx.array(np.full((N, ldo), SENTINEL))
        ctx.call("nh_syn_absorption", ctx.array(d["w"]), ctx.array(d["dlw"]), ctx.array(d["B"]), 3,
                 N, ctx.array(d["gam"]), ctx.array(d["lx"]), nG, ctx.array(d["E"]), nE, out, ldo)
        _hold(out.get(), ref, nE, "%s/%s" % (cid, gname))
        nan = np.isnan(ref["kappa"])
        assert all(nan[r].all() for r in AC.BAD_B)
        assert np.array_equal(nan[AC.NAN_ROW], ref["i0"][AC.NAN_ROW] <= d["nan_node"])


def test_syn_absorption_refusals(ctx):
    """return codes, nothing launches: NULL pointers, nG = 1, nE = 0, ldo < nE, ldB = 0, N < 0,
    nG = 5035 (150 KB of LDS); N = 0 is fine and leaves `out` as it was"""
    from naima_amd import _lib
    lib = _lib.load()
    N, nG, nE = 9, 40, 12
    d = AC.make_inputs(N, nG, nE, "low", "d40")
    dev = {k: ctx.array(d[k]) for k in ("w", "dlw", "B", "gam", "lx", "E")}
    out = ctx.array(np.full((N, nE), SENTINEL))

    def rc(N=N, nG=nG, nE=nE, ldo=nE, ldB=3, **ptr):
        a = {k: v.ptr for k, v in dev.items()}
        a.update(out=out.ptr, h=ctx.h)
        a.update(ptr)
        return lib.nh_syn_absorption(a["h"], a["w"], a["dlw"], a["B"], ldB, N, a["gam"], a["lx"],
                                     nG, a["E"], nE, a["out"], ldo)

    assert rc(nG=1) != 0 and rc(nE=0) != 0 and rc(ldo=nE - 1) != 0 and rc(ldB=0) != 0
    assert rc(N=-1) != 0
    assert rc(nG=5035) != 0 and b"LDS" in lib.nh_last_error()
    for name in ("h", "w", "dlw", "B", "gam", "lx", "E", "out"):
        assert rc(**{name: None}) != 0, name
        assert b"NULL" in lib.nh_last_error()
    o = [C.c_int(7) for _ in range(3)]
    assert lib.nh_syn_absorption_plan(16, 100, 40, None, *[C.byref(v) for v in o]) != 0
    assert rc(N=0) == 0
    ctx.sync()
    assert np.all(out.get() == SENTINEL)
    assert rc() == 0
    assert np.all(out.get() != SENTINEL)


# ----------------------------------------------------------------------------- 2. nh_ssa_apply
def _apply(ctx, kap, ldk, R, geometry, terms=(), colfac=None, write_tau=0, N=None, m=None, pad=3):
    from naima_amd.darray import as_lazy, nh_comp
    from naima_amd._lib import NH_SSA_GEOMETRY
    kd = ctx.array(kap)
    ldo = m + pad
    out = ctx.array(np.full((N, ldo), SENTINEL))
    keep = [ctx.array(b) for _, b in terms]
    comps = (nh_comp * max(len(terms), 1))()
    for j, ((s, b), dv) in enumerate(zip(terms, keep)):
        comps[j] = nh_comp(dv.ptr, b.shape[1], s)
    lz = as_lazy(R)
    ctx.call("nh_ssa_apply", kd, ldk, C.byref(lz), NH_SSA_GEOMETRY[geometry],
             comps if terms else None, len(terms), ctx.array(colfac) if colfac is not None else None,
             write_tau, N, m, out, ldo)
    got = out.get()
    assert np.all(got[:, m:] == SENTINEL)
    return got[:, :m]


def _rel(got, ref):
    """max |got / ref - 1| over an object array of mpf"""
    worst = 0.0
    for g, r in zip(np.ravel(got), np.ravel(ref)):
        worst = max(worst, abs(float(mpmath.mpf(float(g)) / r - 1)))
    return worst


@pytest.mark.parametrize("geometry", ANP.GEOMETRIES)
def test_ssa_apply_against_mpmath(ctx, geometry):
    """tau from 1e-12 to 1e4 and on both sides of tau = 1, nine walkers with radii over thirty
    decades from a device vector, m = 78 (more than one trip of a wave), per-walker rows: the
    factor alone, the optical depth, and the factor times two and eight positive terms with a
    column factor"""
    from naima_amd.darray import DVec
    rng = np.random.default_rng(5)
    tau0 = np.concatenate([AC.APPLY_TAU[1:], 10 ** rng.uniform(-3, 2, 78 - (AC.APPLY_TAU.size - 1))])
    N, m = 9, tau0.size
    R = 10.0 ** np.linspace(-5, 25, N)
    area = (2 * np.pi / 3 if geometry == "sphere" else np.pi) * R * R
    kap = np.stack([np.roll(tau0, 7 * w) for w in range(N)]) * area[:, None]
    Rd = ctx.array(R)
    Rv = DVec(ctx, Rd, Rd.ptr, N)
    ref = ANP.apply(kap, R, geometry)
    tau = np.array([[float(ANP.tau_of(kap[w, k], R[w], geometry)) for k in range(m)]
                    for w in range(N)])
    assert (tau < 1).sum() > 100 and (tau >= 1).sum() > 100
    assert ((tau < 1) & (tau > 1 - 1e-15)).any() and ((tau >= 1) & (tau < 1 + 1e-15)).any()
    got = _apply(ctx, kap, m, Rv, geometry, N=N, m=m)
    worst = _rel(got, ref)
    print("%s: max relative error of f = %.3g (bound %.3g)" % (geometry, worst, F_BOUND[geometry]))
    assert worst <= F_BOUND[geometry]
    assert np.all((got > 0) & (got <= 1))
    got = _apply(ctx, kap, m, Rv, geometry, write_tau=1, N=N, m=m)
    assert _rel(got, ANP.apply(kap, R, geometry, write_tau=True)) <= 5 * EPS
    for nc in (2, 8):
        terms = [(float(rng.uniform(0.5, 2)), rng.uniform(1, 2, (N, m)) * 1e-11) for _ in range(nc)]
        cf = rng.uniform(0.5, 2, m)
        got = _apply(ctx, kap, m, Rv, geometry, terms=terms, colfac=cf, N=N, m=m)
        worst = _rel(got, ANP.apply(kap, R, geometry, terms=terms, colfac=cf))
        assert worst <= F_BOUND[geometry] + (2 * nc + 2) * EPS, (nc, worst)


@pytest.mark.parametrize("geometry", ANP.GEOMETRIES)
def test_ssa_apply_rules(ctx, geometry):
    """kappa = 0 gives exactly the terms' sum times the column factor (and exactly 1 without
    terms); a NaN kappa gives NaN; a shared kappa row (ldk = 0) is every walker's; walkers with
    R <= 0, NaN or +-inf get NaN rows; a constant radius serves every walker"""
    from naima_amd.darray import DVec
    rng = np.random.default_rng(9)
    N, m = 7, 12
    row = np.concatenate([[0.0, np.nan, 0.0], 10 ** rng.uniform(-2, 2, m - 3)])
    R = np.array([1.0, 2.0, 0.0, -1.0, np.nan, np.inf, -np.inf])
    Rd = ctx.array(R)
    Rv = DVec(ctx, Rd, Rd.ptr, N)
    buf = rng.uniform(1, 2, (N, m))
    cf = rng.uniform(1, 2, m)
    with np.errstate(all="ignore"):
        got = _apply(ctx, row, 0, Rv, geometry, terms=[(0.5, buf), (0.25, buf)], colfac=cf, N=N, m=m)
    assert np.isnan(got[2:]).all() and np.isnan(got[:2, 1]).all()
    assert_array_equal(got[:2, [0, 2]], ((0.5 * buf + 0.25 * buf) * cf)[:2][:, [0, 2]])
    ref = ANP.apply(row, R, geometry, terms=[(0.5, buf), (0.25, buf)], colfac=cf)
    assert _rel(got[:2, 3:], ref[:2, 3:]) <= F_BOUND[geometry] + 6 * EPS
    alone = _apply(ctx, row, 0, Rv, geometry, N=N, m=m)
    assert np.all(alone[:2, [0, 2]] == 1.0) and np.isnan(alone[2:]).all()
    # the shared row against the same row given per walker, and a constant radius against a vector
    per = _apply(ctx, np.tile(row, (N, 1)), m, Rv, geometry, N=N, m=m)
    assert_array_equal(per, alone)
    const = _apply(ctx, row, 0, 2.0, geometry, N=3, m=m)
    assert_array_equal(const, np.tile(alone[1], (3, 1)))
    tau = _apply(ctx, row, 0, Rv, geometry, write_tau=1, N=N, m=m)
    assert np.all(tau[:2, [0, 2]] == 0.0) and np.isnan(tau[2:]).all() and np.isnan(tau[:2, 1]).all()


def test_ssa_apply_refusals(ctx):
    """every refusal returns a code and launches nothing; N = 0 is fine"""
    from naima_amd import _lib
    from naima_amd.darray import lazy_const, nh_comp
    lib = _lib.load()
    N, m = 4, 12
    kap = ctx.array(np.ones((N, m)))
    out = ctx.array(np.full((N, m), SENTINEL))
    lz = lazy_const(1.0)
    comps = (nh_comp * 9)()
    for j in range(9):
        comps[j] = nh_comp(kap.ptr, m, 1.0)
    cf = ctx.array(np.ones(m))

    def rc(h=ctx.h, k=kap.ptr, ldk=m, R=C.byref(lz), geo=0, comps=None, nc=0, cf=None, wt=0, N=N,
           m=m, o=out.ptr, ldo=m):
        return lib.nh_ssa_apply(h, k, ldk, R, geo, comps, nc, cf, wt, N, m, o, ldo)

    for kw in (dict(h=None), dict(k=None), dict(R=None), dict(o=None), dict(geo=2), dict(geo=-1),
               dict(nc=9, comps=comps), dict(nc=-1), dict(nc=1, comps=None),
               dict(wt=1, nc=1, comps=comps), dict(wt=1, cf=cf.ptr), dict(m=0), dict(ldo=m - 1),
               dict(ldk=m - 1), dict(ldk=-1), dict(N=-1)):
        assert rc(**kw) != 0, kw
    bad = (nh_comp * 1)()
    bad[0] = nh_comp(None, m, 1.0)
    assert rc(nc=1, comps=bad) != 0
    assert rc(N=0) == 0
    ctx.sync()
    assert np.all(out.get() == SENTINEL)
    assert rc(nc=8, comps=comps, cf=cf.ptr) == 0
    assert np.all(out.get() != SENTINEL)


# -------------------------------------------------------------------------------- 3. the model
ENERGIES_EV = np.geomspace(2e-6, 50.0, 12)  # 0.5 GHz .. 50 eV: opaque below ~1e-4 eV
KW = dict(Eemin=5e6, Eemax=5e11, nEed=60)   # eV


def _values(N=8):
    rng = np.random.default_rng(17)
    return dict(amp=10 ** rng.uniform(30.0, 31.0, N), alpha=rng.uniform(2.0, 3.0, N),
                cut=10 ** rng.uniform(10.5, 11.5, N), B=rng.uniform(0.1, 1.0, N),
                R=10 ** rng.uniform(14.5, 15.5, N))


def _analytic(na, v):
    u = na.u
    pd = na.ExponentialCutoffPowerLaw(v["amp"] / u.eV, 1e12 * u.eV, v["alpha"], v["cut"] * u.eV)
    return na.Synchrotron(pd, B=v["B"] * u.G, Eemin=KW["Eemin"] * u.eV, Eemax=KW["Eemax"] * u.eV,
                          nEed=KW["nEed"]), v["R"] * u.cm


def _cooled(na, v):
    u = na.u
    inj = na.PowerLaw(v["amp"] * 1e-6 / u.eV / u.s, 1e12 * u.eV, 2.0)
    pd = na.CooledElectrons(inj, v["B"] * u.G, v["alpha"] * 1e6 * u.s, seed_photon_fields=["CMB"],
                            Emin=5e6 * u.eV, Emax=5e11 * u.eV, n_per_decade=40)
    return na.Synchrotron(pd, B=v["B"] * u.G, Eemin=KW["Eemin"] * u.eV, Eemax=KW["Eemax"] * u.eV,
                          nEed=KW["nEed"]), v["R"] * u.cm


@pytest.mark.parametrize("build", [_analytic, _cooled], ids=["analytic", "cooled"])
@pytest.mark.parametrize("geometry", ANP.GEOMETRIES)
def test_scalar_host_batch_and_device_agree(na, ctx, build, geometry):
    """8 walkers x 12 energies.  The host batch and the same numbers as device values go through
    the same launches on the same bits (every value in the kernels' own units: nothing is
    converted): bit-equal.  A walker's scalar model is a launch of one walker at the batch's
    instance and chunking (the planner's C depends on N only above 16384 waves): its kappa is
    held to the reassociation of a chunked sum of positive terms, 2 (nseg + 64) eps = 1e-13, and
    tau and f follow kappa with |dln f / dln tau| <= 1.  flux(radius=R) is flux() times
    transmission(), from the same launches: bit-equal on the host and per walker"""
    from naima_amd.darray import DPars, DSsa
    u = na.u
    v = _values()
    names = list(v)
    N = 8
    e = ENERGIES_EV * u.eV
    syn, R = build(na, v)
    m = syn.self_absorption(R, geometry)
    assert m.batch_size == N and not m.on_device
    kap, tau, tr = m.absorption_area(e).to("cm2").value, m.opacity(e), m.transmission(e)
    assert kap.shape == tau.shape == tr.shape == (N, e.size)
    assert np.all(kap > 0) and tau.max() > 1 and tau.min() < 1e-3 and np.all((tr > 0) & (tr <= 1))
    assert tr.min() < 0.5
    area = (2 * np.pi / 3 if geometry == "sphere" else np.pi) * v["R"] ** 2
    assert_allclose(tau, kap / area[:, None], rtol=8 * EPS)
    f0 = syn.flux(e, distance=1 * u.kpc)
    fr = syn.flux(e, distance=1 * u.kpc, radius=R, geometry=geometry)
    assert_array_equal(fr.value, (f0 * tr).value)
    assert fr.unit == f0.unit
    sr = syn.sed(e, distance=0, radius=R, geometry=geometry)
    assert_allclose(sr.value, (syn.sed(e, distance=0) * tr).value, rtol=4 * EPS)  # (f T E^2, f E^2 T)
    # the same numbers on the device
    pars = DPars(ctx, ctx.array(np.stack([v[k] for k in names])), len(names), N)
    dsyn, dR = build(na, {k: pars[i] for i, k in enumerate(names)})
    dm = dsyn.self_absorption(dR, geometry)
    assert dm.on_device and dm.batch_size == N
    dt = dm.transmission(e)
    assert isinstance(dt, DSsa) and dt.shape == (N, e.size)
    assert_array_equal(dt.get(), tr)
    assert_array_equal(dm.opacity(e).get(), tau)
    assert_array_equal(np.asarray(dm.absorption_area(e).value), kap)
    dfr = dsyn.flux(e, distance=1 * u.kpc, radius=dR, geometry=geometry)
    # (1 / (4 pi d^2) is a factor of the device matrix and a divisor on the host: 2 eps)
    assert_allclose(np.asarray(dfr.value), fr.value, rtol=4 * EPS, atol=0)
    # a device radius on a host population, a host radius on a device population
    mixed = syn.flux(e, distance=1 * u.kpc, radius=dR, geometry=geometry)
    assert_array_equal(np.asarray(mixed.value), fr.value)
    assert_array_equal(dsyn.self_absorption(R, geometry).transmission(e).get(), tr)
    # every walker's scalar model
    for w in (0, 3, 7):
        s1, R1 = build(na, {k: float(x[w]) for k, x in v.items()})
        m1 = s1.self_absorption(R1, geometry)
        assert m1.batch_size is None
        t1, o1, k1 = m1.transmission(e), m1.opacity(e), m1.absorption_area(e).value
        assert t1.shape == o1.shape == k1.shape == (e.size,)
        assert_allclose(k1, kap[w], rtol=1e-13, atol=0)
        assert_allclose(o1, tau[w], rtol=1e-13, atol=0)
        assert_allclose(t1, tr[w], rtol=1e-13, atol=0)
        assert_array_equal(s1.flux(e, radius=R1, geometry=geometry).value,
                           (s1.flux(e) * t1).value)
    one = s1.flux(e[5], radius=R1, geometry=geometry)
    # (one energy alone gets every thread of its workgroup: other chunks, the same sum)
    assert one.shape == ()
    assert_allclose(one.value, s1.flux(e, radius=R1, geometry=geometry).value[5], rtol=1e-13)


def test_flux_without_a_radius_is_bit_equal(na):
    """flux() and sed() of a Synchrotron to which the model was attached, and after absorbed
    fluxes were taken from it, are the bits of a Synchrotron built before"""
    u = na.u
    v = _values()
    e = ENERGIES_EV * u.eV
    before, R = _analytic(na, v)
    f0, s0 = before.flux(e, distance=2 * u.kpc).value, before.sed(e).value
    after, _ = _analytic(na, v)
    m = after.self_absorption(R)
    m.transmission(e), after.flux(e, radius=R), m.opacity(e)
    assert_array_equal(after.flux(e, distance=2 * u.kpc).value, f0)
    assert_array_equal(after.sed(e).value, s0)
    assert_array_equal(after.flux(e, distance=2 * u.kpc, radius=None).value, f0)


def test_transmission_is_the_restatement(na):
    """one scalar model against tests/ssa_np.py on the model's own grid and weights: kappa at
    rtol 1e-9 (the particle weights' kernel against numpy's power law), both geometries"""
    u = na.u
    al, amp, B, R = 2.5, 3.65e30, 1.0, 1e15
    pd = na.PowerLaw(amp / u.eV, 1e12 * u.eV, al)
    syn = na.Synchrotron(pd, B=B * u.G, Eemin=KW["Eemin"] * u.eV, Eemax=KW["Eemax"] * u.eV,
                         nEed=100)
    e = ENERGIES_EV * u.eV
    gam = syn._gam
    g = gam.astype(SNP.LD)
    from naima_amd.constants import MEC2_EV
    w = (g * (amp * (g * SNP.LD(MEC2_EV) / SNP.LD(1e12)) ** -SNP.LD(al)) * SNP.LD(MEC2_EV))
    w = w.astype(np.float64)[None, :]
    dlw = np.zeros_like(w)
    dlw[0, :-1] = np.log(w[0, 1:].astype(SNP.LD) / w[0, :-1].astype(SNP.LD))
    lx = np.log(g[1:] / g[:-1]).astype(np.float64)
    ref = ANP.kappa(w, dlw, np.array([B]), gam, lx, ENERGIES_EV)["kappa"][0].astype(np.float64)
    for geo in ANP.GEOMETRIES:
        m = syn.self_absorption(R * u.cm, geo)
        assert_allclose(m.absorption_area(e).value, ref, rtol=1e-9)
        fr = [float(ANP.escape(ANP.tau_of(k, R, geo), geo)) for k in ref]
        assert_allclose(np.asarray(m.transmission(e)), fr, rtol=1e-9)


# --------------------------------------------------------------------------------- 4. in a fit
FIT_E = np.geomspace(3e-6, 3e2, 16)


def fit_model(na):
    """pars: log10 amplitude, alpha, log10(cutoff / eV), B / G, R / 1e15 cm"""
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 1e12 * u.eV, pars[1],
                                          10 ** pars[2] * u.eV)
        SYN = na.Synchrotron(pd, B=pars[3] * u.G, Eemin=KW["Eemin"] * u.eV,
                             Eemax=KW["Eemax"] * u.eV, nEed=KW["nEed"])
        T = SYN.self_absorption(pars[4] * 1e15 * u.cm).transmission(data)
        return SYN.flux(data, distance=1 * u.Mpc) * T, T

    def prior(pars):
        return (na.uniform_prior(pars[0], 25, 35) + na.uniform_prior(pars[1], 1, 4)
                + na.uniform_prior(pars[2], 9, 13) + na.uniform_prior(pars[3], 0.01, 10)
                + na.uniform_prior(pars[4], 0.01, 100))

    return model, prior, np.array([30.5, 2.5, 11.0, 0.5, 1.0]), np.array([0.02, 0.01, 0.02, 0.01,
                                                                          0.02])


def test_in_a_fit(na, monkeypatch):
    """64 walkers x 20 steps with R free: the device loop (piecewise: the one-launch plan does not
    know the two launches) records both in its plan and reproduces the host-driven loop's chain
    as closely as tests/test_gpu_pairabs.py and test_gpu_ebl.py ask of a free absorber; a walker
    with R < 0 has a NaN log-probability"""
    from naima_amd.datatable import make_data
    from naima_amd.sampler import EnsembleSampler
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    model, prior, p0, width = fit_model(na)
    e = FIT_E * na.u.eV
    true = model(np.repeat(p0[:, None], 2, axis=1), dict(energy=e))[0]
    true = true.to("1/(s cm2 eV)").value[0] * FIT_E ** 2 * 1.602176634e-12
    assert true[0] < 0.01 * true.max()  # (the radio points are on the absorbed side)
    raw = make_raw(FIT_E, true, "erg/(cm2 s)", np.random.default_rng(12), uls=(15,),
                   ul_factor=(1.7,))
    data = make_data(raw)
    nw, steps = 64, 20
    pos = p0 + width * np.random.default_rng(3).standard_normal((nw, p0.size))
    k = dict(args=[data, model, prior], seed=31, naima_style=True, store_blobs=True)
    h = EnsembleSampler(nw, p0.size, na.lnprob, device=False, **k)
    d = EnsembleSampler(nw, p0.size, na.lnprob, device=True, **k)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no "host-driven loop" warning)
        h.run_mcmc(pos, steps)
        d.run_mcmc(pos, steps)
    assert d.device is True and d._dev is not None and not d._dev.mega
    assert_allclose(d.get_chain(), h.get_chain(), rtol=1e-8)
    assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-6)
    calls = list(d._dev._plan.calls)
    print("\nlaunches of a step: %s" % calls)
    assert calls.count("nh_syn_absorption") == 1 and calls.count("nh_ssa_apply") == 1
    chain = d.get_chain()
    assert len(np.unique(chain[..., 4])) > nw  # (the radius moved)
    bd = np.asarray(d.get_blobs()[1], dtype=float)
    assert bd.shape == (steps, nw, FIT_E.size) and bd.min() < 0.05 and bd.max() <= 1.0
    again = np.asarray(model(np.ascontiguousarray(chain[-1].T), data)[1])
    assert_allclose(bd[-1], again, rtol=1e-13, atol=0)
    # R < 0: a NaN row, a NaN log-probability without a prior that excludes it
    bad = pos[:4].copy()
    bad[1, 4] = -1.0
    with np.errstate(all="ignore"):
        lp = na.lnprob(np.ascontiguousarray(bad.T), data, model, lambda pars: 0.0 * pars[0])[0]
    assert np.isnan(lp[1]) and np.isfinite(lp[[0, 2, 3]]).all()
