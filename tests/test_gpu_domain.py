"""Scalars outside their physical domain, on the device, against the oracle: the cases of
tests/domain_cases.py (test_domain_host.py holds them to the reference's behaviour).

A stretch move takes a legal ensemble to such values all the time -- a negative scattering angle,
field or density, grid limits that cross, a limit at or below 0 -- and the reference does
arithmetic on them: a finite number, a NaN or an exception.  Whether the proposal is rejected
depends on which, so the kernels have to give the same.  The rule, per walker:

  (a) the oracle's row is entirely finite: the device row equals it (RT_MODEL = 1e-9, RT_WE = 1e-10
      of test_gpu_shapes.py, atol 1e-200 of the row's largest magnitude; an exact 0 is an exact 0);
  (b) the oracle's row has a non-finite element: so has the device row, and the elements finite
      in both agree as in (a);
  (c) the reference raises (int() of a node count that is NaN or inf): a scalar given on the host
      raises the same exception type; a value per walker gives that walker a NaN row, leaves the
      other walkers alone, and is not reported as a grid too long for LDS;
  (d) the legal walkers of a batch equal the same walkers in a batch of their own, bit for bit:
      a batch of the same size and one of their own size (rtol 5e-13 instead only where the
      smaller batch runs another kernel: launch_depends_on_batch).

Every scalar comes as a Python scalar (the shared tables: nh_table_ic_planck +
nh_integrate_tables, k_synchrotron), as a host vector and as a device value (the general kernels
nh_general_electron / nh_general_proton for a scalar that shapes a grid or an emission kernel; a
factor per walker for B, u, n0 and nh), at 6 / 7 photon energies and at 70.

The loops: run_loop / check_oracle / same_chains of test_gpu_shapes.py, 16 walkers, 3 + 4 steps
across a run_mcmc boundary, in all three modes.  What each case measured is in
profiles/NOTES_domain.md; pytest -s prints it."""
import warnings

import numpy as np
import pytest

import domain_cases as D
from test_gpu_shapes import (KPC, MODES, RT_MODEL, RT_WE, _repr, _spread, check_oracle, make_raw,
                             run_loop, same_chains, uniform)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


# ------------------------------------------------------------------------------- class level
def _quantity(na, name, v):
    u = na.u
    if name in ("Eemin", "Eemax"):
        return v * u.eV
    if name in ("Epmin", "Epmax"):
        return v * u.GeV
    if name in ("nEed", "nEpd"):
        return v
    return {"B": lambda: v * u.G, "T": lambda: v * u.K, "u": lambda: v * u.eV / u.cm ** 3,
            "theta": lambda: v * u.rad, "n0": lambda: v / u.cm ** 3, "nh": lambda: v / u.cm ** 3}[name]()


def build(na, cls, par, n):
    """the class with the scalars ``par`` (name -> Python scalar | host vector | device value);
    n: the batch (None: a plain scalar model)"""
    u = na.u
    amp = D.AMP if n is None else np.full(n, D.AMP)
    pd = na.ExponentialCutoffPowerLaw(amp / u.eV, D.E0 * u.eV, D.ALPHA, D.ECUT * u.eV, D.BETA)
    q = {k: _quantity(na, k, v) for k, v in par.items()}
    if cls == "Synchrotron":
        return na.Synchrotron(pd, B=q["B"], Eemin=q["Eemin"], Eemax=q["Eemax"], nEed=q["nEed"])
    if cls == "Bremsstrahlung":
        return na.Bremsstrahlung(pd, n0=q["n0"], Eemin=q["Eemin"], Eemax=q["Eemax"], nEed=q["nEed"])
    if cls == "PionDecay":
        return na.PionDecay(pd, nh=q["nh"], useLUT=False, Epmin=q["Epmin"], Epmax=q["Epmax"],
                            nEpd=q["nEpd"])
    return na.InverseCompton(pd, seed_photon_fields=["CMB", ["star", q["T"], q["u"], q["theta"]]],
                             Eemin=q["Eemin"], Eemax=q["Eemax"], nEed=q["nEed"])


def routes(na, cls, par, n, E):
    """name -> a call that gives the host array of one route of the class: flux [n][nE] 1/(s eV),
    seed (InverseCompton: the second seed alone), W [n] erg (We / Wp over the object's own
    limits) and Wc: compute_We / compute_Wp of an object whose OWN limits are the legal ones, with
    the case's limits as the call's arguments -- validate_scalar_or_batch, the call's limits
    against the object's batch, then the general kernel (radiative.py:168-195, 1023-1055)"""
    u = na.u
    lo, hi = ("Epmin", "Epmax") if cls == "PionDecay" else ("Eemin", "Eemax")

    def host(x, unit):
        return np.asarray(x.to(unit).value, dtype=float)

    def model():
        return build(na, cls, par, n)

    def between():
        own = build(na, cls, dict(par, **{lo: D.DEFAULTS[cls][lo], hi: D.DEFAULTS[cls][hi]}), n)
        kw = {lo: _quantity(na, lo, par[lo]), hi: _quantity(na, hi, par[hi])}
        return host(own.compute_Wp(**kw) if cls == "PionDecay" else own.compute_We(**kw), "erg")

    r = dict(flux=lambda: host(model().flux(E * u.eV, distance=0), "1/(s eV)"))
    if cls == "InverseCompton":
        r["seed"] = lambda: host(model().flux(E * u.eV, distance=0, seed="star"), "1/(s eV)")
    r["W"] = lambda: host(model().Wp if cls == "PionDecay" else model().We, "erg")
    r["Wc"] = between
    return r


def evaluate(na, cls, par, n, E):
    """every route of ``routes`` as host arrays"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (a NaN / inf on the host side of a factor)
        return {k: f() for k, f in routes(na, cls, par, n, E).items()}


worst = {}


def check_row(got, want, rt, where):
    """rules (a) and (b) for one walker's row (or its W, as a row of one)"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape, where
    fin = np.isfinite(want)
    if fin.all():
        assert np.isfinite(got).all(), (where, got, want)
    else:
        assert not np.isfinite(got).all(), (where, got, want)
    both = fin & np.isfinite(got)
    if not both.any():
        return
    g, w = got[both], want[both]
    zero = w == 0.0
    assert np.all(g[zero] == 0.0), (where, g, w)
    atol = 1e-200 * np.max(np.abs(w))
    err = np.abs(g - w)
    rel = float(np.max(err / np.maximum(np.abs(w), 1e-300))) if err.size else 0.0
    worst[where[:2]] = max(worst.get(where[:2], 0.0), rel / rt if np.max(np.abs(w)) > 0 else 0.0)
    assert np.all(err <= atol + rt * np.abs(w)), (where, rel)


def check_batch(got, rows, where):
    for i, r in enumerate(rows):
        w = where + (i,)
        if isinstance(r, type):  # (c): a NaN row for that walker alone
            for key, v in got.items():
                assert np.all(np.isnan(v[i])), (w, key, v[i])
            continue
        for key, v in got.items():
            check_row(v[i], r[key], RT_WE if key in ("W", "Wc") else RT_MODEL, w + (key,))


FORMS = ("host", "device")


def _form(na, cls, name, values, also, form):
    """(par, n) of a batch with the scalar as a host vector or as a device value"""
    from naima_amd._lib import get_context
    from naima_amd.darray import DPars
    v = np.asarray(values, dtype=float)
    base = dict(D.DEFAULTS[cls])
    for a in also:
        base[a] = np.full(v.size, base[a])
    if form == "device":
        ctx = get_context()
        v = DPars(ctx, ctx.array(v[None, :].copy()), 1, v.size)[0]
    return dict(base, **{name: v}), len(values)


def launch_depends_on_batch(cls, name, also, nE, n_full, n_own):
    """True where a smaller batch runs ANOTHER kernel: nh_integrate_tables takes k_integrate_rows
    (nh_seg_term: the series below |dl| = 2^-7) under 1024 (walker, column) pairs and the tiled
    k_integrate_tables (nh_seg_pos: below 2^-10) from there on (integrate_impl, nh_core.hip).
    Only the shared tables go through it -- B, u, n0, nh as a factor per walker -- with the
    components side by side as columns: two seeds, or e-e | e-ion.  The general kernels and
    k_synchrotron run one workgroup per walker (and tile) whatever the batch."""
    if also or name in D.STRUCTURAL or cls == "Synchrotron":
        return False
    nK = nE * (2 if cls in ("InverseCompton", "Bremsstrahlung") else 1)
    return (n_full * nK < 1024) != (n_own * nK < 1024)


@pytest.mark.parametrize("size", D.SIZES)
@pytest.mark.parametrize("cid", D.IDS)
def test_scalar_outside_its_domain(na, cid, size):
    """every case of domain_cases.CASES in every form, rules (a) .. (d) of the module docstring"""
    from naima_amd._lib import get_context
    _, cls, name, values, legal, also = D.CASES[D.IDS.index(cid)]
    rows = D.expected(cid, size)
    E = D.energies(cls, size)
    ctx = get_context()
    # ---- a Python scalar, one walker at a time: the shared tables
    if not also:
        for i, (v, r) in enumerate(zip(values, rows)):
            par = dict(D.DEFAULTS[cls], **{name: v})
            where = (cid, "scalar", i)
            if isinstance(r, type):  # (every route on its own: each has to raise)
                for key, f in routes(na, cls, par, None, E).items():
                    with pytest.raises(r):
                        f()
            elif name in D.REFUSED_NEGATIVE and v < 0:
                with pytest.raises(ValueError, match="positive"):
                    evaluate(na, cls, par, None, E)
            else:
                got = evaluate(na, cls, par, None, E)
                for key, g in got.items():
                    check_row(g, r[key], RT_WE if key in ("W", "Wc") else RT_MODEL, where + (key,))
    # ---- a value per walker, on the host and on the device
    keep = np.asarray(legal)
    for form in FORMS:
        par, n = _form(na, cls, name, values, also, form)
        if form == "device" and cls == "InverseCompton" and name == "nEed":
            # (InverseCompton evaluates a node density per walker one walker at a time, on the host)
            with pytest.raises(NotImplementedError):
                evaluate(na, cls, par, n, E)
            continue
        got = evaluate(na, cls, par, n, E)
        # no "grid too long": on the host form the check is Context.check_general inside the call,
        # which raises; a device value leaves the status word for the sampler, so it is read here
        assert int(ctx.general_status().get()[0]) == 0, (cid, form)
        check_batch(got, rows, (cid, form))
        # (d): the legal walkers in a batch of their own, bit for bit -- of the same size, walker
        # 0's value in the place of every illegal one, and of their own size.  Where the smaller
        # batch runs another kernel (launch_depends_on_batch) the two differ in how a segment's
        # term is formed: nh_common.h gives the main form's loss to the cancellation in u2 - u1 as
        # 2e-13 and its reciprocal's as 3e-14, so twice 2.3e-13 there, and only there
        same = [v if k else values[0] for v, k in zip(values, keep)]
        own = [v for v, k in zip(values, keep) if k]
        alone = evaluate(na, cls, *_form(na, cls, name, same, also, form), E)
        for key in got:
            assert np.array_equal(got[key][keep], alone[key][keep]), (cid, form, key)
        alone = evaluate(na, cls, *_form(na, cls, name, own, also, form), E)
        other = launch_depends_on_batch(cls, name, also, E.size, len(values), len(own))
        for key in got:
            a, b = got[key][keep], alone[key]
            if other and key in ("flux", "seed"):
                dmax = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
                worst[(cid, form + " own size")] = max(worst.get((cid, form + " own size"), 0.0), dmax)
                np.testing.assert_allclose(a, b, rtol=5e-13, atol=0, err_msg=str((cid, form, key)))
            else:
                assert np.array_equal(a, b), (cid, form, key, "own size")
    print("\n%s (%s): largest error over the tolerance %s" % (
        cid, size, {k[1]: "%.2g" % v for k, v in worst.items() if k[0] == cid}))


def test_grid_too_long_is_still_reported(na):
    """a span whose node count exceeds Context.general_nmax ends the call with the library's
    error, as before: the NaN row of a walker whose count is not finite is another matter"""
    from naima_amd._lib import NaimaHipError, get_context
    _, cls, name, values = D.TOO_LONG
    par = dict(D.DEFAULTS[cls], **{name: np.asarray(values)})
    assert get_context().general_nmax == 2048
    with pytest.raises(NaimaHipError, match="2670 nodes"):
        evaluate(na, cls, par, len(values), D.energies(cls, "small"))


@pytest.mark.parametrize("cid", ["ic-theta", "ic-theta-general"])
def test_scattering_angle_is_even(na, cid):
    """theta and -theta in one batch give the same row (rtol 1e-13, as test_gpu_general.py holds
    two routes of the same arithmetic), as a host vector and as a device value -- and that row is
    not the isotropic seed's, which is more than twice as large"""
    _, cls, name, values, legal, also = D.CASES[D.IDS.index(cid)]
    E = D.energies(cls, "small")
    assert values[0] == -values[1] == 0.7
    u = na.u
    pd = na.ExponentialCutoffPowerLaw(D.AMP / u.eV, D.E0 * u.eV, D.ALPHA, D.ECUT * u.eV, D.BETA)
    d = D.DEFAULTS[cls]
    iso = na.InverseCompton(pd, seed_photon_fields=["CMB", ["star", d["T"] * u.K, d["u"] * u.eV / u.cm ** 3]],
                            Eemin=d["Eemin"] * u.eV, Eemax=d["Eemax"] * u.eV, nEed=d["nEed"])
    iso = np.asarray(iso.flux(E * u.eV, distance=0, seed="star").to("1/(s eV)").value, dtype=float)
    for form in FORMS:
        got = evaluate(na, cls, *_form(na, cls, name, values, also, form), E)
        for key in ("flux", "seed"):
            np.testing.assert_allclose(got[key][1], got[key][0], rtol=1e-13, err_msg=form)
        for i in (0, 1):
            ratio = iso / got["seed"][i]
            print("\n%s %s theta = %+.1f: isotropic / anisotropic = %s" % (cid, form, values[i], ratio))
            assert np.all(ratio > 2), (form, i, ratio)


# ------------------------------------------------------------------------------------- loops
NW, STEPS, SEED = 16, (3, 4), 5


def _ecpl(na, pars):
    u = na.u
    return na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1], 10 ** pars[2] * u.TeV)


def _ecpl_o(p):
    from oracle import naima_np as O
    return O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12, alpha=p[1],
                          e_cutoff=10 ** p[2] * 1e12, beta=1.0)


def _all_walkers(nsteps):
    return [(s, w) for s in (0, nsteps - 1) for w in range(NW)]


def _data(omodel, p0, E, seed, flux_unit="erg/(cm2 s)"):
    rng = np.random.default_rng(seed)
    return make_raw(E, _repr(omodel(p0, E)[0], E, flux_unit), flux_unit, rng, rel=(0.05, 0.05),
                    scatter=0.05, cl0=0.9, dcl=0.0)


def test_loop_scattering_angle_straddles_zero(na, monkeypatch):
    """IC on the CMB and one anisotropic seed whose theta is a fit parameter, started in a ball
    around 0.3 rad of width 0.4 under the prior [-3, 3]: the sampled positions hold negative and
    positive angles (asserted), and every one of them has the oracle's spectrum for ITS angle"""
    from oracle import naima_np as O
    u = na.u
    grid = (2e11, 1e15, 20)

    def model(pars, data):
        IC = na.InverseCompton(_ecpl(na, pars), seed_photon_fields=[
            "CMB", ["star", 30 * u.K, 0.5 * u.eV / u.cm ** 3, pars[3] * u.rad]],
            Eemin=grid[0] * u.eV, Eemax=grid[1] * u.eV, nEed=grid[2])
        return IC.flux(data, distance=1 * u.kpc)

    def omodel(p, E):
        g = O.electron_grid(*grid)
        seeds = [O.thermal_seed("CMB"), dict(type="thermal", T=30.0, u=0.5 * O.ERG_PER_EV, theta=p[3])]
        return O.to_flux(O.ic_spectrum(E, g, O.nelec_on(_ecpl_o(p), g), seeds)[0], KPC), None

    prior, oprior = uniform([(20, 45), (1, 4), (-1, 3), (-3, 3)])
    p0 = np.array([33.0, 2.4, 1.3, 0.3])
    E = np.geomspace(2e11, 1e14, 40)
    raw = _data(omodel, p0, E, 51, "1/(cm2 s TeV)")
    pos = _spread(p0, NW, np.random.default_rng(52), [0.3, 0.04, 0.05, 0.4])
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m, steps=STEPS, seed=SEED)
            for m in MODES}
    th = runs["resident"]["chain"][:, :, 3]
    assert np.sum(th < 0) >= 3 and np.sum(th > 0) >= 3, th
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=_all_walkers(sum(STEPS)),
                 tag="D theta")
    same_chains(runs)


def _syn_ic(na, q):
    """Synchrotron + IC on the CMB, nEed 20; q(pars) -> dict(B [uG], Eemin [eV], Eemax [eV]),
    on the device's lazy parameters and on the oracle's numbers alike"""
    from oracle import naima_np as O
    u = na.u

    def model(pars, data):
        pd, v = _ecpl(na, pars), q(pars)
        kw = dict(Eemin=v["Eemin"] * u.eV, Eemax=v["Eemax"] * u.eV, nEed=20)
        SYN = na.Synchrotron(pd, B=v["B"] * u.uG, **kw)
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], **kw)
        return SYN.flux(data, distance=1 * u.kpc) + IC.flux(data, distance=1 * u.kpc)

    def omodel(p, E):
        pd, v = _ecpl_o(p), q(p)
        g = O.electron_grid(v["Eemin"], v["Eemax"], 20)
        ne = O.nelec_on(pd, g)
        sy = O.synchrotron_spectrum(E, g, ne, v["B"] * 1e-6)
        ic, _ = O.ic_spectrum(E, g, ne, [O.thermal_seed("CMB")])
        return O.to_flux(sy + ic, KPC), None

    return model, omodel


def test_loop_grid_limits_cross(na, monkeypatch):
    """Synchrotron + IC with Eemin = 10**p and Eemax = 10**q eV as fit parameters, started so
    close together that some walkers have Eemin > Eemax (asserted): a descending grid of 10 nodes
    and a spectrum of the opposite sign, which is what the reference computes"""
    model, omodel = _syn_ic(na, lambda p: dict(B=10 ** p[3], Eemin=10 ** p[4], Eemax=10 ** p[5]))
    prior, oprior = uniform([(20, 45), (1, 4), (-1, 3), (-1, 4), (9, 16), (9, 16)])
    p0 = np.array([33.0, 2.4, 1.5, 1.0, 13.0, 13.2])
    E = np.geomspace(1e-2, 1e13, 40)
    raw = _data(omodel, p0, E, 61)
    pos = _spread(p0, NW, np.random.default_rng(62), [0.3, 0.03, 0.05, 0.02, 0.5, 0.5])
    assert 3 <= np.sum(pos[:, 4] > pos[:, 5]) < NW
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m, steps=STEPS, seed=SEED)
            for m in MODES}
    c = runs["resident"]["chain"]
    inverted = c[:, :, 4] > c[:, :, 5]  # (sampled positions, not only proposals)
    assert np.sum(inverted) >= 3 and not inverted.all(), inverted
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=_all_walkers(sum(STEPS)),
                 tag="D limits cross")
    same_chains(runs)


def _replay(omodel, E, raw, oprior, pos):
    """the run's seeded move stream through oracle.stretch_move_reference with the oracle's own
    log-probability; where the oracle gives NaN or the reference's int() raises, the proposal is
    counted and rejected: (chain, final log-probability, proposals, NaN proposals)"""
    from naima_amd._lib import Moves
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    seen = dict(n=0, bad=0)

    def lnp(x, count=True):
        out = []
        for p in np.atleast_2d(x):
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                try:
                    lp = O.lnprobmodel(WN.to_data_repr(omodel(p, E)[0], raw), raw) + oprior(p)
                except (ValueError, OverflowError):
                    lp = np.nan
            if count:
                seen["n"] += 1
                seen["bad"] += int(np.isnan(lp))
            out.append(lp)
        return np.array(out)

    m = Moves(SEED, NW, 2.0, ksteps=32, depth=4)
    S, P, Z, L = [], [], [], []
    for n in STEPS:  # (the sampler takes the moves of each run_mcmc call on their own)
        addr, got = m.take(n)
        assert got == n
        for o, v in zip((S, P, Z, L), m.view(addr, got)):
            o.append(np.array(v))
    m.close()
    S, P, Z, L = [np.concatenate(o) for o in (S, P, Z, L)]
    c, l = pos.copy(), lnp(pos, count=False)
    assert np.all(np.isfinite(l))
    chain = []
    for k in range(sum(STEPS)):
        c, l, _ = O.stretch_move_reference(c, l, lnp, S[k], P[k], Z[k], L[k])
        chain.append(c.copy())
    return np.array(chain), l, seen


LINEAR = [
    # Eemin = p TeV: the reference's int() raises for p <= 0 (ValueError below 0, OverflowError at 0)
    ("Eemin", lambda p: dict(B=10 ** p[3], Eemin=p[4] * 1e12, Eemax=1e15)),
    # B = p uG: the reference's spectrum is NaN for p <= 0
    ("B", lambda p: dict(B=p[4], Eemin=1e11, Eemax=1e15)),
]


@pytest.mark.parametrize("case", LINEAR, ids=[c[0] for c in LINEAR])
def test_loop_linear_scalar_straddles_zero(na, monkeypatch, case):
    """Synchrotron + IC with Eemin [TeV] or B [uG] as the plain coordinate, started between 0.5 and
    30 without a prior against negative values (the pattern of test_nonpositive_energy): with
    nan_policy="reject" every mode counts exactly the proposals the oracle-driven sampler finds
    NaN on the same move stream, and its chain is that sampler's"""
    name, q = case
    model, omodel = _syn_ic(na, q)
    bounds = [(-1000.0, 1000.0)] * 5
    prior, oprior = uniform(bounds)
    p0 = np.array([33.0, 2.4, 1.5, 1.0, 10.0])
    E = np.geomspace(1e-2, 1e13, 40)
    raw = _data(omodel, p0, E, 71)
    rng = np.random.default_rng(31)
    pos = _spread(p0, NW, rng, [0.3, 0.03, 0.05, 0.02, 0.0])
    pos[:, 4] = np.geomspace(0.5, 30.0, NW)[rng.permutation(NW)]
    chain, l, seen = _replay(omodel, E, raw, oprior, pos)
    print("\n%s: %d of %d proposals are NaN for the oracle" % (name, seen["bad"], seen["n"]))
    assert seen["n"] == sum(STEPS) * NW and 3 <= seen["bad"] < seen["n"] / 2, seen
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m, steps=STEPS, seed=SEED,
                        nan_policy="reject") for m in MODES}
    for m, r in runs.items():
        assert r["nan"] == seen["bad"], (m, r["nan"], seen["bad"])
        assert np.all(np.isfinite(r["lp"])), m
        assert np.all(r["chain"][:, :, 4] > 0), m  # (no walker ever holds such a value)
        np.testing.assert_allclose(r["chain"], chain, rtol=1e-8, err_msg=m)
        np.testing.assert_allclose(r["lp"][-1], l, rtol=1e-6, err_msg=m)
    same_chains(runs)
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="D linear " + name)
