"""The device loops against the NumPy oracle at shapes the BASELINE workloads never reach.

test_gpu_loops.py holds the resident loop (k_half_step_run, nh_persist.hip), the one-launch
half-step (k_half_step, nh_halfstep.hip) and the separate kernels (NAIMA_AMD_MEGA=0, the
likelihood of nh_lnprob.h) to each other and to the host-driven loop, on the workloads' own data
and grids.  Here each of them is held to oracle/naima_np.py (plain float64, pinned to the
reference by test_oracle.py) on inputs built to reach the branches the workloads leave alone:

  L  the likelihood epilogues: asymmetric errors whose larger side alternates, data on both sides
     of the model, five upper limits spread through the table, a distinct cl per point, walkers
     that violate several different numbers of limits;
  S  the log-domain synchrotron comb (nh_syn2.h) at all four piece sizes m = 2, 4, 8, 16, the
     direct form on either side, the linear last piece below t = -46, weights that underflow, a
     grid shared with a table, and the three walker regimes of the resident loop;
  T  emission tables with whole tiles of columns beyond the particles' kinematic reach (exact
     zeros), with the rows in registers and streamed.

Every case runs a few steps of EnsembleSampler(device=True, naima_style=True, store_blobs=True)
across a run_mcmc boundary in every mode it names, asserts the path it was written for through
``_dev.resident_info``, asserts that the modes made the same accept decisions (the same chain),
and re-evaluates a sample of (step, walker) pairs of every mode with the oracle (check_oracle):

  * the model blob at rtol 1e-9 (the LUT pion mode 1e-7, as test_gpu_random.py), atol 1e-200 of
    the row's largest value; where the oracle gives an exact 0, the kernel must too;
  * a We blob at rtol 1e-10;
  * the log-probability of every mode to a bound PROPAGATED from the spectrum's tolerance,
        |d lp| <= sum_k |d_k| (rtol_model |m_k| + atol_k) / sigma_k^2 + 1e-12 |lp|,
    sigma_k the error naima picks (core.py:79-87: flux_error_hi where the model is above the
    data).  No sampled model lies within 1e-8 of an upper limit (asserted), so rounding cannot
    move a violation count.  With errors of 8 % and 25 % on alternating sides, picking the wrong
    side moves lp by O(1) per point, and cl one index off (cl = 0.5 + 0.007 k) moves it by
    ~0.014 per violated limit.  Measured against the bound (1e-6 .. 3e-5 here): lo / hi swapped
    in either epilogue, 40 .. 200 (L1, L2); cl[max(nviol - 1, 0)], 0.014 and 0.029.

The largest relative error each case measured is printed (pytest -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KPC = 3.0856775814913673e21
RT_MODEL, RT_LUT, RT_WE = 1e-9, 1e-7, 1e-10


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


# ------------------------------------------------------------------------------------ harness
MODES = {"resident": {}, "per-launch": {"NAIMA_AMD_RESIDENT": "0"},
         "separate": {"NAIMA_AMD_MEGA": "0"}}


def run_loop(na, monkeypatch, model, prior, raw, pos, mode="resident", env=None, steps=(3, 4),
             seed=5, nan_policy="raise"):
    """``steps[0]`` then ``steps[1]`` steps of the device loop in ``mode`` (resident: the default
    environment; per-launch: NAIMA_AMD_RESIDENT=0; separate: NAIMA_AMD_MEGA=0) ->
    dict(chain, lp, blobs (as arrays), units, info, launches, reason, mega, fused, and the
    sampler's nan_proposals and prior_forbidden_proposals)"""
    from naima_amd.datatable import make_data
    from naima_amd.sampler import EnsembleSampler
    for k in ("NAIMA_AMD_RESIDENT", "NAIMA_AMD_MEGA", "NH_RUN_RT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(MODES[mode], **(env or {})).items():
        monkeypatch.setenv(k, v)
    nw, nd = pos.shape
    s = EnsembleSampler(nw, nd, na.lnprob, args=[make_data(raw), model, prior], seed=seed,
                        naima_style=True, store_blobs=True, device=True, nan_policy=nan_policy)
    st = s.run_mcmc(pos, steps[0])
    s.run_mcmc(st, steps[1])
    dev = s._dev
    assert dev is not None
    if mode == "resident":
        print("\nresident_info (%s): %s" % (env or "", getattr(dev, "resident_info", None)))
    return dict(chain=s.get_chain(), lp=s.get_log_prob(),
                blobs=[np.asarray(b, dtype=float) for b in s.get_blobs()],
                units=list(s.blob_units or []), info=getattr(dev, "resident_info", None),
                launches=dev.resident_launches, reason=getattr(dev, "resident_reason", None),
                mega=dev.mega, fused=dev.fused, nan=s.nan_proposals,
                forbidden=s.prior_forbidden_proposals)


def sample_pairs(nsteps, nw, extra=5, seed=0):
    rng = np.random.default_rng(seed)
    ws = sorted(set([0, nw // 2, nw - 1] + rng.choice(nw, size=min(extra, nw), replace=False).tolist()))
    return [(s, w) for s in (0, nsteps - 1) for w in ws]


def _to(na, unit, target):
    return 1.0 if unit is None else float((1.0 * unit).to(target).value)


def _sigma(raw, model_repr):
    d = model_repr - raw["flux"]
    return d, np.where(d > 0, raw["flux_error_hi"], raw["flux_error_lo"])


def check_oracle(na, runs, raw, omodel, oprior, rt_model=RT_MODEL, lut=False, pairs=None,
                 tag=""):
    """the sampled (step, walker) positions of every run in ``runs`` re-evaluated with the oracle
    (each run at its own chain's positions: a fault in one mode shows as that mode's error, not
    only as chains that part).  omodel(p) -> (flux 1/(s cm2 eV), We erg or None).  Returns the
    oracle's (violation counts, error branches) over the pairs, for the cases' preconditions."""
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    ul = np.asarray(raw["ul"], dtype=bool)
    nu = ~ul
    nviols, branches = [], set()
    worst = dict(model=0.0, we=0.0, lp=0.0)
    cache = {}

    def oracle_at(p):
        key = p.tobytes()
        if key not in cache:
            flux, We = omodel(p)
            rep = WN.to_data_repr(flux, raw)
            lp_o = O.lnprobmodel(rep, raw) + oprior(p)
            d, sg = _sigma(raw, rep)
            if ul.any():  # (rounding must not be able to flip a violation)
                rel = np.abs(rep[ul] - raw["flux"][ul]) / np.abs(raw["flux"][ul])
                assert rel.min() > 1e-8, (tag, p, rel.min())
            # (the LUT mode's absolute tolerance propagated the same way)
            atol_rep = WN.to_data_repr(np.full(flux.shape, (1e-9 if lut else 1e-200) * np.max(np.abs(flux))), raw)
            bound = np.sum(np.abs(d[nu]) * (rt_model * np.abs(rep[nu]) + atol_rep[nu]) / sg[nu] ** 2) + \
                1e-12 * abs(lp_o)
            cache[key] = (flux, We, lp_o, bound, int(np.sum(rep[ul] > raw["flux"][ul])),
                          set((d[nu] > 0).tolist()))
        return cache[key]

    for mode, r in runs.items():
        nsteps, nw, _ = r["chain"].shape
        for (s, w) in (pairs or sample_pairs(nsteps, nw)):
            where = (tag, mode, s, w)
            flux, We, lp_o, bound, nviol, br = oracle_at(r["chain"][s, w])
            nviols.append(nviol)
            branches |= br
            row = r["blobs"][0][s, w] * _to(na, r["units"][0] if r["units"] else None,
                                           "1/(s cm2 eV)")
            zero = flux == 0.0
            assert np.all(row[zero] == 0.0), (where, np.nonzero(zero & (row != 0.0))[0])
            atol = (1e-9 if lut else 1e-200) * np.max(np.abs(flux))
            err = np.abs(row - flux)
            assert np.all(err <= atol + rt_model * np.abs(flux)), \
                (where, np.max(err / np.maximum(np.abs(flux), 1e-300)))
            big = np.abs(flux) > 1e-150 * np.max(np.abs(flux))  # (not the tails held by atol)
            worst["model"] = max(worst["model"], float(np.max(err[big] / np.abs(flux[big]))))
            if We is not None:
                got = float(r["blobs"][1][s, w]) * _to(na, r["units"][1] if len(r["units"]) > 1 else None, "erg")
                assert abs(got - We) <= RT_WE * abs(We), (where, got, We)
                worst["we"] = max(worst["we"], abs(got - We) / abs(We))
            lp = float(r["lp"][s, w])
            assert abs(lp - lp_o) <= bound, (where, lp, lp_o, bound)
            worst["lp"] = max(worst["lp"], abs(lp - lp_o) / bound)
    print("\n%s: largest relative error of the model (above 1e-150 of its peak) %.2e, of We %.2e; "
          "|d lp| / bound %.2e" % (tag, worst["model"], worst["we"], worst["lp"]))
    return nviols, branches


def same_chains(runs):
    ref = next(iter(runs.values()))
    for mode, r in runs.items():
        assert np.array_equal(r["chain"], ref["chain"]), mode  # (the same accept decisions)


def uniform(bounds):
    """(na prior, oracle prior) of independent uniform priors"""
    from oracle import naima_np as O

    def prior(pars):
        from naima_amd import uniform_prior
        return sum(uniform_prior(pars[i], lo, hi) for i, (lo, hi) in enumerate(bounds))

    def oprior(p):
        return float(sum(O.uniform_prior(p[i], lo, hi) for i, (lo, hi) in enumerate(bounds)))

    return prior, oprior


def make_raw(E_eV, true, flux_unit, rng, rel=(0.08, 0.25), uls=(), ul_factor=(), cl0=0.5,
             dcl=0.007, scatter=0.15, zero_below=1e-100):
    """a data table (plain arrays, make_data's input) around ``true`` (already in flux_unit):
    errors rel[0] / rel[1] below / above on even points, the other way round on odd ones; the
    points in ``uls`` upper limits at ul_factor x true; cl = cl0 + dcl k.  Points where the model
    is 0, or below ``zero_below`` of its largest value (an error whose square would underflow),
    get that fraction of the largest value as flux and error."""
    n = E_eV.size
    t = np.asarray(true, dtype=float).copy()
    zero = t <= zero_below * t.max()
    t[zero] = zero_below * t.max()
    even = np.arange(n) % 2 == 0
    lo = np.where(even, rel[0], rel[1]) * t
    hi = np.where(even, rel[1], rel[0]) * t
    flux = t * (1 + scatter * rng.standard_normal(n))
    flux[zero] = t[zero]
    lo[zero] = hi[zero] = t[zero]
    ul = np.zeros(n, dtype=bool)
    for i, f in zip(uls, ul_factor):
        ul[i] = True
        flux[i] = f * t[i]
        lo[i] = hi[i] = 0.0
    return dict(energy=E_eV, energy_unit="eV", flux=flux, flux_error_lo=lo, flux_error_hi=hi,
                ul=ul, cl=cl0 + dcl * np.arange(n), flux_unit=flux_unit)


def _repr(flux, E, flux_unit):
    if flux_unit == "erg/(cm2 s)":
        return flux * E ** 2 * 1.602176634e-12
    return flux * 1e12


# ------------------------------------------------------------------- the models of the cases
def _ecpl_o(p, beta=1.0):
    from oracle import naima_np as O
    return O.ParticleDist("ExponentialCutoffPowerLaw", amplitude=10 ** p[0], e_0=10e12, alpha=p[1],
                          e_cutoff=10 ** p[2] * 1e12, beta=beta)


def ic_only(na, grid):
    """IC on the CMB, pars: log10 amplitude, alpha, log10(cutoff / TeV); grid (Eemin, Eemax, nEed)"""
    from oracle import naima_np as O
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1], 10 ** pars[2] * u.TeV)
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=grid[0] * u.eV,
                               Eemax=grid[1] * u.eV, nEed=grid[2])
        return IC.flux(data, distance=1 * u.kpc)

    def omodel(p, E):
        g = O.electron_grid(*grid)
        ic, _ = O.ic_spectrum(E, g, O.nelec_on(_ecpl_o(p), g), [O.thermal_seed("CMB")])
        return O.to_flux(ic, KPC), None

    return model, omodel


def syn_ic(na, sgrid, igrid, beta=1.0):
    """Synchrotron + IC on the CMB with We > 1 TeV as a blob; pars: log10 amplitude, alpha,
    log10(cutoff / TeV), log10(B / uG)"""
    from oracle import naima_np as O
    u = na.u

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                          10 ** pars[2] * u.TeV, beta)
        SYN = na.Synchrotron(pd, B=10 ** pars[3] * u.uG, Eemin=sgrid[0] * u.eV,
                             Eemax=sgrid[1] * u.eV, nEed=sgrid[2])
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=igrid[0] * u.eV,
                               Eemax=igrid[1] * u.eV, nEed=igrid[2])
        return (SYN.flux(data, distance=1 * u.kpc) + IC.flux(data, distance=1 * u.kpc),
                IC.compute_We(Eemin=1 * u.TeV))

    def omodel(p, E):
        pd = _ecpl_o(p, beta)
        gs, gi = O.electron_grid(*sgrid), O.electron_grid(*igrid)
        sy = O.synchrotron_spectrum(E, gs, O.nelec_on(pd, gs), 10 ** p[3] * 1e-6)
        ic, _ = O.ic_spectrum(E, gi, O.nelec_on(pd, gi), [O.thermal_seed("CMB")])
        We = O.electron_energy_content(pd, O.electron_grid(1e12, igrid[1], igrid[2]))
        return O.to_flux(sy + ic, KPC), We

    return model, omodel


def _spread(p0, nw, rng, widths):
    return p0 + np.asarray(widths) * rng.uniform(-1, 1, (nw, len(p0)))


# ------------------------------------------------------------------------- L: the likelihood
def _nviol_preconditions(nviols, branches):
    assert len(set(nviols)) >= 3, sorted(set(nviols))  # (several violation counts ...)
    assert branches == {True, False}  # (... and both sides of the error model)


def test_likelihood_epilogues_table_only(na, monkeypatch):
    """L1: IC on the CMB (table-only instance, cfg1-like) on a differential-flux table of 90
    points -- the resident epilogue's k += 64 loop takes two passes -- with asymmetric errors
    whose larger side alternates, data scattered on both sides, five upper limits spread through
    the energy range and cl = 0.5 + 0.007 k.  The walkers' amplitudes span a decade, so the
    oracle counts at least three different numbers of violated limits among the sampled walkers
    (asserted).  The resident loop keeps the table's rows in registers.  Resident loop, one launch
    per half-step and the separate likelihood kernel are each held to the oracle's
    log-probability to the propagated bound (module docstring)."""
    grid = (1e11, 1e15, 60)
    model, omodel = ic_only(na, grid)
    prior, oprior = uniform([(20, 40), (1, 4), (-1, 3)])
    p0 = np.array([33.0, 2.4, 1.3])
    E = np.geomspace(2e11, 1e14, 90)
    rng = np.random.default_rng(11)
    true = _repr(omodel(p0, E)[0], E, "1/(cm2 s TeV)")
    uls = (6, 27, 45, 66, 88)
    raw = make_raw(E, true, "1/(cm2 s TeV)", rng, uls=uls, ul_factor=(0.6, 0.9, 1.4, 2.0, 2.8))
    nw = 16
    pos = _spread(p0, nw, np.random.default_rng(12), [0.5, 0.04, 0.05])
    pos[:, 0] += 0.1
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    r = runs["resident"]
    assert r["launches"] > 0, r["reason"]
    assert r["info"]["tables_in_registers"], r["info"]
    assert not runs["per-launch"]["launches"] and runs["per-launch"]["mega"]
    assert not runs["separate"]["mega"]
    nviols, branches = check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="L1")
    same_chains(runs)
    _nviol_preconditions(nviols, branches)


def test_likelihood_epilogues_sed_two_walkers_in_flight(na, monkeypatch):
    """L2: the same features on an SED table (erg/(cm2 s), 90 points from 1e-6 eV to 50 TeV)
    with a synchrotron + IC model: the resident loop's 1024-thread instance, at 1024 walkers --
    512 per half-step, more than the launch's workgroups: two walkers in flight."""
    model, omodel = syn_ic(na, (1e9, 1e15, 60), (1e11, 1e15, 80))
    prior, oprior = uniform([(20, 45), (1, 4), (-1, 3), (-1, 4)])
    p0 = np.array([33.0, 2.4, 1.5, 1.0])
    E = np.geomspace(1e-6, 5e13, 90)
    rng = np.random.default_rng(21)
    true = _repr(omodel(p0, E)[0], E, "erg/(cm2 s)")
    raw = make_raw(E, true, "erg/(cm2 s)", rng, uls=(4, 30, 52, 71, 89),
                   ul_factor=(0.6, 0.9, 1.4, 2.0, 2.8))
    nw = 1024
    pos = _spread(p0, nw, np.random.default_rng(22), [0.5, 0.03, 0.05, 0.02])
    pos[:, 0] += 0.1
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    info = runs["resident"]["info"]
    assert runs["resident"]["launches"] > 0, runs["resident"]["reason"]
    assert info["threads"] == 1024 and info["two_walkers_in_flight"], info
    assert info["syn_log_domain"], info
    nviols, branches = check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="L2")
    same_chains(runs)
    _nviol_preconditions(nviols, branches)


# ------------------------------------------------------------- S: the synchrotron comb
def _comb(p, E, grid):
    """(Z, live, x at the grid's last node) per energy for walker p, by hs_s2_prepare's
    arithmetic: node i of energy E sits z + i comb steps below T_top = 7, z = (7 - ln x_0) / (2 lx),
    Z = floor(z); the energy is live where x <= 746 at the last node"""
    from oracle import naima_np as O
    g = O.electron_grid(*grid)
    B = 10 ** p[3] * 1e-6
    Ec = 3 * O.E_GAUSS * O.HBAR_CGS * B * g ** 2 / (2 * O.M_E_G * O.C_CGS)
    x0 = E * O.ERG_PER_EV / Ec[0]
    lx = np.log(g[-1] / g[0]) / (g.size - 1)
    Z = np.floor((7.0 - np.log(x0)) / (2 * lx)).astype(np.int64)
    xl = E * O.ERG_PER_EV / Ec[-1]
    return Z, xl <= 746.0, xl


# (id, (Eemin, Eemax, nEed) of the synchrotron grid, IC grid ("same", or None: 100 GeV .. 1 PeV,
#  nEed 40), walkers, nodes per piece (0: the direct form), data energies, ECPL beta, the walker
#  regime asserted: K = at least K workgroups per walker, "one" = one per CU, "two" = two walkers
#  in flight, None = not asserted)
E_WIDE = np.geomspace(1e-7, 3e13, 100)
E_DEEP = np.geomspace(1e-24, 3e13, 100)
S_CASES = [
    ("m2-split", (1e9, 1e15, 60), None, 16, 2, E_WIDE, 1.0, 2),
    ("m4-one-per-cu", (1e12, 1e15, 120), None, 512, 4, E_WIDE, 1.0, "one"),
    ("m8-two-in-flight", (1e13, 1e15, 240), None, 1024, 8, E_WIDE, 1.0, "two"),
    ("m16-split4", (1e13, 3e14, 480), None, 8, 16, E_WIDE, 1.0, 4),
    ("direct-30", (1e9, 510998.95e9, 30), None, 16, 0, E_WIDE, 1.0, None),
    ("direct-800", (1e14, 5e14, 800), None, 16, 0, E_WIDE, 1.0, 2),
    ("below-tbot", (1e9, 1e15, 100), None, 16, 4, E_DEEP, 1.0, 2),
    ("underflow-beta2", (1e9, 1e15, 100), None, 16, 4, E_WIDE, 2.0, 2),
    ("shared-grid", (1e11, 1e14, 100), "same", 16, 4, E_WIDE, 1.0, 2),
]


@pytest.mark.parametrize("case", S_CASES, ids=[c[0] for c in S_CASES])
def test_synchrotron_comb(na, monkeypatch, case):
    """S: Synchrotron + IC with log10 B a fit parameter, the walkers' fields spread over three
    decades (1 uG .. 1 mG), data from 1e-7 eV (1e-24 eV for below-tbot) to 30 TeV: along one row
    the synchrotron spectrum is live, partly live and dead.  The comb's piece size follows from
    hs_s2_prepare: lm = rint(log2(0.16 / (2 lx))), lx = ln(Eemax / Eemin) / (nG - 1), so nEed 60,
    120, 240, 480 give m = 2, 4, 8, 16, and nEed 30 and 800 (lm = 0 and 5) the direct form
    (hs_syn_item).  Asserted through resident_info:

      m2-split          m = 2,   8 walkers per half-step: workgroups_per_walker >= 2
      m4-one-per-cu     m = 4,   256 per half-step, about one per CU: one workgroup each,
                        not two in flight
      m8-two-in-flight  m = 8,   512 per half-step: two walkers in flight
      m16-split4        m = 16 on 10 .. 300 TeV (1.5 decades, nG = 709; on 1 TeV .. 1 PeV, nG =
                        1440, the library declines: "hs_run_create: the resident loop's working
                        set does not fit in LDS"), 4 walkers per half-step:
                        workgroups_per_walker >= 4 (tcompact).  A chunk
                        starts on a piece boundary, so the last chunk of energy E walks
                        n = (Z + nG) mod 16 nodes past its last whole piece (Z = floor(z), _comb);
                        where that is 1 its final piece runs the full 15 nodes into the 16 guard
                        nodes (HS_S2_GUARD).  Z moves by ln(10) / (2 lx) = 240 comb steps per
                        decade of E, so across 100 energies and a spread of fields every residue
                        occurs: the test asserts sampled (walker, energy) pairs with the overrun.
                        1e-3 added to c[0] of the table's middle piece (7e-7 of the integrand
                        there) shows as a 1.2e-7 error of the spectrum.
      direct-30 / -800  syn_log_domain False
      below-tbot        data down to 1e-24 eV: x = E / Ec < e^-50 at the grid's top nodes
                        (asserted), the clamp to the linear last piece (pe = min(p, P)).  The
                        last table piece's polynomial, continued below t = -46, leaves the
                        linear form only slowly (3.6e-4 / Lambda at t = -49, 3e-2 at -54), so the
                        nodes below -50 have to carry weight: an index of 0.3 and a cut-off at
                        200 TeV give them most of the lowest energy's integral
                        (asserted: > 1 % for some sampled walker).  With data down to 1e-15 eV
                        and an index of 2.3 the clamp to piece P - 1 changed nothing the test
                        could see; down to 1e-18 eV and an index of 0.3, 3e-10; to 1e-21 eV, 9e-9.
      underflow-beta2   ECPL with beta = 2 and a cut-off of 0.3 .. 3 TeV against Eemax = 1 PeV:
                        the top of the grid's weights underflow to exact zeros (asserted on the
                        oracle's weights), the log-domain floor (HS_S2_FLOOR / s2_lnw0)
      shared-grid       Syn and IC on one grid (same Eemin / Eemax / nEed): the plan then has a
                        table on the synchrotron grid, so the resident loop keeps separate comb
                        arrays (s2_own == 0; not visible through the ABI -- it follows from the
                        shared grid: nh_persist.hip sets s2_own only when no table reads it)

    Resident loop and one launch per half-step (and the separate kernels, for the chain) against
    the oracle."""
    from oracle import naima_np as O
    cid, sgrid, igrid, nw, m, E, beta, regime = case
    igrid = sgrid if igrid == "same" else (1e11, 1e15, 40)
    model, omodel = syn_ic(na, sgrid, igrid, beta)
    prior, oprior = uniform([(20, 45), (-1, 4), (-2, 3), (-0.5, 3.5)])
    p0 = np.array([33.0, 2.3, 1.2 if beta == 1.0 else 0.0, 1.5])
    if cid == "below-tbot":  # (a hard spectrum up to 200 TeV: the grid's top decades carry weight)
        p0 = np.array([31.0, 0.3, 2.3, 1.5])
    rng = np.random.default_rng(len(cid) * 7 + nw)
    true = _repr(omodel(p0, E)[0], E, "erg/(cm2 s)")
    raw = make_raw(E, true, "erg/(cm2 s)", rng, rel=(0.05, 0.05), scatter=0.05, cl0=0.9, dcl=0.0)
    pos = _spread(p0, nw, np.random.default_rng(31), [0.1, 0.05, 0.5, 1.5])
    modes = ("resident", "per-launch", "separate")
    runs = {md: run_loop(na, monkeypatch, model, prior, raw, pos, md) for md in modes}
    r = runs["resident"]
    info = r["info"]
    assert r["launches"] > 0, r["reason"]
    assert info["syn_log_domain"] == (m > 0), info
    if m:
        assert info["syn_nodes_per_piece"] == m, info
    if regime == "one":  # (nw / 2 = 256 walkers per half-step, one per CU)
        assert info["workgroups_per_walker"] == 1 and not info["two_walkers_in_flight"], info
    elif regime == "two":  # (512 per half-step)
        assert info["two_walkers_in_flight"], info
    elif regime is not None:  # (fewer walkers per half-step than CUs)
        assert info["workgroups_per_walker"] >= regime and not info["two_walkers_in_flight"], info
    nsteps = r["chain"].shape[0]
    pairs = sample_pairs(nsteps, nw)
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=pairs, tag="S " + cid)
    same_chains(runs)
    # the preconditions of the case, on the sampled positions
    chain = r["chain"]
    if cid == "m16-split4":
        g = O.electron_grid(*sgrid)
        assert g.size == 709
        over = 0
        for s, w in pairs:
            Z, live, _ = _comb(chain[s, w], E, sgrid)
            over += int(np.sum(live & ((Z + g.size) % 16 == 1)))
        assert over > 0
    if cid == "below-tbot":
        g = O.electron_grid(*sgrid)
        share = []
        for s, w in pairs:
            p = chain[s, w]
            x = E[0] * O.ERG_PER_EV / (3 * O.E_GAUSS * O.HBAR_CGS * 10 ** p[3] * 1e-6 * g ** 2
                                       / (2 * O.M_E_G * O.C_CGS))
            seg = O.trapz_loglog(O.nelec_on(_ecpl_o(p), g) * O.gtilde(x), g, intervals=True)
            share.append(seg[x[1:] < np.exp(-50.0)].sum() / seg.sum())
        assert max(share) > 0.01, share
    if cid == "underflow-beta2":
        g = O.electron_grid(*sgrid)
        for s, w in pairs:
            ne = O.nelec_on(_ecpl_o(chain[s, w], beta), g)
            assert ne[0] > 0 and ne[-1] == 0.0, chain[s, w]
    # more than a decade of the field among the sampled walkers
    Bs = [chain[s, w][3] for s, w in pairs]
    assert max(Bs) - min(Bs) > 1.0


# ------------------------------------------------------------------- T: table edges
def _table_case(na, kind):
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    u = na.u
    if kind == "ic":
        grid = (1e9, 1e13, 100)
        model, omodel = ic_only(na, grid)
        E = np.concatenate([np.geomspace(1e11, 8e12, 30), np.geomspace(1.2e13, 1e15, 70)])
        return model, (lambda p: omodel(p, E)), E, False
    if kind.startswith("pion"):
        lut = kind == "pion-lut"
        Epmin = O.M_P_GEV + O.T_TH_GEV + 1e-4
        Epmax = 1e4  # GeV: nothing above ~10 TeV

        def model(pars, data):
            pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1],
                                              10 ** pars[2] * u.TeV)
            PP = na.PionDecay(pd, nh=1.0 / u.cm ** 3, useLUT=lut, Epmax=Epmax * u.GeV, nEpd=25)
            return PP.flux(data, distance=1 * u.kpc)

        E = np.concatenate([np.geomspace(1e10, 5e12, 30), np.geomspace(1.1e13, 1e15, 70)])

        def omodel(p):
            Ep = O.proton_grid(Epmin, Epmax, 25)
            J = O.J_on(_ecpl_o(p), Ep)
            sp = O.pion_spectrum(E, Ep, J, 1.0, diffsigma=WN.get_lut() if lut else None)
            return O.to_flux(sp, KPC), None

        return model, omodel, E, lut
    # (a nEed other than the class's 300; 100 nodes, so that the rows fit the registers)
    grid = (1e12, 1e14, 50)

    def model(pars, data):
        pd = na.ExponentialCutoffPowerLaw(10 ** pars[0] / u.eV, 10 * u.TeV, pars[1], 10 ** pars[2] * u.TeV)
        BR = na.Bremsstrahlung(pd, n0=1.0 / u.cm ** 3, Eemin=grid[0] * u.eV, Eemax=grid[1] * u.eV,
                               nEed=grid[2])
        return BR.flux(data, distance=1 * u.kpc)

    E = np.concatenate([np.geomspace(1e11, 5e13, 30), np.geomspace(2e14, 1e16, 70)])

    def omodel(p):
        g = O.electron_grid(*grid)
        return O.to_flux(O.brems_spectrum(E, g, O.nelec_on(_ecpl_o(p), g), n0=1.0), KPC), None

    return model, omodel, E, False


@pytest.mark.parametrize("kind", ["ic", "pion-lut", "pion-analytic", "bremsstrahlung"])
def test_table_columns_beyond_reach(na, monkeypatch, kind):
    """T: 70 of 100 photon energies beyond the particles' kinematic reach -- IC above Eemax =
    10 TeV, pi0 decay above what Epmax = 10 TeV makes, bremsstrahlung above Eemax = 100 TeV on a
    grid of nEed 50 -- so whole 64-column tiles of the sorted emission table are exact zeros
    (their first non-zero row is nG).  The resident loop with the rows in registers
    (NH_RUN_RT=1) and streamed (NH_RUN_RT=0), one launch per half-step and the separate kernels:
    the zero columns come back as exact 0.0 (the oracle's exact zeros; the LUT mode's spline is
    not 0 there and is held to its tolerance), the rest to the oracle's values."""
    model, omodel, E, lut = _table_case(na, kind)
    prior, oprior = uniform([(20, 60), (1, 4), (-1, 3)])
    p0 = np.array([46.0 if kind.startswith("pion") else 33.0, 2.3, 1.0])
    f0 = omodel(p0)[0]
    nzero = int(np.sum(f0 == 0.0))
    assert nzero >= (0 if lut else 64), nzero
    rng = np.random.default_rng(41)
    true = _repr(f0, E, "1/(cm2 s TeV)")
    # (the LUT's spline is not 0 beyond the reach: there the data sit at 1e-6 of the peak, so
    # that the spectrum's absolute tolerance stays a small part of the likelihood)
    raw = make_raw(E, true, "1/(cm2 s TeV)", rng, zero_below=1e-6 if lut else 1e-100)
    nw = 16
    pos = _spread(p0, nw, np.random.default_rng(42), [0.05, 0.05, 0.1])
    runs = {}
    for rt in ("1", "0"):
        r = run_loop(na, monkeypatch, model, prior, raw, pos, "resident", env={"NH_RUN_RT": rt})
        assert r["launches"] > 0, r["reason"]
        assert r["info"]["tables_in_registers"] == (rt == "1"), r["info"]
        runs["resident-rt" + rt] = r
    for md in ("per-launch", "separate"):
        runs[md] = run_loop(na, monkeypatch, model, prior, raw, pos, md)
    check_oracle(na, runs, raw, omodel, oprior, rt_model=RT_LUT if lut else RT_MODEL, lut=lut,
                 tag="T " + kind)
    same_chains(runs)
