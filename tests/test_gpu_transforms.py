"""The three device loops under the parameter transforms a model may write.

Whatever arithmetic a model function does on ``pars[i]`` reaches the loops as ``a * tf(b x + c)``
(naima_amd/darray.py).  The resident loop (nh_persist_phase_a.inc) has a fast path for "every column
is the identity or a power of ten of its coordinate" and a second path, chosen by a wave-wide
ballot, for everything else (hsr_lazy_apply, then a library logarithm behind it for ln e_0,
ln e_cutoff, ln e_break and ln |amplitude|); the one-launch half-step (nh_halfstep.hip) and the
separate kernels' front (nh_core.hip) evaluate nh_lazy_apply.  Every other test, example and
workload writes ``pars[k]`` and ``10 ** pars[k]`` only, and every energy as a constant or a power
of ten.  Here the models of test_gpu_shapes.py's L1 (IC on the CMB: the 512-thread table-only
instance) and L2 (synchrotron + IC with We: the 1024-thread instance with the log-domain
synchrotron items) are REPARAMETERISED -- the same physical parameters, data table and grids, so
the oracle's preconditions are the ones known to hold -- and run with test_gpu_shapes.py's
harness: 3 + 4 steps across a run_mcmc boundary in the modes resident / per-launch / separate,
the same chain in all three, sampled (step, walker) pairs re-evaluated by oracle/naima_np.py
at the project's tolerances (model 1e-9, We 1e-10, log-probability to check_oracle's propagated
bound).  The SAME Python expression gives the device model its parameters (on ``DVec``s) and the
oracle its numbers (on floats).  Every case asserts the loop it ran (assert_loops).

Non-positive energies (test_nonpositive_energy).  ``e_cutoff = pars[2] * u.TeV`` without a prior
lets a stretch move propose a negative energy.  The batched weights kernels took ``ln e = 0`` for
any energy that is not positive -- meant for the slots a distribution leaves unused -- so such a
walker was evaluated as if the energy were 1 eV and got a finite log-probability.  Now an energy
the distribution USES that is zero, negative or NaN makes the spectrum and the log-probability NaN
(pd_ln_default, nh_pdist.h) in all three loops, which the sampler's nan_policy then counts or raises.
The oracle gives NaN for e_0 < 0 and for e_cutoff < 0 with beta = 1.5, and finite numbers for
e_cutoff < 0 with beta = 1 and for e_break < 0 with an integer alpha_2 - alpha_1: there the loop
gives NaN as well (the documented choice, README), and the oracle-driven sampler the chain is
compared with treats every proposal with a non-positive used energy as NaN.

prior_forbidden_proposals (test_priors_on_transformed_values).  Only the one-launch kernels
counted the proposals the prior forbids; under NAIMA_AMD_MEGA=0, and in the first half-steps of
any run, the counter stayed behind ({'per-launch': 14, 'resident': 14, 'separate': 0}).  The
separate kernels' accepts count them now (nh_forbidden_count), so the number is the run's, not
the path's.

Measured on an MI355X (pytest -s; profiles/NOTES_transforms.md): over all cases the model's largest
relative error is 9.3e-12 ([log-of-pow]; 5.6e-10 for [nonpositive ecut-beta1.5], beta = 1.5 with
cut-offs down to 0.5 TeV) against 1e-9, We 1.5e-13 against 1e-10, |d lp| / bound 1.7e-4.

Before the fix (the parent's kernels) all four test_nonpositive_energy cases fail at
``assert r["nan"] == seen["bad"]``: ('resident', 0, 10), ('resident', 0, 15), ('resident', 0, 16),
('resident', 0, 13) -- the loop counted no NaN proposal where 10 .. 16 had a non-positive energy.

Mutation checks (by hand, on scratch copies of the library; the existing tests named ran with
each and passed: test_gpu_shapes.py's two likelihood cases, test_gpu_loops.py's
test_device_loop_equals_oracle_driven_sampler*, test_resident_loop_equals_per_launch_loop and
test_two_walkers_in_flight_changes_no_bit, 26 tests):
  * ``c`` dropped in the resident loop's pack path (xl = zb * qv): [affine] fails in same_chains
    ("AssertionError: per-launch": with an amplitude 1e30 too large the resident loop accepts
    nothing, so what it stored is the start, which the oracle confirms -- the chains say it);
  * ``hsr_log(fabs(val))`` replaced by 0: [exp-table-only], [exp-syn+tables],
    [identity-energy-table-only] and [identity-energy-syn+tables] fail in check_oracle
    ((('X exp-table-only', 'resident', 6, 7), 1.0): the model off by 100 %);
  * a prior term on the raw coordinate in the resident loop (nh_persist_priors.inc):
    test_priors_on_transformed_values fails in same_chains ("AssertionError: per-launch");
  * the LOG and SQRT labels of nh_lazy_apply swapped: [square-sqrt-recip] and
    [mixed-wave-syn+tables] fail (the per-launch and separate loops).
"""
import warnings

import numpy as np
import pytest

from test_gpu_shapes import (KPC, MODES, _repr, _spread, check_oracle, make_raw, run_loop,
                             same_chains, uniform)

pytestmark = pytest.mark.gpu

IC_GRID = (1e11, 1e15, 60)  # L1
SYN_GRID, SIC_GRID = (1e9, 1e15, 60), (1e11, 1e15, 80)  # L2
KINDS = {"ECPL": "ExponentialCutoffPowerLaw", "BPL": "BrokenPowerLaw",
         "ECBPL": "ExponentialCutoffBrokenPowerLaw"}


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


# ------------------------------------------------------------------------------- the models
def build(na, kind, syn, q):
    """the L1 (syn False) or L2 (syn True) model with the particle distribution ``kind`` and the
    parameters q(pars) -> dict(A 1/eV, e0 TeV (default 10), a1, a2, ec TeV, beta (default 1), eb
    TeV, B uG): (device model, oracle model(p, E) -> (flux, We))"""
    from oracle import naima_np as O
    u = na.u

    def model(pars, data):
        p = q(pars)
        A, e0 = p["A"] / u.eV, p.get("e0", 10.0) * u.TeV
        if kind == "ECPL":
            pd = na.ExponentialCutoffPowerLaw(A, e0, p["a1"], p["ec"] * u.TeV, p.get("beta", 1.0))
        elif kind == "BPL":
            pd = na.BrokenPowerLaw(A, e0, p["eb"] * u.TeV, p["a1"], p["a2"])
        else:
            pd = na.ExponentialCutoffBrokenPowerLaw(A, e0, p["eb"] * u.TeV, p["a1"], p["a2"],
                                                    p["ec"] * u.TeV, p.get("beta", 1.0))
        g = SIC_GRID if syn else IC_GRID
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=g[0] * u.eV,
                               Eemax=g[1] * u.eV, nEed=g[2])
        if not syn:
            return IC.flux(data, distance=1 * u.kpc)
        SYN = na.Synchrotron(pd, B=p["B"] * u.uG, Eemin=SYN_GRID[0] * u.eV,
                             Eemax=SYN_GRID[1] * u.eV, nEed=SYN_GRID[2])
        return (SYN.flux(data, distance=1 * u.kpc) + IC.flux(data, distance=1 * u.kpc),
                IC.compute_We(Eemin=1 * u.TeV))

    def opd(p):
        v = q(p)
        kw = dict(amplitude=float(v["A"]), e_0=float(v.get("e0", 10.0)) * 1e12)
        if kind == "ECPL":
            kw.update(alpha=float(v["a1"]))
        else:
            kw.update(alpha_1=float(v["a1"]), alpha_2=float(v["a2"]), e_break=float(v["eb"]) * 1e12)
        if kind != "BPL":
            kw.update(e_cutoff=float(v["ec"]) * 1e12, beta=float(v.get("beta", 1.0)))
        return O.ParticleDist(KINDS[kind], **kw)

    def omodel(p, E):
        pd = opd(p)
        gi = O.electron_grid(*(SIC_GRID if syn else IC_GRID))
        ic, _ = O.ic_spectrum(E, gi, O.nelec_on(pd, gi), [O.thermal_seed("CMB")])
        if not syn:
            return O.to_flux(ic, KPC), None
        gs = O.electron_grid(*SYN_GRID)
        sy = O.synchrotron_spectrum(E, gs, O.nelec_on(pd, gs), float(q(p)["B"]) * 1e-6)
        We = O.electron_energy_content(pd, O.electron_grid(1e12, SIC_GRID[1], SIC_GRID[2]))
        return O.to_flux(sy + ic, KPC), We

    return model, omodel


def data_for(omodel, p0, syn, seed, uls=True, negate=False):
    """L1's differential-flux table (90 points, five upper limits) or L2's SED table around the
    model at p0"""
    rng = np.random.default_rng(seed)
    if syn:
        E, fu, ul = np.geomspace(1e-6, 5e13, 90), "erg/(cm2 s)", (4, 30, 52, 71, 89)
    else:
        E, fu, ul = np.geomspace(2e11, 1e14, 90), "1/(cm2 s TeV)", (6, 27, 45, 66, 88)
    true = _repr(omodel(p0, E)[0], E, fu)
    if negate:
        raw = make_raw(E, -true, fu, rng)
        raw["flux"] = -raw["flux"]
        return E, raw
    return E, make_raw(E, true, fu, rng, uls=ul if uls else (),
                       ul_factor=(0.6, 0.9, 1.4, 2.0, 2.8) if uls else ())


def assert_loops(runs, syn, two=None):
    """each mode ran the loop it names: the resident loop launched (512 threads with the table's
    rows in registers for the table-only model; 1024 threads with the log-domain synchrotron
    items for synchrotron + IC), NAIMA_AMD_RESIDENT=0 ran one launch per half-step, and
    NAIMA_AMD_MEGA=0 the separate kernels behind nh_step_front"""
    r = runs["resident"]
    assert r["launches"] > 0 and r["mega"] and r["fused"], (r["reason"], r["mega"], r["fused"])
    info = r["info"]
    if syn:
        assert info["threads"] == 1024 and info["syn_log_domain"], info
    else:
        assert info["threads"] == 512 and info["tables_in_registers"], info
    if two is not None:
        assert bool(info["two_walkers_in_flight"]) == two, info
    p = runs["per-launch"]
    assert not p["launches"] and p["mega"] and p["fused"], p["reason"]
    s = runs["separate"]
    assert not s["launches"] and not s["mega"] and s["fused"], s["reason"]


def ln(x):
    return float(np.log(x))


# (id, kind, syn, q, p0, spread, prior bounds, walkers)
CASES = [
    # natural-log walk: amplitude, cut-off and field are exp() of their coordinates
    ("exp-table-only", "ECPL", False,
     lambda p: dict(A=np.exp(p[0]), a1=p[1], ec=np.exp(p[2])),
     [ln(1e33), 2.4, ln(20.0)], [1.0, 0.04, 0.1], [(40, 110), (1, 4), (-3, 8)], 16),
    ("exp-syn+tables", "ECPL", True,
     lambda p: dict(A=np.exp(p[0]), a1=p[1], ec=np.exp(p[2]), B=np.exp(p[3])),
     [ln(1e33), 2.4, ln(30.0), ln(10.0)], [1.0, 0.03, 0.1, 0.05],
     [(40, 110), (1, 4), (-3, 8), (-3, 10)], 16),
    ("exp-syn+tables-two-in-flight", "ECPL", True,
     lambda p: dict(A=np.exp(p[0]), a1=p[1], ec=np.exp(p[2]), B=np.exp(p[3])),
     [ln(1e33), 2.4, ln(30.0), ln(10.0)], [1.0, 0.03, 0.1, 0.05],
     [(40, 110), (1, 4), (-3, 8), (-3, 10)], 1024),
    # identity values that still need the logarithm: e_cutoff, e_0 and the amplitude
    ("identity-energy-table-only", "ECPL", False,
     lambda p: dict(A=p[0] * 1e33, a1=p[1], ec=p[2], e0=p[3]),
     [1.0, 2.4, 20.0, 10.0], [0.3, 0.04, 1.0, 1.0], [(1e-3, 100), (1, 4), (1, 200), (1, 100)], 16),
    ("identity-energy-syn+tables", "ECPL", True,
     lambda p: dict(A=p[0] * 1e33, a1=p[1], ec=p[2], e0=p[3], B=p[4]),
     [1.0, 2.4, 30.0, 10.0, 10.0], [0.3, 0.03, 1.5, 1.0, 0.5],
     [(1e-3, 100), (1, 4), (1, 200), (1, 100), (0.1, 100)], 16),
    # e_cutoff = x**2, e_break = sqrt(x) (column 5 live), B = 1 / x
    ("square-sqrt-recip", "ECBPL", True,
     lambda p: dict(A=10 ** p[0], a1=p[1], a2=p[1] + 1.0, ec=p[2] ** 2, B=1 / p[3],
                    eb=np.sqrt(p[4])),
     [33.0, 2.0, 30.0 ** 0.5, 0.1, 9.0], [0.3, 0.03, 0.1, 0.002, 0.5],
     [(20, 45), (0, 4), (1, 20), (1e-3, 1), (0.1, 100)], 16),
    # affine arguments, one coordinate in two columns, one in none, beta a coordinate
    ("affine", "ECBPL", False,
     lambda p: dict(A=10 ** (2 * p[0] - 30), a1=p[1] + 0.5, a2=p[1] + 1.5, eb=3.0,
                    ec=10 ** p[2], beta=p[3]),
     [31.5, 1.9, 1.3, 1.0, 0.7], [0.15, 0.04, 0.05, 0.05, 0.3],
     [(20, 45), (0, 4), (-1, 3), (0.2, 3), (-5, 5)], 16),
    # one odd column among powers of ten: the ballot sends the whole wave down the second path
    ("mixed-wave-table-only", "ECPL", False,
     lambda p: dict(A=10 ** p[0], a1=1 / p[1], ec=10 ** p[2]),
     [33.0, 1 / 2.4, 1.3], [0.5, 0.007, 0.05], [(20, 40), (0.2, 1), (-1, 3)], 16),
    ("mixed-wave-syn+tables", "ECPL", True,
     lambda p: dict(A=10 ** p[0], a1=p[1], ec=10 ** p[2], B=np.sqrt(p[3])),
     [33.0, 2.4, 1.5, 100.0], [0.5, 0.03, 0.05, 10.0], [(20, 45), (1, 4), (-1, 3), (1, 1e4)], 16),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_transformed_parameters(na, monkeypatch, case):
    """the loops on models whose columns are not powers of ten of their coordinates (CASES)"""
    cid, kind, syn, q, p0, widths, bounds, nw = case
    p0 = np.array(p0)
    model, omodel = build(na, kind, syn, q)
    prior, oprior = uniform(bounds)
    E, raw = data_for(omodel, p0, syn, 100 + len(cid))
    pos = _spread(p0, nw, np.random.default_rng(12), widths)
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    assert_loops(runs, syn, two=(nw == 1024))
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="X " + cid)
    same_chains(runs)
    chain = runs["resident"]["chain"]
    assert np.any(chain[-1] != chain[0])  # (something was accepted)


def test_values_that_do_not_fold_onto_a_coordinate(na, monkeypatch):
    """[log-of-pow]: ``10 ** np.log10(10 ** pars[2])`` (a transform of a transform) and
    ``pars[1] * pars[3]`` (a product of two coordinates) are produced by eager kernels into buffers
    outside the proposal block, so the recorded half-step cannot become nh_step_front's
    (_record_half_step returns before ``fused``): in every mode the loop stays on its recorded launch
    sequence -- asserted -- and that loop is held to the oracle just the same"""
    q = lambda p: dict(A=10 ** p[0], a1=p[1] * p[3], ec=10 ** np.log10(10 ** p[2]))
    p0 = np.array([33.0, 2.4, 1.3, 1.0])
    model, omodel = build(na, "ECPL", False, q)
    prior, oprior = uniform([(20, 40), (1, 4), (-1, 3), (0.5, 2)])
    E, raw = data_for(omodel, p0, False, 7)
    pos = _spread(p0, 16, np.random.default_rng(12), [0.5, 0.04, 0.05, 0.01])
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    for m, r in runs.items():
        assert not r["fused"] and not r["mega"] and not r["launches"], (m, r["reason"])
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="X log-of-pow")
    same_chains(runs)


def test_priors_on_transformed_values(na, monkeypatch):
    """[priors]: the three kinds on transformed values plus a numeric constant, on L2's model;
    three walkers start outside the uniform prior (log-probability -inf), so proposals are refused
    by the prior: prior_forbidden_proposals > 0 and the same in every mode.  The log-probability of
    EVERY stored position is compared with the same priors in NumPy: -inf where they say -inf,
    and through check_oracle on the sampled pairs elsewhere"""
    from oracle import naima_np as O
    q = lambda p: dict(A=10 ** p[0], a1=p[1], ec=10 ** p[2], B=10 ** p[3])
    p0 = np.array([33.0, 2.4, 1.5, 1.0])
    model, omodel = build(na, "ECPL", True, q)

    def prior(pars):
        from naima_amd import log_uniform_prior, normal_prior, uniform_prior
        return (uniform_prior(10 ** pars[2], 20.0, 45.0) + normal_prior(np.log10(pars[1]), 0.38, 0.05)
                + log_uniform_prior(pars[3] ** 2, 0.5, 2.0) + uniform_prior(pars[0], 20, 45) + 0.125)

    def oprior(p):
        with np.errstate(all="ignore"):
            return float(O.uniform_prior(10 ** p[2], 20.0, 45.0)
                         + O.normal_prior(np.log10(p[1]), 0.38, 0.05)
                         + O.log_uniform_prior(p[3] ** 2, 0.5, 2.0)
                         + O.uniform_prior(p[0], 20, 45) + 0.125)

    E, raw = data_for(omodel, p0, True, 9)
    nw = 16
    pos = _spread(p0, nw, np.random.default_rng(12), [0.5, 0.03, 0.08, 0.05])
    pos[[2, 7, 13], 2] = [1.75, 1.2, 1.7]  # (e_cutoff = 56, 16, 50 TeV: outside [20, 45])
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    assert_loops(runs, True)
    same_chains(runs)
    forb = {m: r["forbidden"] for m, r in runs.items()}
    assert forb["resident"] > 0 and len(set(forb.values())) == 1, forb
    r = runs["resident"]
    inside = np.array([[np.isfinite(oprior(p)) for p in step] for step in r["chain"]])
    assert (~inside).sum() >= 3 and inside.sum() >= 10 * (~inside).sum() or inside.sum() > 50
    for m, rr in runs.items():
        assert np.array_equal(np.isneginf(rr["lp"]), ~inside), m
    nsteps = r["chain"].shape[0]
    pairs = [(s, w) for s in (0, nsteps - 1) for w in range(nw) if inside[s, w]]
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=pairs, tag="X priors")


def test_negative_amplitude(na, monkeypatch):
    """[negative-amplitude]: amplitude -(10 ** pars[0]) on synchrotron + IC -- the log-domain items
    carry ln |A| and the sign separately.  The data are the negated table; the oracle decides
    what the spectrum is"""
    q = lambda p: dict(A=-(10 ** p[0]), a1=p[1], ec=10 ** p[2], B=10 ** p[3])
    p0 = np.array([33.0, 2.4, 1.5, 1.0])
    model, omodel = build(na, "ECPL", True, q)
    prior, oprior = uniform([(20, 45), (1, 4), (-1, 3), (-1, 4)])
    E, raw = data_for(omodel, p0, True, 11, negate=True)
    assert np.all(raw["flux"] < 0)
    pos = _spread(p0, 16, np.random.default_rng(12), [0.3, 0.03, 0.05, 0.02])
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m) for m in MODES}
    assert_loops(runs, True)
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="X negative-amplitude")
    same_chains(runs)
    assert np.all(runs["resident"]["blobs"][0] <= 0) and np.any(runs["resident"]["blobs"][0] < 0)


# ------------------------------------------------------------------- non-positive energies
# (id, kind, syn, q, the coordinate that is an energy, p0, spread of the others)
NP_CASES = [
    ("ecut-beta1", "ECPL", False, lambda p: dict(A=10 ** p[0], a1=p[1], ec=p[2]), 2,
     [33.0, 2.4, 0.0], [0.3, 0.04, 0.0]),
    ("ecut-beta1.5", "ECPL", True,
     lambda p: dict(A=10 ** p[0], a1=p[1], ec=p[2], beta=1.5, B=10 ** p[3]), 2,
     [33.0, 2.4, 0.0, 1.0], [0.3, 0.03, 0.0, 0.02]),
    ("e0", "ECPL", False, lambda p: dict(A=10 ** p[0], a1=p[1], ec=10 ** p[2], e0=p[3]), 3,
     [33.0, 2.4, 1.3, 0.0], [0.3, 0.04, 0.05, 0.0]),
    ("ebreak", "BPL", True,
     lambda p: dict(A=10 ** p[0], a1=p[1], a2=p[1] + 1.0, eb=p[2], B=10 ** p[3]), 2,
     [33.0, 2.0, 0.0, 1.0], [0.3, 0.03, 0.0, 0.02]),
]
NP_SEED, NP_STEPS, NP_NW = 5, (3, 4), 16


def np_problem(case):
    """(q, p0 with the energy at 10 TeV, start positions: the energy coordinate spread over
    0.5 .. 30 TeV, wide uniform bounds that leave negative energies allowed)"""
    cid, kind, syn, q, ke, p0, widths = case
    p0 = np.array(p0)
    p0[ke] = 10.0
    rng = np.random.default_rng(31)
    pos = _spread(p0, NP_NW, rng, widths)
    pos[:, ke] = np.geomspace(0.5, 30.0, NP_NW)[rng.permutation(NP_NW)]
    bounds = [(-1000.0, 1000.0)] * len(p0)
    return q, p0, pos, bounds


def np_replay(case, omodel, E, raw, oprior, pos, nsteps):
    """the run's seeded move stream through oracle.stretch_move_reference with the oracle's lnprob,
    a proposal whose energy coordinate is not positive counted and treated as NaN:
    (chain, log-probability after the last step, proposals, non-positive ones, what the oracle
    itself gives for those)"""
    from naima_amd._lib import Moves
    from oracle import naima_np as O
    from oracle import workloads_np as WN
    ke = case[4]
    seen = dict(n=0, bad=0, oracle=[])

    def lnp(x, count=True):
        out = []
        for p in np.atleast_2d(x):
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (a negative number under a real power)
                lp = O.lnprobmodel(WN.to_data_repr(omodel(p, E)[0], raw), raw) + oprior(p)
            if count:
                seen["n"] += 1
            if not p[ke] > 0.0:
                if count:
                    seen["bad"] += 1
                    seen["oracle"].append(float(lp))
                lp = np.nan
            out.append(lp)
        return np.array(out)

    m = Moves(NP_SEED, NP_NW, 2.0, ksteps=32, depth=4)
    S, P, Z, L = [], [], [], []
    for n in nsteps:  # (the sampler takes the moves of each run_mcmc call on their own)
        addr, got = m.take(n)
        assert got == n
        for o, v in zip((S, P, Z, L), m.view(addr, got)):
            o.append(np.array(v))
    m.close()
    S, P, Z, L = [np.concatenate(o) for o in (S, P, Z, L)]
    c, l = pos.copy(), lnp(pos, count=False)
    assert np.all(np.isfinite(l))
    chain = []
    for k in range(sum(nsteps)):
        c, l, _ = O.stretch_move_reference(c, l, lnp, S[k], P[k], Z[k], L[k])
        chain.append(c.copy())
    return np.array(chain), l, seen


@pytest.mark.parametrize("case", NP_CASES, ids=[c[0] for c in NP_CASES])
def test_nonpositive_energy(na, monkeypatch, case):
    """[nonpositive-energy] (module docstring): e_cutoff (beta = 1 and 1.5), e_0 and e_break as
    the plain coordinate, started between 0.5 and 30 TeV without a prior against negative values.
    Asserted on the replayed stream: at least five proposals with a non-positive energy, fewer
    than half of all.  nan_policy="reject": the loop counts exactly those as NaN, in every mode,
    and its chain is the oracle-driven sampler's; "raise": emcee's ValueError in every mode.  The
    host-driven loop never gets that far: the distribution's constructor refuses a negative
    energy on the host (validator.py, as the reference's), where the device path cannot look."""
    from naima_amd.datatable import make_data
    from naima_amd.sampler import EnsembleSampler
    cid, kind, syn = case[:3]
    q, p0, pos, bounds = np_problem(case)
    model, omodel = build(na, kind, syn, q)
    prior, oprior = uniform(bounds)
    E, raw = data_for(omodel, p0, syn, 13, uls=False)
    chain, l, seen = np_replay(case, omodel, E, raw, oprior, pos, NP_STEPS)
    print("\n%s: %d of %d proposals have a non-positive energy; the oracle gives %s for them"
          % (cid, seen["bad"], seen["n"], np.array(seen["oracle"])))
    assert seen["n"] == sum(NP_STEPS) * NP_NW
    assert 5 <= seen["bad"] < seen["n"] / 2, seen
    runs = {m: run_loop(na, monkeypatch, model, prior, raw, pos, m, steps=NP_STEPS, seed=NP_SEED,
                        nan_policy="reject") for m in MODES}
    assert_loops(runs, syn)
    for m, r in runs.items():
        assert r["nan"] == seen["bad"], (m, r["nan"], seen["bad"])
        assert np.all(np.isfinite(r["lp"])), m
        assert np.all(r["chain"][:, :, case[4]] > 0), m  # (no walker ever holds such an energy)
        np.testing.assert_allclose(r["chain"], chain, rtol=1e-8, err_msg=m)
        np.testing.assert_allclose(r["lp"][-1], l, rtol=1e-6, err_msg=m)
    same_chains(runs)
    check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, tag="X nonpositive " + cid)
    for m in MODES:
        with pytest.raises(ValueError, match="returned NaN"):
            run_loop(na, monkeypatch, model, prior, raw, pos, m, steps=NP_STEPS, seed=NP_SEED,
                     nan_policy="raise")
    for k in ("NAIMA_AMD_RESIDENT", "NAIMA_AMD_MEGA"):
        monkeypatch.delenv(k, raising=False)
    h = EnsembleSampler(NP_NW, len(p0), na.lnprob, args=[make_data(raw), model, prior],
                        seed=NP_SEED, naima_style=True, store_blobs=True, nan_policy="reject")
    with pytest.raises(ValueError, match="should be positive"):
        h.run_mcmc(pos, sum(NP_STEPS))
