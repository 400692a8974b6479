"""The resident loop's synchrotron items start a live range at x <= 128 where the distribution's
form allows it (nh_syn2.h: hs_s2_cut_ok; the rule itself: test_syn_dead_prefix_host.py) -- here the
kernel that takes the decision, against the oracle and against the per-launch kernel, which keeps
the whole range from x <= 746 on.

Synchrotron + IC on the CMB with We as a blob (cfg3's shape), 16 walkers, three steps across a
run_mcmc boundary, at most eight photon energies.  Every case: the resident loop's model spectra,
We and log-probability against the NumPy oracle at test_gpu_shapes.py's tolerances (1e-9 on the
flux), and against one launch per half-step at 1e-10.  Under NH_HS_DEBUG the kernel counts the
live ranges that start at x <= 128 and those that keep their head; the cases assert the path they
were written for through those two counters:

  * every kind of distribution, the walkers' fields spread from 1e-3 to 1e4 uG and energies from
    1 eV to 100 keV: along one row the first live node runs from node 0 to past the grid's end;
  * an energy set for which every node is live (nothing to leave out) and one with no live node;
  * a grid shared between the synchrotron and the IC table;
  * a power law of index 40 and a log-parabola of strongly negative curvature, whose ln w rises
    steeply toward low gamma: the guard fails and the whole range is walked (asserted);
  * degenerate walkers among normal ones -- a NaN amplitude and an index the prior forbids as
    starting positions, negative fields as proposals (a NaN log-probability is an error for a
    starting position): the same NaN / -inf pattern as the per-launch loop.
"""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

import test_gpu_shapes as TS

pytestmark = pytest.mark.gpu

KPC = TS.KPC
SGRID = (1e9, 510998.9499961643e9, 100)   # naima's default electron grid of Synchrotron
IGRID = (1e11, 1e15, 40)
KINDS = ["PowerLaw", "ExponentialCutoffPowerLaw", "BrokenPowerLaw", "ExponentialCutoffBrokenPowerLaw",
         "LogParabola"]


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def syn_ic(na, kind, sgrid=SGRID, igrid=IGRID, linear_B=False):
    """pars: log10 amplitude, index, log10(e_cutoff or e_break / TeV), log10(B / uG) (B / uG itself
    with linear_B), the second shape parameter (beta, alpha_2, or the log-parabola's curvature)"""
    from oracle import naima_np as O
    u = na.u

    def pdist(pars):
        amp, e0, e1 = 10 ** pars[0] / u.eV, 10.0 * u.TeV, 10 ** pars[2] * u.TeV
        if kind == "PowerLaw":
            return na.PowerLaw(amp, e0, pars[1])
        if kind == "ExponentialCutoffPowerLaw":
            return na.ExponentialCutoffPowerLaw(amp, e0, pars[1], e1, pars[4])
        if kind == "BrokenPowerLaw":
            return na.BrokenPowerLaw(amp, e0, e1, pars[1], pars[4])
        if kind == "ExponentialCutoffBrokenPowerLaw":
            return na.ExponentialCutoffBrokenPowerLaw(amp, e0, e1, pars[1], pars[4], 30.0 * e1)
        return na.LogParabola(amp, e0, pars[1], pars[4])

    def opdist(p):
        amp, e1 = 10 ** p[0], 10 ** p[2] * 1e12
        kw = {"PowerLaw": dict(alpha=p[1]),
              "ExponentialCutoffPowerLaw": dict(alpha=p[1], e_cutoff=e1, beta=p[4]),
              "BrokenPowerLaw": dict(e_break=e1, alpha_1=p[1], alpha_2=p[4]),
              "ExponentialCutoffBrokenPowerLaw": dict(e_break=e1, alpha_1=p[1], alpha_2=p[4],
                                                      e_cutoff=30.0 * e1, beta=1.0),
              "LogParabola": dict(alpha=p[1], beta=p[4])}[kind]
        return O.ParticleDist(kind, amplitude=amp, e_0=10e12, **kw)

    def model(pars, data):
        pd = pdist(pars)
        B = (pars[3] if linear_B else 10 ** pars[3]) * u.uG
        SYN = na.Synchrotron(pd, B=B, Eemin=sgrid[0] * u.eV, Eemax=sgrid[1] * u.eV, nEed=sgrid[2])
        IC = na.InverseCompton(pd, seed_photon_fields=["CMB"], Eemin=igrid[0] * u.eV,
                               Eemax=igrid[1] * u.eV, nEed=igrid[2])
        return (SYN.flux(data, distance=1 * u.kpc) + IC.flux(data, distance=1 * u.kpc),
                IC.compute_We(Eemin=1 * u.TeV))

    def omodel(p, E):
        pd = opdist(p)
        gs, gi = O.electron_grid(*sgrid), O.electron_grid(*igrid)
        B = (p[3] if linear_B else 10 ** p[3]) * 1e-6
        with np.errstate(all="ignore"):
            sy = O.synchrotron_spectrum(E, gs, O.nelec_on(pd, gs), B)
            ic, _ = O.ic_spectrum(E, gi, O.nelec_on(pd, gi), [O.thermal_seed("CMB")])
            We = O.electron_energy_content(pd, O.electron_grid(1e12, igrid[1], igrid[2]))
        return O.to_flux(sy + ic, KPC), We

    return model, omodel


def run_modes(na, monkeypatch, model, prior, raw, pos, nan_policy="raise"):
    """two steps, then one, of the resident loop (with its debug counters) and of the per-launch
    loop -> (runs as test_gpu_shapes.run_loop returns them, ranges cut, ranges kept)"""
    from naima_amd import _lib
    from naima_amd.datatable import make_data
    from naima_amd.sampler import EnsembleSampler
    runs, counts = {}, None
    nw, nd = pos.shape
    for mode in ("resident", "per-launch"):
        for k in ("NAIMA_AMD_RESIDENT", "NAIMA_AMD_MEGA", "NH_RUN_RT", "NH_HS_DEBUG"):
            monkeypatch.delenv(k, raising=False)
        for k, v in TS.MODES[mode].items():
            monkeypatch.setenv(k, v)
        if mode == "resident":
            monkeypatch.setenv("NH_HS_DEBUG", "1")
        s = EnsembleSampler(nw, nd, na.lnprob, args=[make_data(raw), model, prior], seed=5,
                            naima_style=True, store_blobs=True, device=True, nan_policy=nan_policy)
        with np.errstate(all="ignore"):
            st = s.run_mcmc(pos, 2)  # (the first call's half-steps settle and record the plan)
            s.run_mcmc(st, 1)
        dev = s._dev
        assert dev is not None and dev.mega
        runs[mode] = dict(chain=s.get_chain(), lp=s.get_log_prob(),
                          blobs=[np.asarray(b, dtype=float) for b in s.get_blobs()],
                          units=list(s.blob_units or []), info=getattr(dev, "resident_info", None),
                          launches=dev.resident_launches, reason=getattr(dev, "resident_reason", None),
                          nan=s.nan_proposals)
        if mode == "resident":
            assert dev.resident_launches > 0, getattr(dev, "resident_reason", "")
            assert dev.resident_info["syn_log_domain"], dev.resident_info
            buf = np.zeros((256 * 64 * 8 + 64 * 4 * 16,), dtype=np.int64)
            _lib._chk(_lib._lib.nh_half_step_run_stamps(_lib.get_context().h, dev._run,
                                                        buf.ctypes.data_as(C.c_void_p)))
            counts = (int(buf[256 * 64 * 8 + 11 * 16]), int(buf[256 * 64 * 8 + 11 * 16 + 1]))
        else:
            assert dev.resident_launches == 0
    return runs, counts[0], counts[1]


def same_as_per_launch(runs):
    a, b = runs["per-launch"], runs["resident"]
    assert_allclose(b["chain"], a["chain"], rtol=1e-10)
    assert np.array_equal(np.isnan(b["lp"]), np.isnan(a["lp"]))
    assert np.array_equal(np.isinf(b["lp"]), np.isinf(a["lp"]))
    fin = np.isfinite(a["lp"])
    assert_allclose(b["lp"][fin], a["lp"][fin], rtol=1e-10)
    for x, y in zip(b["blobs"], a["blobs"]):
        assert_allclose(x, y, rtol=1e-10, atol=1e-300, equal_nan=True)


def data_around(omodel, p0, E, seed):
    true = TS._repr(omodel(p0, E)[0], E, "erg/(cm2 s)")
    return TS.make_raw(E, true, "erg/(cm2 s)", np.random.default_rng(seed), rel=(0.05, 0.05),
                       scatter=0.05, cl0=0.9, dcl=0.0)


P0 = {"PowerLaw": [33.0, 2.6, 0.0, 1.0, 0.0],
      "ExponentialCutoffPowerLaw": [33.0, 2.3, 1.6, 1.0, 1.0],
      "BrokenPowerLaw": [33.0, 2.0, 0.5, 1.0, 3.0],
      "ExponentialCutoffBrokenPowerLaw": [33.0, 2.0, 0.5, 1.0, 3.0],
      "LogParabola": [33.0, 2.3, 0.0, 1.0, 0.15]}
BOUNDS = [(20, 45), (-1, 45), (-3, 5), (-4, 5), (-5, 5)]
E_WIDE = np.geomspace(1.0, 1e5, 8)  # eV


def spread_fields(p0, nw, seed):
    """walkers around p0 whose fields run from 1e-3 to 1e4 uG"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(p0) + np.array([0.1, 0.05, 0.1, 0.0, 0.05]) * rng.uniform(-1, 1, (nw, 5))
    pos[:, 3] = np.linspace(-3.0, 4.0, nw)
    return pos


@pytest.mark.parametrize("kind", KINDS)
def test_every_first_live_node_every_kind(na, monkeypatch, kind):
    """fields from 1e-3 to 1e4 uG against energies from 1 eV to 100 keV: x at the grid's first node
    runs from 5e-3 to 3e11 and at its last one from 2e-14 to 1e3, so ranges begin at node 0, inside
    every unit of 64 nodes, and nowhere; where one begins inside the grid with room for the guard's
    two kept nodes it starts at x <= 128 (these distributions pass the guard: counted)"""
    model, omodel = syn_ic(na, kind)
    prior, oprior = TS.uniform(BOUNDS)
    nw = 16
    pos = spread_fields(P0[kind], nw, 3)
    raw = data_around(omodel, np.asarray(P0[kind]), E_WIDE, 4)
    runs, ncut, nkept = run_modes(na, monkeypatch, model, prior, raw, pos)
    print("\n%s: live ranges that start at x <= 128: %d, that keep their head: %d" % (kind, ncut, nkept))
    assert ncut > 0
    pairs = [(s, w) for s in (0, 2) for w in range(nw)]
    TS.check_oracle(na, runs, raw, lambda p: omodel(p, E_WIDE), oprior, pairs=pairs, tag=kind)
    same_as_per_launch(runs)


@pytest.mark.parametrize("which", ["every-node-live", "no-node-live"])
def test_energy_sets_with_nothing_to_leave_out(na, monkeypatch, which):
    """every-node-live: 1e-6 .. 1e-5 eV at 5 .. 50 uG, x <= 30 at the grid's first node; no-node-live:
    20 .. 100 keV at 1e-3 uG, x > 746 at its last one.  No range has a head: both counters stay 0."""
    kind = "ExponentialCutoffPowerLaw"
    model, omodel = syn_ic(na, kind)
    prior, oprior = TS.uniform(BOUNDS)
    nw = 16
    pos = spread_fields(P0[kind], nw, 5)
    if which == "every-node-live":
        E = np.geomspace(1e-6, 1e-5, 4)
        pos[:, 3] = np.linspace(0.7, 1.7, nw)
    else:
        E = np.geomspace(2e4, 1e5, 4)
        pos[:, 3] = np.linspace(-3.05, -2.95, nw)
    p0 = np.asarray(P0[kind], dtype=float)
    p0[3] = pos[nw // 2, 3]
    raw = data_around(omodel, p0, E, 6)
    runs, ncut, nkept = run_modes(na, monkeypatch, model, prior, raw, pos)
    assert (ncut, nkept) == (0, 0)
    pairs = [(s, w) for s in (0, 2) for w in range(nw)]
    TS.check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=pairs, tag=which)
    same_as_per_launch(runs)


def test_grid_shared_with_a_table(na, monkeypatch):
    """the synchrotron and the IC table on one grid (equal Eemin / Eemax / nEed): the table reads
    every weight of it; the synchrotron ranges still start at x <= 128"""
    kind = "ExponentialCutoffPowerLaw"
    grid = (1e11, 1e14, 100)
    model, omodel = syn_ic(na, kind, sgrid=grid, igrid=grid)
    prior, oprior = TS.uniform(BOUNDS)
    nw = 16
    pos = spread_fields(P0[kind], nw, 7)
    raw = data_around(omodel, np.asarray(P0[kind]), E_WIDE, 8)
    runs, ncut, nkept = run_modes(na, monkeypatch, model, prior, raw, pos)
    assert ncut > 0
    pairs = [(s, w) for s in (0, 2) for w in range(nw)]
    TS.check_oracle(na, runs, raw, lambda p: omodel(p, E_WIDE), oprior, pairs=pairs, tag="shared grid")
    same_as_per_launch(runs)


@pytest.mark.parametrize("kind,p0", [("PowerLaw", [33.0, 40.0, 0.0, 1.0, 0.0]),
                                     ("LogParabola", [33.0, 2.0, 0.0, 1.0, -3.0])],
                         ids=["power-law-index-40", "log-parabola-curvature-minus-3"])
def test_guard_fails_and_the_whole_range_is_walked(na, monkeypatch, kind, p0):
    """ln w rises steeply toward low gamma: by 39 per e-fold for the power law -- e^-x loses to it
    from x = 746 down, the head of the range IS the integral -- and by 1 + 6 ln(10 TeV / E) for the
    log-parabola, whose ranges below ~90 GeV keep their head while those above lose it.  The
    spectra are the oracle's; the counter of ranges that kept their head shows the fallback ran
    (for the power law: for every range)."""
    model, omodel = syn_ic(na, kind)
    prior, oprior = TS.uniform(BOUNDS)
    nw = 16
    pos = spread_fields(p0, nw, 9)
    pos[:, 3] = np.linspace(-1.0, 3.0, nw)
    raw = data_around(omodel, np.asarray(p0), E_WIDE, 10)
    runs, ncut, nkept = run_modes(na, monkeypatch, model, prior, raw, pos)
    print("\n%s: live ranges that start at x <= 128: %d, that keep their head: %d" % (kind, ncut, nkept))
    assert nkept > 0
    if kind == "PowerLaw":
        assert ncut == 0
    pairs = [(s, w) for s in (0, 2) for w in range(nw)]
    TS.check_oracle(na, runs, raw, lambda p: omodel(p, E_WIDE), oprior, pairs=pairs, tag="guard " + kind)
    same_as_per_launch(runs)


def test_degenerate_walkers_among_normal_ones(na, monkeypatch):
    """Walkers of cfg3's kind around cfg3's p0 at three of its X-ray energies and three TeV ones,
    the field itself a parameter and its prior open below zero.  A NaN log-probability is emcee's
    error for a STARTING position (here as there), so the degenerate walkers that sit in the
    ensemble are ones the prior forbids -- a NaN amplitude, an index of 5.5: whoever takes them as
    a partner proposes NaN or forbidden parameters -- and the negative fields come as proposals:
    three walkers start at 0.02 .. 0.1 uG, from where a stretch of z > 1 lands below zero; the
    reference's spectrum is NaN there, the proposal is evaluated, rejected and counted (asserted).
    Chain, log-probability and blobs carry the same NaN / -inf pattern as the per-launch loop's,
    and the normal walkers' spectra are the oracle's."""
    kind = "ExponentialCutoffPowerLaw"
    model, omodel = syn_ic(na, kind, igrid=(1e11, 510998.9499961643e9, 100), linear_B=True)
    bounds = [(0, 100), (-1, 5), (-3, 5), (-1e3, 1e6), (0.1, 5)]  # (cfg3's, but for the field's sign)
    prior, oprior = TS.uniform(bounds)
    p0 = np.array([33.0, 2.5, np.log10(48.0), 12.0, 1.0])
    E = np.concatenate([np.geomspace(550.0, 11200.0, 3), np.geomspace(0.33e12, 170e12, 3)])
    nw = 16
    pos = p0 * (1 + 0.03 * np.random.default_rng(11).standard_normal((nw, 5)))
    pos[[3, 4, 10], 3] = [0.05, 0.1, 0.02]
    pos[7, 0] = np.nan
    pos[12, 1] = 5.5
    raw = data_around(omodel, p0, E, 12)
    runs, ncut, nkept = run_modes(na, monkeypatch, model, prior, raw, pos, nan_policy="reject")
    assert ncut > 0
    same_as_per_launch(runs)
    assert runs["resident"]["nan"] > 0 and runs["resident"]["nan"] == runs["per-launch"]["nan"]
    lp = runs["resident"]["lp"]
    print("\ndegenerate: log-probability of the two forbidden walkers", lp[:, [7, 12]].tolist(),
          "NaN proposals rejected", runs["resident"]["nan"])
    normal = [w for w in range(nw) if w not in (7, 12)]
    assert np.isfinite(lp[:, normal]).all() and not np.isfinite(lp[:, 7]).any() and np.isneginf(lp[0, 12])
    chain = runs["resident"]["chain"]
    assert np.all(chain[:, normal, 3] > 0) and np.isnan(chain[:, 7, 0]).all()
    pairs = [(s, w) for s in (0, 2) for w in normal]
    TS.check_oracle(na, runs, raw, lambda p: omodel(p, E), oprior, pairs=pairs, tag="degenerate")
