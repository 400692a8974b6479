"""nh_synchrotron against the long double reference of tests/synchrotron_np.py at every launch
shape its launcher picks (tests/synchrotron_cases.py: each case asks the planner first and fails
when the planner disagrees with the case's label), on grids that take each form of syn_dlnP1,
with dead energies, dead tiles, bad fields and a NaN weight; a workload-shaped case whose weights
come from nh_particle_weights; the likelihood epilogue at every instance that carries it; and the
entry points' refusals.

The bound: |out - ref| <= C0 S + C1 SX per element, S = CS1 sum |term|, SX = CS1 sum |term| x
(x the larger of the segment's two E/Ec).  Derived from the documented errors of the pieces
(nh_syn.h, nh_common.h) and the roundings of the kernel's expressions, eps = 2^-53; not tuned.

A segment's term is (u2 - u1) lx / dl.  Errors that the nodes and dl SHARE cost their own size:
the term is a mean of u1 and u2 (u1 lx expm1(dl)/dl with dl = ln(u2/u1)).  Errors in which dl and
ln(u2/u1) of the computed nodes DISAGREE are divided by |dl| in u2 - u1, |dl| >= 2^-10 (below it
the series takes over, which has no cancellation): a factor A = 1 + 2^10.
  shared, per node   syn_P1: 2e-14 (one Newton step) + 14 eps (its own arithmetic, cb = cbq ig23
                     with two cube roots); exp: 4 eps; w (P ev): 2 eps              -> 2.3e-14
                     x = q ig2: 10 eps (seven roundings in q = E qfac, three in ig2 and the
                     product), which exp(-x) multiplies by x                        -> 10 eps x
  disagreeing        dlw against the rounded weights: 2 eps; the two exponentials: 8 eps; the
                     four products of the two nodes: 4 eps; the sum dlw + dlnP - q dig2: eps
                                                                                      -> A 15 eps
                     syn_dlnP1 against ln(P2/P1) of the computed P, D(grid): the truncation
                     2 s^7/7 of the three-term form (5 terms: 2 s^11/11) + 3e-14 (nh_rcp1f) and
                     three roundings of 2 s; log(P2/P1): 2 eps + eps of its value.  Taken at the
                     largest s^2 the reference finds among the grid's live segments in each
                     form's range (a ballot may give a lane a more accurate form than its own
                     s^2 asks for, never a less accurate one): 9.3e-16 at 100 nodes per decade
                     (s^2 <= 5.9e-5).  On the coarser grids P flattens down the exponential and
                     s^2 passes through every value below the grid's largest, so a wave there may
                     take three terms right at their limit s^2 = 1e-4: 3.5e-15        -> A D
                     x2 - x1 of the rounded x against q dig2: the two x: 2 eps x, ig2: 4 eps x,
                     dig2 = v (r r - 1): 3 eps x, q dig2: eps x                       -> A 10 eps x
  the term           nh_rcp1f: 3e-14; the subtraction and two products: 3 eps
  the sums           a chunk is at most ceil(5033 / 16) = 315 segments + 64 partials (the cases'
                     longest: nG = 5034, C = 16, nA = 40 gives 201 + 25): 400 eps
  CS1 erg/eV         ten roundings: 10 eps
C0 = 2.3e-14 + 3e-14 + 413 eps + A (15 eps + D) = 2.7e-12 at 100 per decade, else 5.4e-12,
C1 = 10 eps + A 10 eps = 1.1e-12.
Nearly all of either is the one worst case |dl| = 2^-10, which the planted segments hit; a
segment away from the peak of its integrand (|dl| ~ lx) is good to 1e-13.

Underflow elements -- S before CS1 below 2^-960, where the nodes that make the sum are denormal
numbers or nearly -- are held only to 0 <= out <= 2 ref + 2^-1000 CS1
(test_synchrotron_host.py: at most 5 % of any case's live elements)."""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

import synchrotron_cases as SC
import synchrotron_np as SNP

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
AMP = 1 + 2.0 ** 10
C1 = 10 * EPS + AMP * 10 * EPS


def c0_of(s2):
    """C0 for a grid whose largest s^2 in the three ranges of syn_dlnP1's forms are s2 [3]"""
    s3, s5, sl = np.sqrt(s2)
    rcp = 3e-14 + 3 * EPS
    D = max(2 * s3 ** 7 / 7 + rcp * 2 * s3, 2 * s5 ** 11 / 11 + rcp * 2 * s5,
            (2 * EPS + EPS * np.log((1 + sl) / (1 - sl))) if sl > 0 else 0.0)
    return 2.3e-14 + 3e-14 + 413 * EPS + AMP * (15 * EPS + D)


UNDER = 2.0 ** -960
SENTINEL = -7.25e77  # what `out` holds before a launch; the padding columns keep it


@pytest.fixture(scope="module")
def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def _launch(ctx, d, N, nG, nE):
    ldo = nE + 3
    out = ctx.array(np.full((N, ldo), SENTINEL))
    ctx.call("nh_synchrotron", ctx.array(d["w"]), ctx.array(d["dlw"]), ctx.array(d["B"]), 3, N,
             ctx.array(d["gam"]), ctx.array(d["lx"]), nG, ctx.array(d["E"]), nE, out, ldo)
    return out.get()


def _hold(got, ref, nE, what):
    """the padding, the NaN pattern, the exact zeros, the underflow cap and the bound; returns
    (the largest |out - ref| / (C0 S + C1 SX), its (walker, energy))"""
    assert np.all(got[:, nE:] == SENTINEL), what
    g = got[:, :nE]
    C0 = c0_of(ref["s2"])
    spec, S, SX = ref["spec"], ref["S"], ref["SX"]
    nan = np.isnan(spec)
    assert np.array_equal(np.isnan(g), nan), (what, np.argwhere(np.isnan(g) != nan)[:8].tolist())
    dead = ~nan & (S == 0)
    assert np.all(g[dead] == 0.0), what
    live = ~nan & (S > 0)
    under = live & (ref["S_raw"] < UNDER)
    gl = g.astype(SNP.LD)
    cap = 2 * spec + SNP.LD(2) ** -1000 * ref["cs1"]
    assert np.all((gl[under] >= 0) & (gl[under] <= cap[under])), what
    held = live & ~under
    with np.errstate(all="ignore"):
        frac = np.where(held, np.abs(gl - spec) / (C0 * S + C1 * SX), 0)
    at = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[at])
    of_s = float(np.abs(gl[at] - spec[at]) / S[at]) if held[at] else 0.0
    print("%-28s C0 = %.3g: max |out - ref| / (C0 S + C1 SX) = %.3g at walker %d, energy %d: "
          "%.3g of S, SX/S = %.3g (%d held, %d under the cap, %d dead, %d NaN)"
          % (what, C0, worst, at[0], at[1], of_s, float(SX[at] / S[at]) if held[at] else 0.0,
             held.sum(), under.sum(), dead.sum(), nan.sum()))
    assert worst <= 1.0, (what, worst, np.argwhere(frac > 1)[:8].tolist())
    return worst, at


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_synchrotron_variant(ctx, case):
    """one shape, on every grid of synchrotron_cases.grids_of: B read with ldB = 3, ldo = nE + 3,
    against the reference.  Walkers 3..6 of a case with N >= 8 have B = 0, < 0, NaN, +inf (NaN
    rows); walker 7 has a NaN weight at an interior node m: NaN exactly where i0 <= m"""
    cid, N, nG, nE, label, _ = case
    rc, p = SC.plan(N, nG, nE, 0)
    assert rc == 0 and p[:3] == label, "the planner picks %r for %s" % (p, cid)
    for gname in SC.grids_of(nG):
        d = SC.make_case(cid, gname)
        ref = SC.case_reference(cid, gname)
        got = _launch(ctx, d, N, nG, nE)
        _hold(got, ref, nE, "%s/%s" % (cid, gname))
        if N >= 8:
            nan = np.isnan(ref["spec"])
            for r, b in SC.BAD_B.items():
                assert nan[r].all()
            m = d["nan_node"]
            assert np.array_equal(nan[SC.NAN_ROW], ref["i0"][SC.NAN_ROW] <= m)
            assert not nan[[0, 1, 2, 8]].any()  # (every such case has nine walkers or more)


def test_synchrotron_on_the_workload_weights(ctx):
    """w, dlw and lx as the workloads make them -- nh_particle_weights (an exponential cutoff
    power law) and nh_grid_logratio on naima's default electron grid, 1 GeV .. 510 TeV at 100 per
    decade -- downloaded and fed to the reference: the analytic dlw together with the kernel.  The
    energies keep x <= 60 at the last node, so that no element hangs on denormal exponentials
    (these weights are 1e50, not 1: S says nothing about underflow here)"""
    from naima_amd.constants import MEC2_EV
    from oracle import naima_np as O
    rng = np.random.default_rng(21)
    N, nE = 12, 64
    gam = O.electron_grid(1e9, 510e12, 100)
    nG = gam.size
    rows = np.zeros((N, 8))
    rows[:, 0] = 10 ** rng.normal(33, 0.1, N)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = 1e13, rng.uniform(2, 3, N), 5e13, 1.0
    B = 10 ** rng.uniform(-5.3, -4.3, N)
    gd, ed, rd = ctx.array(gam), ctx.array(gam * MEC2_EV), ctx.array(rows)
    w, dlw, lx = ctx.empty((N, nG)), ctx.empty((N, nG)), ctx.empty((nG - 1,))
    ctx.call("nh_particle_weights", 1, rd, N, ed, gd, nG, MEC2_EV, w, dlw, None)
    ctx.call("nh_grid_logratio", gd, nG, lx)
    E = np.geomspace(1e-7, 60 * SC.ec_ev(B.min(), gam[-1]), nE)
    rc, p = SC.plan(N, nG, nE, 0)
    assert rc == 0 and p[:3] == (16, 64, 1)
    ldo = nE + 3
    out = ctx.array(np.full((N, ldo), SENTINEL))
    ctx.call("nh_synchrotron", w, dlw, ctx.array(B), 1, N, gd, lx, nG, ctx.array(E), nE, out, ldo)
    ref = SNP.spectrum(w.get(), dlw.get(), B, gam, lx.get(), E)
    ref["S_raw"] = np.ones_like(ref["S"])  # (no underflow elements: every energy is held)
    assert (ref["S"] > 0).all() and (ref["i0"] > 0).any() and (ref["i0"] == 0).any()
    _hold(out.get(), ref, nE, "workload weights")


@pytest.mark.parametrize("table", ["live", "dead"])
@pytest.mark.parametrize("shape", SC.EPILOGUE, ids=SC.EPILOGUE_IDS)
def test_synchrotron_epilogue(ctx, shape, table):
    """nh_synchrotron_lnprob against nh_synchrotron + nh_lnprob_accept at every instance with the
    epilogue: the spectra equal to the bit, the totals at rtol 1e-12, the accept state at 1e-13.
    Walkers 3..6 of every 16 have a bad field: their totals are NaN and nh_nan_count counts
    them.  table = dead: every energy above every walker's live range (nA = 0 in every
    workgroup), all spectra zero"""
    from naima_amd import _lib
    from naima_amd.darray import nh_accept, nh_comp
    N, nG, nE, Cw = shape
    assert SC.plan(N, nG, nE, 1)[1][:3] == (Cw, 64, 1)
    lib = _lib.load()
    rng = np.random.default_rng(8 + N + nG + nE)
    d = SC.make_inputs(N, nG, nE, "low", SC.grids_of(nG)[0])
    E = d["E"] if table == "live" else np.geomspace(1e7, 1e9, nE) * SC.ec_ev(SC.B_MID, d["gam"][-1])
    ndim, ns = 3, N
    w, dlw, Bd = ctx.array(d["w"]), ctx.array(d["dlw"]), ctx.array(d["B"])
    gd, lx, Ed = ctx.array(d["gam"]), ctx.array(d["lx"]), ctx.array(E)
    other = ctx.array(rng.random((N, nE)) * 1e-8)
    conv = ctx.array(np.ones(nE))
    flux, err = ctx.array(rng.random(nE) * 1e-7), ctx.array(np.full(nE, 3e-8))
    ulh = np.zeros(nE, dtype=np.int32)
    ulh[-2:] = 1 if nE > 2 else 0
    ul, cl = ctx.array(ulh, dtype=np.int32), ctx.array(np.full(nE + 1, 0.9))
    coords, logp = rng.normal(size=(2 * ns, ndim)), rng.normal(-50, 5, 2 * ns)
    blk_h = np.zeros((1, 3 * ns))
    perm = rng.permutation(2 * ns)
    blk_h[0, :ns], blk_h[0, ns:2 * ns] = (rng.random(ns) + 1) ** 2 / 2, np.log(rng.random(ns))
    iv = blk_h[:, 2 * ns:].view(np.int32)
    iv[0, :ns], iv[0, ns:] = perm[:ns], perm[ns:][rng.integers(ns, size=ns)]
    logp[perm[:ns:2]] = -1e300  # every other active walker accepts whatever comes
    blk = ctx.array(blk_h)
    cursor = ctx.array(np.zeros(1, dtype=np.int32), dtype=np.int32)

    def state():
        return (ctx.array(coords.ravel()), ctx.array(logp), ctx.empty((ns,), dtype=np.int32),
                ctx.array(np.zeros(2 * ns, dtype=np.int32), dtype=np.int32),
                ctx.empty((ns,), dtype=np.int32))

    def mv_of(st):
        return nh_accept(st[0].ptr, st[1].ptr, blk.ptr, cursor.ptr, ns, ndim, 0, 0, st[2].ptr,
                         st[3].ptr, st[4].ptr)

    def comps_of(out, scale):
        c = (nh_comp * 2)()
        c[0], c[1] = nh_comp(other.ptr, nE, 1.0), nh_comp(out.ptr, nE, scale)
        return c

    def nans():
        ctx.sync()
        n = C.c_int(-1)
        assert lib.nh_nan_count(ctx.h, 1, C.byref(n)) == 0
        return n.value

    o1, o2, t1, t2 = ctx.empty((N, nE)), ctx.empty((N, nE)), ctx.empty((N,)), ctx.empty((N,))
    s1, s2 = state(), state()
    m1, m2 = mv_of(s1), mv_of(s2)
    sa = (w, dlw, Bd, 3, N, gd, lx, nG, Ed, nE)
    nans()
    ctx.call("nh_synchrotron", *sa, o1, nE)
    ctx.call("nh_lnprob_accept", comps_of(o1, 0.5), 2, N, nE, conv, flux, err, err, ul, cl, None,
             None, 0, None, t1, C.addressof(m1))
    n1 = nans()
    ctx.call("nh_synchrotron_lnprob", *sa, o2, nE, comps_of(o2, 0.5), 2, 1, conv, flux, err, err,
             ul, cl, None, None, 0, t2, C.addressof(m2))
    n2 = nans()
    a, b = o1.get(), o2.get()
    assert np.array_equal(a, b, equal_nan=True)
    bad = ~(d["B"][:, 0] > 0) | ~np.isfinite(d["B"][:, 0])
    assert bad.sum() == 4 * (N // 16) + (4 if N % 16 >= 8 else 0)
    good = a[~bad & (np.arange(N) % 16 != SC.NAN_ROW)]
    assert np.isnan(a[bad]).all() and not np.isnan(good).any()
    if table == "dead":
        assert np.all(a[~bad] == 0.0)
    else:
        assert (good >= 0).all() and (good > 0).mean() > 0.5  # (some underflow to 0)
    ta, tb = t1.get(), t2.get()
    assert np.isnan(ta[bad]).all() and np.isfinite(ta[~np.isnan(a).any(axis=1)]).all()
    assert_allclose(tb, ta, rtol=1e-12)
    for x, y in zip(s1, s2):
        assert_allclose(x.get(), y.get(), rtol=1e-13)
    assert n1 == n2 == np.isnan(ta).sum() >= bad.sum()
    assert 0 < s1[2].get().sum() <= ns


def test_synchrotron_refusals(ctx):
    """return codes, nothing launches: NULL pointers, nG = 1, nE = 0, ldo < nE, ldB = 0, N < 0,
    nG = 5035 (150 KB of LDS), nE = 65 with the epilogue; N = 0 is fine and leaves `out` as it
    was"""
    from naima_amd import _lib
    from naima_amd.darray import nh_comp
    lib = _lib.load()
    N, nG, nE = 8, 40, 12
    d = SC.make_inputs(N, nG, nE, "low", "d40")
    dev = {k: ctx.array(d[k]) for k in ("w", "dlw", "B", "gam", "lx", "E")}
    out = ctx.array(np.full((N, nE), SENTINEL))
    big = ctx.array(np.zeros(65))

    def rc(N=N, nG=nG, nE=nE, ldo=nE, ldB=3, **ptr):
        a = {k: v.ptr for k, v in dev.items()}
        a.update(out=out.ptr, h=ctx.h)
        a.update(ptr)
        return lib.nh_synchrotron(a["h"], a["w"], a["dlw"], a["B"], ldB, N, a["gam"], a["lx"], nG,
                                  a["E"], nE, a["out"], ldo)

    assert rc(nG=1) != 0 and rc(nE=0) != 0 and rc(ldo=nE - 1) != 0 and rc(ldB=0) != 0
    assert rc(N=-1) != 0
    assert rc(nG=5035) != 0 and b"LDS" in lib.nh_last_error()
    for name in ("h", "w", "dlw", "B", "gam", "lx", "E", "out"):
        assert rc(**{name: None}) != 0, name
        assert b"NULL" in lib.nh_last_error()
    # the epilogue needs one tile: nE = 65 is refused before anything is read
    comps = (nh_comp * 1)()
    comps[0] = nh_comp(out.ptr, 65, 1.0)
    tot = ctx.array(np.full(N, SENTINEL))
    r = lib.nh_synchrotron_lnprob(ctx.h, dev["w"].ptr, dev["dlw"].ptr, dev["B"].ptr, 3, N,
                                  dev["gam"].ptr, dev["lx"].ptr, nG, big.ptr, 65, out.ptr, 65,
                                  comps, 1, 0, big.ptr, big.ptr, big.ptr, big.ptr, big.ptr, big.ptr,
                                  None, None, 0, tot.ptr, None)
    assert r != 0 and b"nE <= 64" in lib.nh_last_error()
    assert rc(N=0) == 0
    ctx.sync()
    assert np.all(out.get() == SENTINEL) and np.all(tot.get() == SENTINEL)
    assert rc() == 0  # (and the same call with everything in place launches)
    assert np.all(out.get() != SENTINEL)
