"""nh_integrate_tables against the long double reference of tests/integrate_np.py at every kernel
variant its launcher picks (tests/integrate_cases.py: each case asks the planner first and fails
when the planner disagrees with the case's label), the fused likelihood epilogue at shapes that
reach it, the entry point's refusals, and the contract the non-negative form relies on, held
against the table builders whose callers promise it.

The bound: |out - ref| <= 5e-13 * S per element, S = scale * sum |term| of the element's plane,
and exactly 0 where S = 0.  Derived, not tuned: nh_common.h documents 2e-13 per segment at the
series threshold (the cancellation in u2 - u1) + 3e-14 for nh_rcp1f, and the worst case of a
sequential sum of 3072 terms adds 3072 * 2^-53 = 3.4e-13."""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

import integrate_cases as IC
import integrate_np as INP

pytestmark = pytest.mark.gpu

BOUND = 5e-13
SENTINEL = -7.25e77  # what `out` holds before a launch; the padding columns keep it


@pytest.fixture(scope="module")
def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def _launch(ctx, dev, N, nG, nK, scale, nonneg, nsplit):
    ldo = nK + 3
    out = ctx.array(np.full((nsplit, N, ldo), SENTINEL))
    ctx.call("nh_integrate_tables", dev["w"], dev["dlw"], N, nG, dev["lx"], dev["Kt"], dev["dlnKt"],
             nK, None if scale is None else ctx.array(scale), out, ldo, nonneg, nsplit)
    return out.get()


def _hold(got, planes, S, nK, rows_kernel, what):
    """the bound on every element of every plane; returns the largest |out - ref| / S"""
    assert np.all(got[:, :, nK:] == SENTINEL), what
    g = got[:, :, :nK]
    if rows_kernel and len(g) > 1:  # everything is in plane 0, the others are zeroed
        assert np.all(g[1:] == 0.0), what
        g, planes, S = g[:1], planes.sum(axis=0)[None], S.sum(axis=0)[None]
    nan = np.isnan(planes)
    assert np.array_equal(np.isnan(g), nan), what
    err = np.abs(g.astype(INP.LD) - planes)
    dead = ~nan & (S == 0)
    assert np.all(g[dead] == 0.0), what
    live = ~nan & (S > 0)
    frac = err[live] / S[live]
    worst = float(frac.max()) if frac.size else 0.0
    print("%-44s max |out - ref| / S = %.3g" % (what, worst))
    bad = np.argwhere(live & (err > BOUND * S))
    assert bad.size == 0, (what, worst, bad[:8].tolist())
    return worst


@pytest.mark.parametrize("nonneg", [1, 0], ids=["nonneg", "signed"])
@pytest.mark.parametrize("case", IC.CASES, ids=IC.CASE_IDS)
def test_integrate_tables_variant(ctx, case, nonneg):
    """one shape of the table, scale given and NULL, ldo = nK + 3, against the reference.
    nonneg: zero table entries marked dlnKt = 1e300 (isolated, a run, a whole column, a whole
    tile) and planted |dl| on both sides of the series threshold; signed: the same + sign
    changes, an all-negative walker, unmarked zeros and -0.0 in w and Kt, NaN dl, and one walker
    with a NaN weight, whose row is NaN while its neighbours hold the bound"""
    cid, N, nG, nK, nsplit, label = case
    rc, p = IC.plan(N, nG, nK, nsplit, 0)
    assert rc == 0 and p[:4] == label, "the planner picks %r for %s" % (p, cid)
    d = IC.make_case(N, nG, nK, signed=not nonneg)
    dev = {k: ctx.array(d[k]) for k in ("w", "dlw", "lx", "Kt", "dlnKt")}
    r = d["nan_row"]
    for scale in (d["scale"], None):
        planes, S = IC.reference(d, N, nsplit, scale)
        got = _launch(ctx, dev, N, nG, nK, scale, nonneg, nsplit)
        what = "%s/%s/%s" % (cid, "nonneg" if nonneg else "signed",
                             "scale" if scale is not None else "null")
        _hold(got, planes, S, nK, label[0], what)
        if r is not None:  # (the reference's NaNs are the NaN walker's, and it has some)
            nan = np.isnan(planes)
            assert nan[:, r].any() and not np.delete(nan, r, axis=1).any()
    if not nonneg:
        return
    # exact zeros: column 1 of every plane, the second tile where there is one, empty planes
    g = got[:, :, :nK]
    if nK > 1:
        assert np.all(g[:, :, 1] == 0.0)
    if nK >= 128:
        assert np.all(g[:, :, 64:128] == 0.0)
    hper = -(-(nG - 1) // nsplit)
    for h in range(nsplit):
        if h * hper >= nG - 1 and not label[0]:
            assert np.all(g[h] == 0.0), h


def _weights(ctx, N, nG, rng):
    from naima_amd.constants import MEC2_EV
    gam = np.logspace(3, 8.5, nG)
    rows = np.zeros((N, 8))
    rows[:, 0] = 10 ** rng.normal(33, 0.1, N)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = 1e13, rng.uniform(2, 3, N), 5e13, 1.0
    gd, ed, rd = ctx.array(gam), ctx.array(gam * MEC2_EV), ctx.array(rows)
    w, dlw, lx = ctx.empty((N, nG)), ctx.empty((N, nG)), ctx.empty((nG - 1,))
    ctx.call("nh_particle_weights", 1, rd, N, ed, gd, nG, MEC2_EV, w, dlw, None)
    ctx.call("nh_grid_logratio", gd, nG, lx)
    return w, dlw, lx


@pytest.mark.parametrize("nonneg", [1, 0], ids=["nonneg", "signed"])
@pytest.mark.parametrize("shape", IC.FUSED, ids=["w1-c16", "w1-c8", "w2-c16", "w2-c8-odd"])
def test_fused_epilogue_is_reached(ctx, shape, nonneg):
    """nh_integrate_tables_lnprob where the launch DOES carry the likelihood (the planner says
    fused = 1; tests/test_gpu_parity.py::test_abi_last_producer_epilogues covers the fallback):
    the spectra equal nh_integrate_tables' to the bit, the likelihood and the accept state equal
    nh_integrate_tables + nh_lnprob_accept at that test's tolerances"""
    from naima_amd.darray import nh_accept, nh_comp
    N, nG, nE, cw = shape
    assert IC.plan(N, nG, nE, 1, 1) == (0, (0,) + cw + (1, 1))
    rng = np.random.default_rng(8 + N + nG)
    ndim, ns = 3, N
    w, dlw, lx = _weights(ctx, N, nG, rng)
    other = ctx.array(rng.random((N, nE)) * 1e20)
    conv = ctx.array(np.ones(nE))
    flux, err = ctx.array(rng.random(nE) * 1e21), ctx.array(np.full(nE, 3e20))
    ulh = np.zeros(nE, dtype=np.int32)
    ulh[-2:] = 1
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

    K = rng.random((nG, nE)) + 0.1
    dK = np.zeros_like(K)
    dK[:-1] = np.log(K[1:] / K[:-1])
    Kt, dKt, sc = ctx.array(K), ctx.array(dK), ctx.array(rng.random(nE) + 0.5)
    o1, o2, t1, t2 = ctx.empty((N, nE)), ctx.empty((N, nE)), ctx.empty((N,)), ctx.empty((N,))
    s1, s2 = state(), state()
    m1, m2 = mv_of(s1), mv_of(s2)
    ia = (w, dlw, N, nG, lx, Kt, dKt, nE, sc)
    ctx.call("nh_integrate_tables", *ia, o1, nE, nonneg, 1)
    ctx.call("nh_lnprob_accept", comps_of(o1, 2.0), 2, N, nE, conv, flux, err, err, ul, cl, None,
             None, 0, None, t1, C.addressof(m1))
    ctx.call("nh_integrate_tables_lnprob", *ia, o2, nE, nonneg, comps_of(o2, 2.0), 2, 1, conv, flux,
             err, err, ul, cl, None, None, 0, t2, C.addressof(m2))
    a, b = o1.get(), o2.get()
    assert np.isfinite(a).all() and (a > 0).all()
    assert np.array_equal(a, b)
    assert_allclose(t2.get(), t1.get(), rtol=1e-12)
    for x, y in zip(s1, s2):
        assert_allclose(x.get(), y.get(), rtol=1e-13)
    assert 0 < s1[2].get().sum() <= ns


def test_unfused_shapes_say_so():
    for N, nG, nK in IC.NOT_FUSED:
        assert IC.plan(N, nG, nK, 1, 1)[1][4] == 0


def test_integrate_tables_refusals(ctx):
    """return codes, nothing launches: nsplit 0 and 9, ldo < nK, nG = 1, NULL pointers; N = 0 is
    fine and leaves `out` as it was"""
    from naima_amd import _lib
    lib = _lib.load()
    N, nG, nK = 16, 20, 64
    d = IC.make_case(N, nG, nK, signed=0)
    dev = {k: ctx.array(d[k]) for k in ("w", "dlw", "lx", "Kt", "dlnKt")}
    out = ctx.array(np.full((N, nK), SENTINEL))

    def rc(N=N, nG=nG, nK=nK, ldo=nK, nsplit=1, **ptr):
        a = dict(w=dev["w"].ptr, dlw=dev["dlw"].ptr, lx=dev["lx"].ptr, Kt=dev["Kt"].ptr,
                 dlnKt=dev["dlnKt"].ptr, out=out.ptr, h=ctx.h)
        a.update(ptr)
        return lib.nh_integrate_tables(a["h"], a["w"], a["dlw"], N, nG, a["lx"], a["Kt"], a["dlnKt"],
                                       nK, None, a["out"], ldo, 1, nsplit)

    assert rc(nsplit=0) != 0 and rc(nsplit=9) != 0
    assert rc(ldo=nK - 1) != 0
    assert rc(nG=1) != 0
    assert rc(nK=0) != 0 and rc(N=-1) != 0
    for name in ("h", "w", "dlw", "lx", "Kt", "dlnKt", "out"):
        assert rc(**{name: None}) != 0, name
        assert b"NULL" in lib.nh_last_error()
    assert rc(N=0) == 0
    ctx.sync()
    assert np.all(out.get() == SENTINEL)
    assert rc() == 0  # (and the same call with everything in place launches)
    assert np.all(out.get() != SENTINEL)


def _ulp_diff(a, ref):
    """|a - ref| in units of the spacing of float64 at ref (ref in long double)"""
    return np.abs(a.astype(INP.LD) - ref) / np.spacing(np.abs(ref.astype(np.float64)))


def _builders(ctx, gd, nG, Ed, nE):
    se7 = np.geomspace(0.05, 20.0, 7)
    sd7 = np.random.default_rng(4).uniform(0.1, 2.0, 7)
    return [
        ("planck-iso", lambda K, D, ld: ctx.call("nh_table_ic_planck", gd, nG, Ed, nE, 2.72, 0.0, 1,
                                                 K, D, ld)),
        ("planck-ani", lambda K, D, ld: ctx.call("nh_table_ic_planck", gd, nG, Ed, nE, 30.0, 2.0, 0,
                                                 K, D, ld)),
        ("seed-1", lambda K, D, ld: ctx.call("nh_table_ic_seed", gd, nG, Ed, nE,
                                             ctx.array(np.array([1.5])), ctx.array(np.array([0.26])),
                                             1, K, D, ld)),
        ("seed-7", lambda K, D, ld: ctx.call("nh_table_ic_seed", gd, nG, Ed, nE, ctx.array(se7),
                                             ctx.array(sd7), 7, K, D, ld)),
    ]


@pytest.mark.parametrize("which", ["planck-iso", "planck-ani", "seed-1", "seed-7", "pion"])
def test_builders_keep_the_nonnegative_contract(ctx, which):
    """what nonnegative = 1 relies on, from the builders whose callers pass it: on a 40-node grid
    with kinematically forbidden corners (nE = 65, ld = 70) Kt is finite and >= 0, dlnKt is finite,
    >= 1e300 exactly where Kt[i] or Kt[i+1] is zero, elsewhere within 4 ulp of
    ln(Kt[i+1]/Kt[i]) taken in long double from the device's own Kt, 0 in the last row; the
    padding columns are untouched"""
    from naima_amd.constants import MEC2_EV
    nG, nE, ld = 40, 65, 70
    if which == "pion":
        x = np.geomspace(1.2181, 1e7, nG)        # proton energies, GeV, from the threshold up
        E = np.geomspace(1e7, 1e16, nE)          # photons up to a GeV above the last proton
        gd, Ed = ctx.array(x), ctx.array(E)
        build = lambda K, D, ld: ctx.call("nh_table_pion_analytic", gd, nG, Ed, nE, 1, 1, K, D, ld)
    else:
        x = np.geomspace(3.0, 1e7, nG)           # Lorentz factors
        E = np.geomspace(1e3, 2e13, nE)          # photons beyond gamma m c^2 of most nodes
        assert (E[-1] > x * MEC2_EV).sum() > nG // 2
        gd, Ed = ctx.array(x), ctx.array(E)
        build = dict(_builders(ctx, gd, nG, Ed, nE))[which]
    Kt, dK = ctx.array(np.full((nG, ld), SENTINEL)), ctx.array(np.full((nG, ld), SENTINEL))
    build(Kt, dK, ld)
    K, D = Kt.get(), dK.get()
    assert np.all(K[:, nE:] == SENTINEL) and np.all(D[:, nE:] == SENTINEL)
    K, D = K[:, :nE], D[:, :nE]
    assert np.isfinite(K).all() and (K >= 0).all() and np.isfinite(D).all()
    z = K == 0
    assert 0 < z.sum() < z.size
    assert z[:, -1].any() and (~z).sum() > nG * nE // 4, "the grids miss the forbidden corner"
    ends = z[:-1] | z[1:]
    assert np.array_equal(D[:-1] >= 1e300, ends)
    assert np.all(D[-1] == 0.0)
    KL = K.astype(INP.LD)
    with np.errstate(all="ignore"):
        ref = np.log(KL[1:] / KL[:-1])
    live = ~ends
    ulps = _ulp_diff(D[:-1][live], ref[live])
    print("%-12s max |dlnKt - ln(K2/K1)| = %.3g ulp over %d segments" % (which, ulps.max(),
                                                                          live.sum()))
    assert ulps.max() <= 4
