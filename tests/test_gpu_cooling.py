"""Cooled electron populations on the GPU (nh_cooled_electrons / nh_cooled_weights,
CooledElectrons): the kernel against the NumPy restatement at every shape its code treats
differently and against the closed form, bit identity between calls, between host batches and
device parameters and between a batch and its walkers, the resampling kernel, the domain, the
radiative classes on a cooled population, secondaries, a fit on the device loop, the examples."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cooling_cases as CC
import cooling_np as CN

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# nh_cooled_electrons against the restatement: the two differ in libm and in the order of the
# scans' sums.  4 x the largest relative difference measured on an MI355X over every case below
# (profiles/NOTES_cooling.md): 7.9e-13, at 2048 nodes and three fields; 3e-14 up to 257 nodes.
RTOL_KERNEL = 4 * 7.9e-13
# against the closed form: 4 x the measured 8.3e-14 | 8.3e-14 | 6.7e-16 (ages of CC.CF_AGES), and
# 4 x the measured 4.4e-16 for n / (Q age) - 1 at the tiny age
RTOL_CLOSED = (4 * 8.3e-14, 4 * 8.3e-14, 4 * 6.7e-16)
RTOL_LIMIT = 4 * 4.5e-16


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def _lazy(ctx, v, keep):
    from naima_amd.darray import DVec, lazy_const, nh_lazy
    if isinstance(v, DVec):
        keep.append(v)
        return v.lazy()
    if np.ndim(v) == 0:
        return lazy_const(float(v))
    d = ctx.array(np.asarray(v, dtype=float))
    keep.append(d)
    return nh_lazy(d.ptr, 1, 1.0, 1.0, 0.0, 0, 0)


def solve_gpu(e, Q, N, B, age, loss=None, u=(), shared_row=False, want_status=False):
    """n[N][nC] of one nh_cooled_electrons launch; B, age, u[f]: floats, host vectors or DVecs"""
    from naima_amd import _lib
    from naima_amd.darray import nh_lazy
    from naima_amd.models import cool_status
    ctx = _lib.get_context()
    keep = []
    e = np.asarray(e, dtype=float)
    nC = e.size
    ed, Qd = ctx.array(e), ctx.array(np.ascontiguousarray(Q, dtype=float))
    Bl, al = _lazy(ctx, B, keep), _lazy(ctx, age, keep)
    nf = len(u)
    ul = (nh_lazy * max(nf, 1))()
    for f in range(nf):
        ul[f] = _lazy(ctx, u[f], keep)
    ld = ctx.array(np.ascontiguousarray(loss, dtype=float)) if nf else None
    out = ctx.empty((N, nC))
    st = cool_status(ctx)
    st.set(np.zeros(1, dtype=np.int32))
    ctx.call("nh_cooled_electrons", Qd, 0 if shared_row else nC, N, ed, nC, C.addressof(Bl),
             ld.ptr if ld is not None else None, nf, ul, C.addressof(al), out, st)
    got = out.get()
    return (got, int(st.get()[0])) if want_status else got


def injection_gpu(kind, rows, e):
    """Q[N][nC] of nh_particle_weights (n_out) for parameter rows [N][8]"""
    from naima_amd import _lib
    ctx = _lib.get_context()
    rows = np.atleast_2d(np.asarray(rows, dtype=float))
    N, nC = rows.shape[0], e.size
    if nC < 2:
        raise ValueError
    ed, rd = ctx.array(e), ctx.array(rows)
    w, lw, n = ctx.empty((N, nC)), ctx.empty((N, nC)), ctx.empty((N, nC))
    ctx.call("nh_particle_weights", kind, rd, N, ed, ed, nC, 1.0, w, lw, n)
    return n.get()


def rel_diff(got, ref):
    """largest relative difference; zeros and NaNs have to sit in the same places"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert_array_equal(np.isnan(got), np.isnan(ref))
    assert_array_equal(got == 0.0, ref == 0.0)
    m = np.isfinite(ref) & (ref != 0.0)
    return float(np.abs(got[m] / ref[m] - 1.0).max()) if m.any() else 0.0


# --------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("nf", CC.KERNEL_NF)
@pytest.mark.parametrize("nC", CC.KERNEL_NC)
def test_kernel_against_restatement_shapes(na, nC, nf):
    """below a wave, across the wave boundary, across the 256-thread stride, the cap; 0, 1, 3
    fields; 1, 3 and 65 walkers with ages from far below to far above the cooling times"""
    e = CC.kernel_grid(nC)
    loss = CC.synthetic_loss(nf, e)
    kind, p = CC.INJECTIONS["ECPL"]
    worst = 0.0
    for N in CC.KERNEL_N:
        B, age, u = CC.walker_values(N, nf)
        rows = np.tile(np.asarray(p, dtype=float), (N, 1))
        rows[:, 2] += 0.05 * np.arange(N)
        Q = injection_gpu(kind, rows, e)
        got = solve_gpu(e, Q, N, B, age, loss, list(u))
        ref = CN.solve_batch(e, Q, B, age, loss, u)
        worst = max(worst, rel_diff(got, ref))
    print("nC %d nf %d: max relative difference %.3g" % (nC, nf, worst))
    assert worst < RTOL_KERNEL


@pytest.mark.parametrize("name", list(CC.INJECTIONS) + ["BPL_break_on_node"])
def test_kernel_against_restatement_injections(na, name):
    """all five kinds; a break on a node and between nodes; a cut-off below the grid, whose zero
    nodes must come out as exact zeros"""
    e = CC.kernel_grid(257)
    kind, p = CC.INJECTIONS["BPL" if name == "BPL_break_on_node" else name]
    p = list(p)
    if name == "BPL_break_on_node":
        p[5] = e[100]
    else:
        assert not np.any(e == p[5])
    N, nf = 3, 2
    B, age, u = CC.walker_values(N, nf, seed=3)
    loss = CC.synthetic_loss(nf, e)
    Q = injection_gpu(kind, np.tile(p, (N, 1)), e)
    # (the helper's kind and row layout; subnormal values carry fewer bits: compared above 1e-280)
    Qn = CC.injection_np(kind, p, e)
    assert_allclose(Q[0][Qn > 1e-280], Qn[Qn > 1e-280], rtol=1e-12, atol=0)
    got = solve_gpu(e, Q, N, B, age, loss, list(u))
    ref = CN.solve_batch(e, Q, B, age, loss, u)
    d = rel_diff(got, ref)
    print("%s: max relative difference %.3g, %d zero nodes" % (name, d, (Q[0] == 0).sum()))
    assert d < RTOL_KERNEL
    if name == "ECPL_cut_below_grid":
        assert np.all(Q == 0.0) and np.all(got == 0.0)
    if name == "ECPL_zeros_on_top":
        z = Q[0] == 0.0
        assert 0 < z.sum() < e.size and np.all(got[:, z] == 0.0) and np.all(got[:, :20] > 0.0)


def test_more_than_2048_nodes_are_refused(na):
    from naima_amd._lib import NaimaHipError
    e = CC.kernel_grid(2049)
    with pytest.raises(NaimaHipError, match="2048"):
        solve_gpu(e, np.ones((1, 2049)), 1, 1e-5, 1e10)


# ----------------------------------------------------------------------- 2. the closed form
@pytest.mark.parametrize("k", range(3))
def test_kernel_against_closed_form(na, k):
    c, age = CC.CF, CC.CF_AGES[k]
    e = CN._log_grid(c["Emin"], c["Emax"], c["npd"])
    a = CN.syn_coefficient(c["B_G"])
    Q = c["Q0"] * (e / c["e0"]) ** -c["alpha"]
    n = solve_gpu(e, Q[None, :], 1, c["B_G"], age)[0]
    exact = CN.closed_form_powerlaw(e, c["Q0"], c["e0"], c["alpha"], a, age, e[-1])
    rel = np.abs(n[:-1] / exact[:-1] - 1.0)
    print("closed form, age %g s: max rel %.3g at node %d" % (age, rel.max(), rel.argmax()))
    assert n[-1] == 0.0 and rel.max() < RTOL_CLOSED[k]
    if k == 2:
        lim = np.abs(n[:-1] / (Q[:-1] * age) - 1.0).max()
        print("n / (Q age) - 1: %.3g" % lim)
        assert lim < RTOL_LIMIT


# ----------------------------------------------------------------------------- 3. bit identity
def test_bit_identity(na):
    from naima_amd import _lib
    from naima_amd.darray import DVec
    ctx = _lib.get_context()
    nC, N, nf = 570, 7, 2
    e = CC.kernel_grid(nC)
    loss = CC.synthetic_loss(nf, e)
    B, age, u = CC.walker_values(N, nf, seed=5)
    kind, p = CC.INJECTIONS["ECBPL"]
    rows = np.tile(np.asarray(p, dtype=float), (N, 1))
    rows[:, 2] += 0.03 * np.arange(N)
    Q = injection_gpu(kind, rows, e)
    a = solve_gpu(e, Q, N, B, age, loss, list(u))
    assert_array_equal(a, solve_gpu(e, Q, N, B, age, loss, list(u)))  # two calls
    keep = [ctx.array(v) for v in (B, age, u[0], u[1])]
    dv = [DVec(ctx, d, d.ptr, N) for d in keep]
    assert_array_equal(a, solve_gpu(e, Q, N, dv[0], dv[1], loss, dv[2:]))  # device parameters
    for k in range(N):  # a batch's row is the scalar call of that walker
        one = solve_gpu(e, Q[k:k + 1], 1, float(B[k]), float(age[k]), loss,
                        [float(u[0][k]), float(u[1][k])])
        assert_array_equal(a[k], one[0])
    shared = solve_gpu(e, Q[:1], N, B, age, loss, list(u), shared_row=True)  # ldq = 0
    assert_array_equal(shared, solve_gpu(e, np.repeat(Q[:1], N, axis=0), N, B, age, loss, list(u)))


def test_model_host_batch_device_parameters_and_walkers_agree_bitwise(na):
    """the same through CooledElectrons: a host-vector batch, the same values as device
    parameters, and the scalar model of every walker"""
    from naima_amd import _lib
    from naima_amd.darray import DVec
    u_ = na.u
    ctx = _lib.get_context()
    N = 5
    B = np.linspace(5.0, 60.0, N)
    lage = np.linspace(2.0, 5.5, N)
    ufir = np.linspace(0.2, 0.9, N)
    inj = na.ExponentialCutoffPowerLaw(1e36 / u_.eV / u_.s, 1 * u_.TeV, 2.1, 80 * u_.TeV)
    E = np.geomspace(2e9, 4e14, 40) * u_.eV

    def model(B, age, uf):
        return na.CooledElectrons(inj, B * u_.uG, age * u_.yr,
                                  ["CMB", ["FIR", 30 * u_.K, uf * u_.eV / u_.cm ** 3]])

    host = model(B, 10 ** lage, ufir)
    h = host(E).value
    assert h.shape == (N, 40) and np.all(h > 0) and host.batch_size == N and not host.on_device
    d = [ctx.array(v) for v in (B, 10 ** lage, ufir)]
    dev = model(*[DVec(ctx, x, x.ptr, N) for x in d])
    assert dev.on_device and dev.batch_size == N
    assert_array_equal(np.asarray(dev(E).value), h)
    for k in range(N):
        assert_array_equal(model(B[k], 10 ** lage[k], ufir[k])(E).value, h[k])
    # against the restatement on the model's grid and loss table
    e = host.energies.value
    loss = np.stack([CN.loss_table(T, e) for T in (2.72548, 30.0)])
    uu = np.stack([np.full(N, CN.AR_CGS * 2.72548 ** 4), ufir * 1.602176634e-12])
    Qn = CC.injection_np(1, [1e36, 1e12, 2.1, 80e12, 1.0, 0, 0], e)
    ref = CN.solve_batch(e, Qn, B * 1e-6, 10 ** lage * CC.YR, loss, uu)
    got = host(host.energies).value
    # (the loss table: the GPU's IC kernel against the oracle's, 1e-9 as in tests/test_gpu_*.py)
    assert_allclose(got[:, :-1], ref[:, :-1], rtol=1e-8)
    tb = host.break_energy().to("eV").value
    tc = host.cooling_time(tb[2] * u_.eV).to("yr").value
    assert_allclose(tc[2], 10 ** lage[2], rtol=1e-10)
    # walker 0 (100 yr in 5 uG) has not cooled anywhere on the grid: no break; then older
    # walkers in stronger fields break lower
    assert np.isnan(tb[0]) and np.all(np.diff(tb[1:]) < 0)


# ----------------------------------------------------------------------- 4. nh_cooled_weights
def weights_gpu(n, ec, e, xg, scale):
    from naima_amd import _lib
    ctx = _lib.get_context()
    n = np.atleast_2d(np.asarray(n, dtype=float))
    N, nG = n.shape[0], e.size
    w, lw = ctx.empty((N, nG)), ctx.empty((N, nG))
    ctx.call("nh_cooled_weights", ctx.array(n), ctx.array(ec), ec.size, N, ctx.array(e),
             ctx.array(xg), nG, float(scale), w, lw)
    return w.get(), lw.get()


def test_weights_same_grid_overhang_and_power_law(na):
    ec = CC.kernel_grid(300)
    rng = np.random.default_rng(2)
    n = np.stack([1e40 * (ec / 1e12) ** -2.2, 1e38 * (ec / 1e12) ** -1.0 * rng.uniform(0.5, 2, 300),
                  1e40 * (ec / 1e12) ** -2.2])
    n[2, 100:110] = 0.0
    xg = ec / 510998.9499961643
    w, lw = weights_gpu(n, ec, ec, xg, 510998.9499961643)
    assert_array_equal(w, xg * 510998.9499961643 * n)  # the solve grid itself: bit for bit
    for k in range(3):
        rw, rl = CN.resample(n[k], ec, ec, xg, 510998.9499961643)
        assert_array_equal(w[k], rw)
        assert_array_equal(lw[k] == 1e300, rl == 1e300)
        assert_allclose(lw[k], rl, rtol=1e-12, atol=1e-13)
    assert np.all(lw[2, 99:110] == 1e300) and lw[2, 98] != 1e300 and np.all(lw[:, -1] == 0.0)
    # a target grid that overhangs both ends, finer than the solve grid
    e = np.geomspace(ec[0] / 30, ec[-1] * 30, 1301)
    w, lw = weights_gpu(n, ec, e, e, 1.0)
    out = (e < ec[0]) | (e > ec[-1])
    assert out.sum() > 100 and np.all(w[:, out] == 0.0) and np.all(w[:2, ~out] > 0.0)
    first, last = np.nonzero(~out)[0][[0, -1]]
    assert np.all(lw[:, first - 1] == 1e300) and np.all(lw[:, last] == 1e300)
    assert np.all(lw[:, :first - 1] == 1e300) and np.all(lw[:, last + 1:-1] == 1e300)
    # a power law is reproduced to rounding: e n = 1e40 e (e/1e12)^-2.2
    pl = 1e40 * e[~out] * (e[~out] / 1e12) ** -2.2
    d = np.abs(w[0, ~out] / pl - 1.0).max()
    print("power law on a finer grid: max rel %.3g" % d)
    assert d < 2e-13  # (|ln(n2/n1)| <= 80 x 2^-53 x the exponent's condition, as in pd_core)
    for k in range(3):
        rw, _ = CN.resample(n[k], ec, e, e, 1.0)
        assert_allclose(w[k], rw, rtol=1e-12, atol=0)
        assert_array_equal(w[k] == 0.0, rw == 0.0)


# ------------------------------------------------------------------------------- 5. the domain
DOMAIN = [("age_zero", dict(age=0.0)), ("age_negative", dict(age=-1e10)),
          ("age_nan", dict(age=np.nan)), ("B_nan", dict(B=np.nan)),
          ("B_zero_no_u", dict(B=0.0, u=0.0)), ("B_negative_no_u", dict(B=-1e-5, u=0.0)),
          ("u_negative", dict(u=-1e-13)),
          ("u_inf", dict(u=np.inf)), ("u_nan", dict(u=np.nan))]


@pytest.mark.parametrize("name,bad", DOMAIN)
def test_domain_one_bad_walker_in_a_batch(na, name, bad):
    """every NaN-row case, one walker inside a batch of good ones whose rows must not change:
    age <= 0 or NaN; B NaN; B = 0 and B < 0 with no positive u; a negative, infinite or NaN u"""
    nC, N, nf = 130, 6, 1
    e = CC.kernel_grid(nC)
    loss = CC.synthetic_loss(nf, e)
    B, age, u = CC.walker_values(N, nf, seed=11)
    Q = np.tile(1e36 * (e / 1e12) ** -2.0, (N, 1))
    good = solve_gpu(e, Q, N, B, age, loss, list(u))
    assert np.all(np.isfinite(good))
    B2, age2, u2 = B.copy(), age.copy(), u.copy()
    B2[3] = bad.get("B", B[3])
    age2[3] = bad.get("age", age[3])
    u2[0][3] = bad.get("u", u[0][3])
    got, count = solve_gpu(e, Q, N, B2, age2, loss, list(u2), want_status=True)
    assert count == 1 and np.all(np.isnan(got[3]))
    rest = np.arange(N) != 3
    assert_array_equal(got[rest], good[rest])
    assert_array_equal(np.isnan(got), np.isnan(CN.solve_batch(e, Q, B2, age2, loss, u2)))


def test_negative_field_with_photons_cools_like_its_magnitude(na):
    """B <= 0 is a domain error only with no positive u (b would not be positive).  With
    photons b > 0 everywhere and the row is finite: B enters as B^2, so B < 0 cools like |B|,
    bit for bit -- a prior on B keeps the sampler away from the mirrored mode"""
    e = CC.kernel_grid(130)
    loss = CC.synthetic_loss(1, e)
    Q = np.tile(1e36 * (e / 1e12) ** -2.0, (2, 1))
    age, uu = np.array([1e11, 1e12]), [np.array([1e-12, 3e-12])]
    neg, count = solve_gpu(e, Q, 2, np.array([-3e-5, -1e-4]), age, loss, uu, want_status=True)
    pos = solve_gpu(e, Q, 2, np.array([3e-5, 1e-4]), age, loss, uu)
    assert count == 0 and np.all(np.isfinite(neg))
    assert_array_equal(neg, pos)


def test_domain_zero_injection_and_zero_field_with_photons(na):
    e = CC.kernel_grid(130)
    loss = CC.synthetic_loss(1, e)
    got, count = solve_gpu(e, np.zeros((2, 130)), 2, np.array([1e-5, 0.0]), np.array([1e11, np.inf]),
                           loss, [np.array([1e-12, 1e-12])], want_status=True)
    assert count == 0 and np.all(got == 0.0)  # Q == 0: exact zeros; B = 0 with photons is fine


def test_model_refusals(na):
    u_ = na.u
    inj = na.PowerLaw(1e36 / u_.eV / u_.s, 1 * u_.TeV, 2.2)
    with pytest.raises(NotImplementedError, match="must be the same for every walker"):
        na.CooledElectrons(inj, 10 * u_.uG, 1e3 * u_.yr,
                           [["dust", np.array([20.0, 30.0]) * u_.K, 0.5 * u_.eV / u_.cm ** 3]])
    with pytest.raises(NotImplementedError, match="monochromatic or tabulated"):
        na.CooledElectrons(inj, 10 * u_.uG, 1e3 * u_.yr,
                           [["star", 1.0 * u_.eV, 1.0 * u_.eV / u_.cm ** 3]])
    with pytest.raises(TypeError):
        na.CooledElectrons(na.PowerLaw(1e36 / u_.eV, 1 * u_.TeV, 2.2), 10 * u_.uG, 1e3 * u_.yr)
    with pytest.raises(ValueError, match="nodes"):
        na.CooledElectrons(inj, 10 * u_.uG, 1e3 * u_.yr, n_per_decade=400)


# ------------------------------------------------------------ 6. through the radiative classes
def test_radiative_classes_on_a_steady_state_power_law(na):
    """age = inf and synchrotron cooling alone: n = Q0 e0^a E^-(a+1) [1 - (E/Emax)^(a-1)] /
    (a_syn (a - 1)), a power law of index a + 1 up to the bracket.  Both sides use Eemax = 10 TeV
    on a population that extends to Emax = 510.998 TeV with a = 2.3: the bracket departs from 1 by
    at most (10 / 511)^1.3 = 6.0e-3 at the top of the particle grid and by less below.  The emission
    is a positive integral of n, so its relative departure is bounded by that of n: the tolerance
    is that 6.0e-3, and the cooled side is never above the power law (the bracket is < 1 and the
    log-log interpolation of a concave function lies below it).  compute_We up to 1 TeV: the
    bracket is within (1 / 511)^1.3 = 3.0e-4 of 1 there."""
    u_ = na.u
    al, Bf = 2.3, 100.0
    a = CN.syn_coefficient(Bf * 1e-6)
    Q0, e0 = 1e36, 1e12
    cooled = na.CooledElectrons(na.PowerLaw(Q0 / u_.eV / u_.s, 1 * u_.TeV, al), Bf * u_.uG,
                                np.inf * u_.s, seed_photon_fields=[])
    pl = na.PowerLaw(Q0 * e0 / (a * (al - 1.0)) / e0 ** 2 / u_.eV, 1 * u_.TeV, al + 1.0)
    kw = dict(Eemax=10 * u_.TeV)
    Es = np.geomspace(1e-3, 1e4, 15) * u_.eV
    Ei = np.geomspace(1e5, 1e9, 12) * u_.eV
    s1 = na.Synchrotron(cooled, B=Bf * u_.uG, **kw).flux(Es, distance=0).value
    s0 = na.Synchrotron(pl, B=Bf * u_.uG, **kw).flux(Es, distance=0).value
    i1 = na.InverseCompton(cooled, ["CMB"], **kw).flux(Ei, distance=0).value
    i0 = na.InverseCompton(pl, ["CMB"], **kw).flux(Ei, distance=0).value
    print("synchrotron: max rel %.3g; IC: max rel %.3g" % (np.abs(s1 / s0 - 1).max(),
                                                         np.abs(i1 / i0 - 1).max()))
    assert np.all(s0 > 0) and np.all(i0 > 0)
    assert_allclose(s1, s0, rtol=6.0e-3)
    assert_allclose(i1, i0, rtol=6.0e-3)
    assert np.all(s1 <= s0 * (1 + 1e-9)) and np.all(i1 <= i0 * (1 + 1e-9))  # the bracket is < 1
    syn = na.Synchrotron(cooled, B=Bf * u_.uG, **kw)
    We1 = syn.compute_We(Eemin=1 * u_.GeV, Eemax=1 * u_.TeV).to("erg").value
    We0 = na.Synchrotron(pl, B=Bf * u_.uG).compute_We(Eemin=1 * u_.GeV,
                                                      Eemax=1 * u_.TeV).to("erg").value
    assert_allclose(We1, We0, rtol=3e-4)
    with pytest.raises(NotImplementedError, match="injection rate"):
        syn.set_We(1e48 * u_.erg)
    # (Bremsstrahlung's own Eemin is 100 MeV, below the cooled population's Emin = 1 GeV, under
    # which it is zero: both sides start at 1 GeV)
    kb = dict(n0=1 / u_.cm ** 3, Eemin=1 * u_.GeV, Eemax=10 * u_.TeV)
    b1 = na.Bremsstrahlung(cooled, **kb).flux(Ei[:-1], distance=0).value
    b0 = na.Bremsstrahlung(pl, **kb).flux(Ei[:-1], distance=0).value
    assert np.all(b0 > 0)
    assert_allclose(b1, b0, rtol=6.0e-3)


def test_walker_loop_slices_a_cooled_batch(na):
    """a structural parameter per walker (Eemax) sends the radiative class through its host
    walker loop, which has to slice B, age and u of the CooledElectrons"""
    u_ = na.u
    B = np.array([10.0, 30.0, 90.0])
    age = np.array([1e3, 1e4, np.inf])
    uf = np.array([0.3, 0.5, 0.7])
    inj = na.PowerLaw(np.array([1e36, 2e36, 3e36]) / u_.eV / u_.s, 1 * u_.TeV, 2.2)

    def cooled(k=slice(None)):
        i2 = na.PowerLaw(inj.amplitude[k], 1 * u_.TeV, 2.2)
        return na.CooledElectrons(i2, B[k] * u_.uG, age[k] * u_.yr,
                                  ["CMB", ["FIR", 30 * u_.K, uf[k] * u_.eV / u_.cm ** 3]])

    E = np.geomspace(1e-2, 1e3, 9) * u_.eV
    Emax = np.array([50.0, 100.0, 200.0]) * u_.TeV
    got = na.Synchrotron(cooled(), B=B * u_.uG, Eemax=Emax).flux(E, distance=0).value
    for k in range(3):
        one = na.Synchrotron(cooled(k), B=B[k] * u_.uG, Eemax=Emax[k]).flux(E, distance=0).value
        assert_array_equal(got[k], one)
    from naima_amd import _lib
    from naima_amd.darray import DVec
    ctx = _lib.get_context()
    d = ctx.array(Emax.to("eV").value)
    with pytest.raises(NotImplementedError, match="device-resident per-walker value"):
        na.Synchrotron(cooled(), B=B * u_.uG,
                       Eemax=DVec(ctx, d, d.ptr, 3) * u_.eV).flux(E, distance=0)


def test_walker_loop_slices_a_batched_secondary_injection(na):
    """the same with the secondary electrons of a proton batch as the injection: the walker loop
    slices nh and the protons' own parameters"""
    u_ = na.u
    amp = np.array([1e36, 2e36, 4e36])
    al = np.array([2.0, 2.2, 2.4])
    nh = np.array([1.0, 10.0, 100.0])
    B, age = np.array([5.0, 20.0, 80.0]), np.array([1e3, 1e4, 1e5])

    def cooled(k=slice(None)):
        protons = na.ExponentialCutoffPowerLaw(amp[k] / u_.eV, 10 * u_.TeV, al[k], 3 * u_.PeV)
        sec = na.SecondaryLeptonsKelner06(protons, nh=nh[k] / u_.cm ** 3, product="electron")
        return na.CooledElectrons(sec, B[k] * u_.uG, age[k] * u_.yr, Emin=10 * u_.GeV,
                                  Emax=300 * u_.TeV, n_per_decade=40)

    E = np.geomspace(1e-2, 1e3, 7) * u_.eV
    Emax = np.array([50.0, 100.0, 200.0]) * u_.TeV
    kw = dict(Eemin=10 * u_.GeV)
    got = na.Synchrotron(cooled(), B=B * u_.uG, Eemax=Emax, **kw).flux(E, distance=0).value
    assert got.shape == (3, 7) and np.all(got > 0)
    for k in range(3):
        one = na.Synchrotron(cooled(k), B=B[k] * u_.uG, Eemax=Emax[k], **kw).flux(
            E, distance=0).value
        assert_array_equal(got[k], one)


def test_rates_as_a_device_matrix(na):
    """(energies, rates) with the rates a device matrix, [N][nC] and one shared row: the bits of
    the same numbers given on the host, and a device result"""
    from naima_amd import _lib
    from naima_amd.darray import DMat
    u_ = na.u
    ctx = _lib.get_context()
    N = 4
    e = CC.kernel_grid(90)
    rates = 1e36 * (e[None, :] / 1e12) ** -np.linspace(1.8, 2.6, N)[:, None]
    B, age = np.linspace(5, 50, N) * u_.uG, np.geomspace(1e2, 1e5, N) * u_.yr
    E = np.geomspace(2e9, 4e14, 25) * u_.eV
    unit = u_.Unit("1/(eV s)")
    for r in (rates, rates[:1]):
        host = na.CooledElectrons((e * u_.eV, u_.Quantity(r if r.shape[0] > 1 else r[0], unit)),
                                  B, age, ["CMB"])
        buf = ctx.array(r)
        dev = na.CooledElectrons((e * u_.eV, u_.Quantity(DMat.from_buffer(ctx, buf, r.shape[0],
                                                                          e.size), unit)),
                                 B, age, ["CMB"])
        assert dev.on_device and not host.on_device and dev.batch_size == N
        h = host(E).value
        assert h.shape == (N, 25) and np.all(h > 0)
        assert_array_equal(np.asarray(dev(E).value), h)
    with pytest.raises(ValueError, match="inconsistent walker-batch sizes"):
        na.CooledElectrons((e * u_.eV, u_.Quantity(DMat.from_buffer(ctx, ctx.array(rates[:3]), 3,
                                                                    e.size), unit)), B, age)


# --------------------------------------------------------------------------- 7. secondaries
def test_cooled_secondaries_equal_their_rows(na):
    u_ = na.u
    N = 3
    protons = na.ExponentialCutoffPowerLaw(np.array([1e36, 2e36, 4e36]) / u_.eV, 10 * u_.TeV,
                                           np.array([2.0, 2.2, 2.4]), 3 * u_.PeV)
    sec = na.SecondaryLeptonsKelner06(protons, nh=np.array([1.0, 10.0, 100.0]) / u_.cm ** 3,
                                      product="electron")
    B, age = np.array([5.0, 20.0, 80.0]) * u_.uG, np.array([1e3, 1e4, 1e5]) * u_.yr
    a = na.CooledElectrons(sec, B, age, Emin=10 * u_.GeV, Emax=300 * u_.TeV, n_per_decade=40)
    Eg = a.energies
    rate = sec.flux(Eg, distance=0)
    assert rate.unit.physical_type != "differential energy" and rate.value.shape == (N, Eg.size)
    b = na.CooledElectrons((Eg, rate), B, age)
    E = np.geomspace(2e10, 2e14, 30) * u_.eV
    na_, nb = a(E).value, b(E).value
    assert np.all(na_ > 0) and a.batch_size == N
    assert_array_equal(na_, nb)
    s = na.Synchrotron(a, B=B).flux(np.geomspace(1e-3, 1e3, 8) * u_.eV, distance=0).value
    assert s.shape == (N, 8) and np.all(s > 0)


# ------------------------------------------------------------------------------- 8. in a fit
FIT_E = np.concatenate([np.geomspace(1e-4, 1e4, 12), np.geomspace(1e9, 3e13, 12)])
FIT_P0 = np.array([40.0, 3.5])  # B [uG], log10(age / yr)


def fit_model(na):
    u_ = na.u

    def model(pars, data):
        inj = na.PowerLaw(3e35 / u_.eV / u_.s, 1 * u_.TeV, 2.2)
        ce = na.CooledElectrons(inj, pars[0] * u_.uG, 10 ** pars[1] * u_.yr, ["CMB", "FIR"],
                                n_per_decade=40)
        syn = na.Synchrotron(ce, B=pars[0] * u_.uG, Eemax=400 * u_.TeV, nEed=40)
        ic = na.InverseCompton(ce, ["CMB", "FIR"], Eemax=400 * u_.TeV, nEed=40)
        return syn.flux(data, distance=2 * u_.kpc) + ic.flux(data, distance=2 * u_.kpc)

    return model


def fit_data(na):
    from naima_amd.datatable import make_data
    from test_gpu_shapes import make_raw
    true = fit_model(na)(np.repeat(FIT_P0[:, None], 2, axis=1), dict(energy=FIT_E * na.u.eV))
    true = true.to("1/(s cm2 eV)").value[0] * FIT_E ** 2 * 1.602176634e-12
    return make_data(make_raw(FIT_E, true, "erg/(cm2 s)", np.random.default_rng(4)))


def test_in_a_fit_on_the_device_loop(na, monkeypatch):
    from naima_amd.sampler import EnsembleSampler
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")
    model, data = fit_model(na), fit_data(na)

    def prior(pars):
        return na.uniform_prior(pars[0], 1, 500) + na.uniform_prior(pars[1], 1, 7)

    nw, steps = 32, 20
    pos = FIT_P0 + np.array([2.0, 0.05]) * np.random.default_rng(8).standard_normal((nw, 2))
    runs = []
    for _ in range(2):
        d = EnsembleSampler(nw, 2, na.lnprob, device=True, args=[data, model, prior], seed=17,
                            naima_style=True, store_blobs=False)
        d.run_mcmc(pos, steps)
        assert d.device is True and d._dev is not None
        # the piecewise device loop: the plan holds launches the one-launch kernels do not know
        assert not d._dev.mega and not d._dev.fused
        runs.append((d.get_chain(), d.get_log_prob()))
    assert_array_equal(runs[0][0], runs[1][0])
    assert_array_equal(runs[0][1], runs[1][1])
    assert len(np.unique(runs[0][0][:, :, 0])) > nw  # (moves were accepted)
    # the last ensemble's log-probabilities against a host-batch evaluation there
    last = runs[0][0][-1]
    lp = na.lnprob(last.T, data, model, prior)[0]
    # to the kernel tolerance, relative to the log-probability itself (measured: 7.5e-14
    # absolute on values of order -10 .. -100)
    diff = np.abs(runs[0][1][-1] - lp)
    print("lnprob device loop against host batch: max diff %.3g, max rel %.3g, |lnprob| >= %.3g"
          % (diff.max(), (diff / np.abs(lp)).max(), np.abs(lp).min()))
    assert np.all(np.isfinite(lp))
    assert_allclose(runs[0][1][-1], lp, rtol=RTOL_KERNEL, atol=0)


def test_negative_ages_without_a_prior_are_counted(na, monkeypatch):
    """the age is a linear parameter without a prior and the walkers start close to 0: the
    stretch move proposes negative ages, the cooling solve gives them NaN rows, and
    nan_policy="reject" counts them, on the device loop as on the host loop"""
    from naima_amd.sampler import EnsembleSampler
    u_ = na.u
    monkeypatch.setenv("NAIMA_AMD_RESIDENT", "0")

    def model(pars, data):
        inj = na.PowerLaw(3e35 / u_.eV / u_.s, 1 * u_.TeV, 2.2)
        ce = na.CooledElectrons(inj, pars[0] * u_.uG, pars[1] * u_.yr, ["CMB"], n_per_decade=20)
        return na.Synchrotron(ce, B=pars[0] * u_.uG, nEed=20).flux(data, distance=2 * u_.kpc)

    def prior(pars):
        return na.uniform_prior(pars[0], 1, 500)

    E = np.geomspace(1e-4, 1e4, 10)
    from naima_amd.datatable import make_data
    from test_gpu_shapes import make_raw
    true = model(np.array([[40.0, 40.0], [50.0, 50.0]]), dict(energy=E * u_.eV))
    true = true.to("1/(s cm2 eV)").value[0] * E ** 2 * 1.602176634e-12
    data = make_data(make_raw(E, true, "erg/(cm2 s)", np.random.default_rng(4)))
    nw = 32
    rng = np.random.default_rng(5)
    pos = np.stack([40.0 + 2 * rng.standard_normal(nw), np.abs(30 * rng.standard_normal(nw)) + 0.5],
                   axis=1)  # (ages close to 0: stretch moves propose negative ones)
    k = dict(args=[data, model, prior], seed=23, naima_style=True, store_blobs=False,
             nan_policy="reject")
    h = EnsembleSampler(nw, 2, na.lnprob, device=False, **k)
    d = EnsembleSampler(nw, 2, na.lnprob, device=True, **k)
    with np.errstate(all="ignore"):
        h.run_mcmc(pos, 20)
        d.run_mcmc(pos, 20)
        cd = d.get_chain()
    assert d.device is True and h.nan_proposals > 0 and d.nan_proposals == h.nan_proposals
    assert np.all(cd[:, :, 1] > 0)
    assert_allclose(cd, h.get_chain(), rtol=1e-8)


# ----------------------------------------------------------------------------- 9. the examples
def _example(name, *args):
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "examples", name)] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_pwn_cooled_example():
    out = _example("pwn_cooled.py", "32", "20", "40")
    assert "device loop: True" in out, out
    for key in ("break energy", "B [uG]", "log10(age/yr)"):
        assert any(key in ln for ln in out.splitlines()), out


def test_pevatron_secondaries_example():
    out = _example("pevatron_secondaries.py")
    for key in ("pi0 gamma rays", "synchrotron of the cooled secondaries", "break energy"):
        assert any(key in ln for ln in out.splitlines()), out
