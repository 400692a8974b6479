"""The reference and the case table of nh_integrate_tables' tests, checked without a GPU:
tests/integrate_np.py against the oracle's trapz_loglog and against mpmath, and
tests/integrate_cases.py against the planner the launcher itself asks
(nh_integrate_tables_plan)."""
import ctypes as C

import numpy as np
import pytest

import integrate_cases as IC
import integrate_np as INP


def _grid(lx):
    lnx = np.concatenate([[0.0], np.cumsum(lx.astype(INP.LD))])
    return np.exp(lnx).astype(np.float64)


def test_reference_against_the_oracle():
    """per segment against oracle.naima_np.trapz_loglog(y = u/x, x, intervals=True) at rtol 1e-13:
    zero nodes, sign changes and a negative walker everywhere; the power-law form where
    |dl| >= 2^-6, away from b + 1 -> 0 (there float64's x2 (x2/x1)^b - x1 cancels to
    eps/|dl| and the oracle is the less accurate of the two)"""
    from oracle import naima_np as O
    R, nG, nK = 4, 60, 9
    d = INP.plant_zeros(INP.make_inputs(5, R, nG, nK), 6)
    d["Kt"][20:, 3] *= -1.0
    d["Kt"][41:, 7] *= -1.0
    d["w"][2] *= -1.0
    x = _grid(d["lx"])
    lx = np.log(x[1:] / x[:-1])  # (what the oracle sees; within 1e-14 of the drawn one)
    t = INP.terms(d["w"], d["dlw"], lx, d["Kt"], d["dlnKt"])
    u = d["w"][:, :, None] * d["Kt"][None]
    want = O.trapz_loglog(u / x[None, :, None], x, axis=1, intervals=True)
    dl = d["dlw"][:, :-1, None] + d["dlnKt"][None, :-1]
    edge = (u[:, :-1] == 0) | (u[:, 1:] == 0) | (np.sign(u[:, :-1]) != np.sign(u[:, 1:]))
    held = edge | (np.abs(dl) >= 2.0 ** -6)
    assert edge.sum() > 100 and (u[:, :-1] * u[:, 1:] < 0).sum() >= 2 * R
    assert (held & ~edge).mean() > 0.75
    got = t.astype(np.float64)
    assert np.all(got[(u[:, :-1] == 0) | (u[:, 1:] == 0)] == 0.0)
    np.testing.assert_allclose(got[held], want[held], rtol=1e-13, atol=0)
    # the planes are the sums of their segments, S of their magnitudes
    planes, S = INP.integrate(d["w"], d["dlw"], lx, d["Kt"], d["dlnKt"], np.full(nK, 2.0), 3)
    hper = -(-(nG - 1) // 3)
    for h in range(3):
        seg = t[:, h * hper:(h + 1) * hper]
        assert np.array_equal(planes[h], 2 * seg.sum(axis=1))
        assert np.array_equal(S[h], 2 * np.abs(seg).sum(axis=1))
    assert (nG - 1) % 3 != 0


def _mpf(mp, v):
    """a long double as an mpf, exactly (two float64 pieces)"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - INP.LD(hi)))


def test_reference_against_mpmath():
    """one 12-node row that holds every rule -- a zero node, a -0.0 node, a sign change with a
    finite and one with a NaN dl, a NaN dl between nodes of one sign, dl = 0, |dl| down to
    2^-20 and up to 40 -- against the rules written out in mpmath at 40 digits"""
    import mpmath
    mp = mpmath.mp
    w = np.array([1.5, 2.25, 2.25, 3.0, 0.0, 1.0, 1.25, -0.75, -0.5, -0.0, 0.3, 0.3 * np.exp(40.0)])
    Kt = np.array([[0.7, 1.0], [0.7, 2.0], [0.7, 2.0 * np.exp(2.0 ** -20)], [1.1, 5.0], [1.3, 1.0],
                   [0.2, 1.0], [0.9, -1.0], [0.9, 1.0], [0.4, 3.0], [0.4, 1.0], [0.4, 0.5],
                   [0.4, 0.5]])
    with np.errstate(all="ignore"):
        dlw = np.zeros(12)
        dlw[:-1] = np.log(np.abs(w[1:] / w[:-1]))
        dK = np.zeros((12, 2))
        dK[:-1] = np.log(np.abs(Kt[1:] / Kt[:-1]))
    dlw[1], dK[1, 0] = 0.0, 0.0            # equal nodes: dl = 0 exactly
    dK[1, 1] = 2.0 ** -20
    dlw[~np.isfinite(dlw)] = 0.25          # (next to a zero node: any finite value, never used)
    dK[5, 0] = np.nan                      # NaN dl, nodes of one sign
    dK[6, :] = np.nan                      # NaN dl: at a sign change (k = 0), and not
    lx = np.linspace(0.02, 0.3, 11)
    scale = np.array([3.0, 0.125])
    planes, S = INP.integrate(w[None], dlw[None], lx, Kt, dK, scale, 2)
    old = mp.dps
    mp.dps = 40
    try:
        seen = set()
        for k in range(2):
            tot, mag = [mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(0)]
            for i in range(11):
                u1, u2 = mp.mpf(w[i]) * mp.mpf(Kt[i, k]), mp.mpf(w[i + 1]) * mp.mpf(Kt[i + 1, k])
                dl = float(dlw[i]) + float(dK[i, k])
                if u1 == 0 or u2 == 0:
                    term, rule = mp.mpf(0), "zero"
                elif (u1 < 0) != (u2 < 0) or dl != dl:
                    term = u1 * mp.mpf(lx[i])
                    rule = "sign" if dl == dl else "nan"
                elif dl == 0:
                    term, rule = u1 * mp.mpf(lx[i]), "flat"
                else:
                    m = mp.mpf(dlw[i]) + mp.mpf(dK[i, k])
                    term, rule = mp.mpf(lx[i]) * u1 * mp.expm1(m) / m, "plaw"
                seen.add(rule)
                tot[i // 6] += term
                mag[i // 6] += abs(term)
            for h in range(2):
                want, wmag = mp.mpf(scale[k]) * tot[h], mp.mpf(scale[k]) * mag[h]
                assert abs(_mpf(mp, planes[h, 0, k]) - want) <= mp.mpf(2) ** -60 * wmag, (h, k)
                assert abs(_mpf(mp, S[h, 0, k]) - wmag) <= mp.mpf(2) ** -60 * wmag, (h, k)
        assert seen == {"zero", "sign", "nan", "flat", "plaw"}
    finally:
        mp.dps = old


def test_generator_nodes_agree_with_their_log_ratios():
    """ln(u2/u1) of the generated nodes is dlw + dlnKt to 2 ulp of the ratio (2.3e-16 absolute
    + the rounding of the sum), the planted peaks sit where make_inputs says, and the planted
    zeros carry dlnKt = 1e300 on both adjacent segments and nowhere else"""
    d = INP.make_inputs(3, 8, 130, 70)
    u = d["w"].astype(INP.LD)[:, :, None] * d["Kt"].astype(INP.LD)[None]
    dl = d["dlw"][:, :-1, None] + d["dlnKt"][None, :-1]
    assert np.abs(np.log(u[:, 1:] / u[:, :-1]) - dl).max() < 4.5e-16
    assert np.abs(d["dlw"]).max() <= 1 and np.abs(d["dlnKt"]).max() <= 1
    i0, i1 = d["peaks"]
    assert np.array_equal(dl[:, i0, :8], np.tile(INP.PEAK_DL, (8, 1)))
    small = np.abs(dl) < 2.0 ** -10
    assert small[:, i0].any() and not small[:, i0].all() and not small[:, i1].any()
    INP.plant_zeros(d, 4)
    z = d["Kt"] == 0
    assert z[:, 1].all() and z[:, 64:].sum() > 0 and 0 < z[:, 2:64].sum() < 400
    assert np.array_equal(d["dlnKt"][:-1] == INP.DL_ZERO, z[:-1] | z[1:])
    assert np.all(d["dlnKt"][-1] == 0)


def test_big_rows_are_exact_copies():
    """row r of a case is distinct row r % 8 times a power of two, no two rows are equal, and the
    signed cases' NaN walker is an odd row with two whole neighbours"""
    d = IC.make_case(4097, 15, 65, signed=1)
    w = d["w"]
    r = d["nan_row"]
    assert r % 2 == 1 and 0 < r < 4096 and np.isnan(w[r]).sum() == 1
    assert not np.isnan(np.delete(w, r, axis=0)).any()
    assert np.array_equal(w[4096], d["dist"][0][0] * 2.0 ** 256)
    keep = np.delete(np.arange(4097), r)
    assert len({w[i].tobytes() for i in keep}) == 4096
    assert (np.abs(w[keep][w[keep] != 0]) > 1e-250).all() and (np.abs(w[keep]) < 1e250).all()


@pytest.mark.parametrize("case", IC.CASES, ids=IC.CASE_IDS)
def test_case_labels_are_the_planners(case):
    cid, N, nG, nK, nsplit, label = case
    rc, p = IC.plan(N, nG, nK, nsplit, 0)
    assert rc == 0 and p == label + (0,)
    assert (N * nK < 1024) == bool(label[0])
    if not label[0]:
        assert label[3] == int(label[2] * nG <= 3072)  # the rows fit 48 KB of LDS


def test_fused_shapes_are_the_planners():
    for N, nG, nK, cw in IC.FUSED:
        assert IC.plan(N, nG, nK, 1, 1) == (0, (0,) + cw + (1, 1))
        assert IC.plan(N, nG, nK, 1, 0) == (0, (0,) + cw + (1, 0))  # (nobody asked)
        assert IC.plan(N, nG, nK, 2, 1)[1][4] == 0                   # (a plane is no spectrum)
    for N, nG, nK in IC.NOT_FUSED:
        assert IC.plan(N, nG, nK, 1, 1)[1][4] == 0


def test_every_variant_of_the_scan_is_a_case():
    """the planner over LATTICE (overrides unset): every (rows_kernel, C, W, staged) it answers
    is the label of a case, every (C, W) it fuses is in FUSED, and the four (C, W, staged) of
    UNREACHED -- with the two sign forms, eight of the 60 + 8 compiled instances -- never
    appear"""
    import os
    assert "NH_INT_W" not in os.environ and "NH_INT_C" not in os.environ
    seen, fused = IC.scan()
    labels = {c[5] for c in IC.CASES}
    assert seen <= labels, seen - labels
    assert fused == {cw for _, _, _, cw in IC.FUSED}
    reached = {(c, w, s) for r, c, w, s in seen if not r}
    every = {(c, w, s) for c in (1, 2, 4, 8, 16) for w in (1, 2, 4) for s in (0, 1)}
    assert every - reached == set(IC.UNREACHED)


def test_planner_refusals():
    """what nh_integrate_tables refuses by its sizes, the planner refuses; N = 0 plans nothing"""
    from naima_amd import _lib
    for N, nG, nK, ns in [(16, 100, 64, 0), (16, 100, 64, 9), (16, 1, 64, 1), (16, 100, 0, 1),
                          (-1, 100, 64, 1), (2 ** 20, 2 ** 11, 64, 1), (16, 2 ** 22, 64, 1)]:
        rc, p = IC.plan(N, nG, nK, ns)
        assert rc != 0 and p == (0, 0, 0, 0, 0), (N, nG, nK, ns)
    assert IC.plan(0, 100, 64, 1, 1) == (0, (0, 0, 0, 0, 0))
    lib = _lib.load()
    o = [C.c_int(7) for _ in range(4)]
    assert lib.nh_integrate_tables_plan(16, 100, 64, 1, 0, None, *[C.byref(v) for v in o]) != 0
    assert b"NULL" in lib.nh_last_error()
