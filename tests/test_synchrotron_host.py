"""The reference and the case table of nh_synchrotron's tests, checked without a GPU:
tests/synchrotron_np.py against oracle.naima_np.synchrotron_spectrum and against mpmath,
tests/synchrotron_cases.py against the planner the launcher itself asks (nh_synchrotron_plan), and
the cases' inputs against the coverage they were made for, worked out from the reference's
liveness map and the kernel's work distribution restated in synchrotron_cases.blocks_of."""
import ctypes as C
import os

import numpy as np
import pytest

import synchrotron_cases as SC
import synchrotron_np as SNP

EPS = 2.0 ** -53
UNDER = 2.0 ** -960   # S before CS1 below this: an underflow element
ALL = [(c[0], g) for c in SC.CASES for g in SC.grids_of(c[2])]
ALL_IDS = ["%s-%s" % cg for cg in ALL]


def _good(B):
    return (B > 0) & np.isfinite(B)


@pytest.mark.parametrize("cid,gname", ALL, ids=ALL_IDS)
def test_reference_against_the_oracle(cid, gname):
    """the reference against oracle.naima_np.synchrotron_spectrum (nelec = w / gamma) on the case's
    distinct rows with a good field and no NaN weight: rtol 1e-12 where SX/S < 30; further down the
    exponential |diff| <= 1e-12 S + 16 eps SX (float64's x = E/Ec carries some eight roundings and
    its exp one more, each worth x times itself) + what a denormal node costs the oracle; the
    underflow elements only under their cap.
    This is looser than the rtol 1e-12 the issue states, in one place: a segment with
    |dl| < 2^-6 (planted, or met by chance: 3e-8 occurs) adds 4 eps / |dl| of its own term, and
    nothing else does where SX/S < 30.  There the oracle's y1 (x2 (x2/x1)^b - x1)/(b + 1) cancels
    to eps/|dl| -- it is the less accurate of the two; test_reference_against_mpmath holds the
    reference where the oracle cannot -- and below |dl| = 1e-10 lx it takes its log branch."""
    from oracle import naima_np as O
    d = SC.make_case(cid, gname)
    wd, dlwd, Bd = d["dist"]
    ref = SC.case_reference(cid, gname)  # (its first rows are the distinct ones, unscaled)
    for r in range(len(wd)):
        if not _good(Bd[r]) or np.isnan(wd[r]).any():
            continue
        t, x, dl = SNP.row_terms(wd[r], dlwd[r], Bd[r], d["gam"], d["lx"], d["E"])
        # (the oracle's cbrt(x)^4 overflows beyond x = 1e230: it gets the grid from the first node
        # on that has x < 1e150 for every energy -- the nodes before it are dead for all of them)
        lo = int(np.argmax(x.max(axis=0) < 1e150))
        got = O.synchrotron_spectrum(d["E"], d["gam"][lo:], (wd[r] / d["gam"])[lo:],
                                     Bd[r]).astype(SNP.LD)
        spec, S, SX = ref["spec"][r], ref["S"][r], ref["SX"][r]
        under = ref["S_raw"][r] < UNDER
        assert np.all(got[S == 0] == 0.0)
        assert np.all((got[under] >= 0) & (got[under] <= 2 * spec[under] + 2.0 ** -1000 *
                                           ref["cs1"][r][under]))
        near = ~under & (SX < 30 * S)
        far = ~under & ~near
        small = (np.abs(dl) < 2.0 ** -6) & (np.abs(dl) > 1e-10 * d["lx"][None, :]) & (t != 0)
        with np.errstate(all="ignore"):
            lost = ref["cs1"][r] * np.where(small, 4 * EPS * np.abs(t / dl), 0).sum(axis=1)
            # a node whose exp(-x) (x > 708) or whose y = nelec CS1 Gtilde is denormal in float64 is
            # 2^-1075 off: its relative error reaches the oracle's term, and through ln(y2/y1) its
            # exponent b + 1 = dl/lx
            ex = np.exp(-x)
            y = np.abs((wd[r] / d["gam"]).astype(SNP.LD)[None, :] * ref["cs1"][r][:, None]
                       * SNP.P_of(x) * ex)
            m = np.minimum(ex, np.where(y > 0, y, 1))
            en = np.where((x <= SNP.X_DEAD) & (m < 2.0 ** -1022), SNP.LD(2) ** -1075 / m, SNP.LD(0))
            deno = ref["cs1"][r] * (np.abs(t) * (en[:, 1:] + en[:, :-1])
                                    * (1 + 1 / np.abs(dl))).sum(axis=1)
        err = np.abs(got - spec)
        assert np.all(err[near] <= 1e-12 * S[near] + lost[near]), (r, (err / S)[near].max())
        assert np.all(err[far] <= 1e-12 * S[far] + 16 * EPS * SX[far] + lost[far] + deno[far]), r


def _mpf(mp, v):
    """a long double as an mpf, exactly (two float64 pieces)"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - SNP.LD(hi)))


def test_reference_against_mpmath():
    """one 12-node row that holds every rule -- dead nodes, one of them with a NaN weight, an
    interior zero weight marked +-1e300, a run of zeros at the top, a NaN weight inside the live
    range of one energy and below that of another, |dl| < 1e-16, |dl| = 2^-20 and |dl| > 30 --
    against the rules written out in mpmath at 40 digits"""
    import mpmath
    mp = mpmath.mp
    gam = np.geomspace(1e3, 1e6, 12)
    lx = np.log(gam[1:] / gam[:-1])
    B = 2e-5
    ec = SC.ec_ev(B, gam[-1])
    E = np.array([5e-4, 0.02, 10.0, 2000.0]) * ec  # x at the last node: live from 0, 3, 8, never
    w = np.array([3.0, np.nan, 1.5, 1.0, 0.8, 0.0, 0.5, 0.45, 0.4, 0.2, 0.0, 0.0])
    with np.errstate(all="ignore"):
        dlw = np.zeros(12)
        dlw[:-1] = np.log(w[1:] / w[:-1])
    dlw[[4, 9, 10]], dlw[5] = -1e300, 1e300
    dlw[[0, 1]] = 0.3
    x = SNP.x_of(B, gam, E)
    i0 = SNP.first_live(x)
    assert list(i0) == [0, 3, 8, 12]
    # energy 1: dl = 0 in segment 6 and 2^-20 in segment 3, each to an ulp of its dlw
    for k, i, target in ((1, 6, 0.0), (1, 3, 2.0 ** -20)):
        P = SNP.P_of(x[k, i:i + 2])
        rest = np.log1p((P[1] - P[0]) / P[0]) - (x[k, i + 1] - x[k, i])
        dlw[i] = np.float64(SNP.LD(target) - rest)
    dlw[7] = 33.0  # (a log-ratio is an input of its own: it need not agree with the weights)
    t, _, dl = SNP.row_terms(w, dlw, B, gam, lx, E)
    assert abs(float(dl[1, 6])) < 1e-15 and abs(float(dl[1, 3]) - 2.0 ** -20) < 1e-13
    ref = SNP.spectrum(w[None], dlw[None], np.array([B]), gam, lx, E)
    assert np.isnan(ref["spec"][0, 0]) and np.all(ref["spec"][0, 3] == 0)
    assert list(ref["i0"][0]) == [0, 3, 8, 12]
    old = mp.dps
    mp.dps = 40
    try:
        seen = set()
        m = lambda v: mp.mpf(float(v))
        e, c, hbar, me, erg = (m(SNP._E), m(SNP._C), m(SNP._HBAR), m(SNP._ME), m(SNP._ERG))

        def node(k, i):
            xx = m(E[k]) * erg * 2 * me * c / (3 * e * hbar * m(B)) / m(gam[i]) ** 2
            cb = mp.cbrt(xx)
            P = (m(1.808) * cb / mp.sqrt(1 + m(3.4) * cb ** 2)
                 * (1 + m(2.210) * cb ** 2 + m(0.347) * cb ** 4)
                 / (1 + m(1.353) * cb ** 2 + m(0.217) * cb ** 4))
            if xx > 746:
                return xx, P, mp.mpf(0)
            return xx, P, (mp.nan if w[i] != w[i] else m(w[i]) * P * mp.exp(-xx))

        for k in (1, 2, 3):
            tot = mag = magx = mp.mpf(0)
            for i in range(11):
                x1, P1, u1 = node(k, i)
                x2, P2, u2 = node(k, i + 1)
                ddl = m(dlw[i]) + mp.log(P2 / P1) - (x2 - x1)
                if u1 == 0 or u2 == 0:
                    term, rule = mp.mpf(0), "zero" if x1 <= 746 else "dead"
                elif abs(ddl) < mp.mpf(10) ** -15:
                    term, rule = u1 * m(lx[i]), "flat"  # (expm1(dl)/dl - 1 = dl/2 < 2^-58)
                else:
                    term, rule = m(lx[i]) * u1 * mp.expm1(ddl) / ddl, "plaw"
                    if abs(ddl) > 30:
                        rule = "steep"
                assert not mp.isnan(term)
                seen.add(rule)
                tot += term
                mag += abs(term)
                magx += abs(term) * max(x1, x2)
            cs1 = ((mp.sqrt(3) * e ** 3 * m(B))
                   / (2 * mp.pi * me * c ** 2 * hbar * m(E[k]) * erg) * erg)
            tol = mp.mpf(2) ** -58
            assert abs(_mpf(mp, ref["spec"][0, k]) - cs1 * tot) <= tol * cs1 * mag, k
            assert abs(_mpf(mp, ref["S"][0, k]) - cs1 * mag) <= tol * cs1 * mag, k
            assert abs(_mpf(mp, ref["SX"][0, k]) - cs1 * magx) <= tol * cs1 * magx, k
        assert seen == {"zero", "dead", "flat", "plaw", "steep"}
        # energy 0 reads the NaN weight at node 1: segments 0 and 1 are NaN, the others are not
        assert np.isnan(t[0, :2]).all() and not np.isnan(t[0, 2:]).any()
    finally:
        mp.dps = old


def test_generator_nodes_agree_with_their_log_ratios():
    """ln(w2/w1) of the generated weights is dlw to 2 ulp of the ratio, dlw are multiples of 2^-20
    but at the planted segments, whose total dl is the target to an ulp of dlw (5e-16: |dlw| < 8),
    and the planted zeros carry -+1e300 on their segments and nowhere else"""
    d = SC.make_case("tiles-130", "d100")
    wd, dlwd, Bd = d["dist"]
    planted = {(r, i) for r, k, i, t in d["planted"]}
    assert len(planted) == 12 and {t for r, k, i, t in d["planted"]} == set(SNP.PLANT_DL)
    for r in range(16):
        w = wd[r].astype(SNP.LD)
        pos = (wd[r, :-1] > 0) & (wd[r, 1:] > 0)
        with np.errstate(all="ignore"):
            got = np.log(w[1:] / w[:-1])
        assert np.abs(got - dlwd[r, :-1])[pos].max() < 4.5e-16
        assert np.all(np.abs(dlwd[r, :-1][~pos & ~np.isnan(wd[r, :-1]) & ~np.isnan(wd[r, 1:])])
                      == SNP.DL_ZERO)
        grid20 = dlwd[r, :-1] * 2.0 ** 20
        off = [i for i in np.flatnonzero(pos) if grid20[i] != np.rint(grid20[i])]
        mine = {i for rr, i in planted if rr == r}
        assert set(off) <= mine
        assert np.all(np.abs(np.delete(dlwd[r, :-1], sorted(mine))[np.delete(pos, sorted(mine))])
                      < 0.1)
        assert np.all(np.abs(dlwd[r, sorted(mine)]) < 8)
        assert wd[r][~np.isnan(wd[r])].max() <= 1.0
    for r, k, i, target in d["planted"]:
        _, _, dl = SNP.row_terms(wd[r], dlwd[r], Bd[r], d["gam"], d["lx"], d["E"])
        assert abs(float(dl[k, i] - SNP.LD(target))) < 5e-16
    assert (wd[1] == 0).sum() == 257 // 8 and (wd[2] == 0).sum() == 1
    assert np.isnan(wd[SC.NAN_ROW]).sum() == 1 and 0 < d["nan_node"] < 256


def test_big_rows_are_exact_copies():
    """row r of a case is distinct row r % 16 with its weights times 2^-(r // 16): same field, same
    log-ratios, and the reference scales with it"""
    d = SC.make_case("halve-8", "d15")
    w, wd = d["w"], d["dist"][0]
    assert np.array_equal(w[2048], wd[0] * 2.0 ** -128)
    assert np.array_equal(w[:16], wd, equal_nan=True)
    assert np.array_equal(d["B"][16:32, 0], d["B"][:16, 0], equal_nan=True)
    assert np.all(d["B"][:, 1:] == -7.0)
    ref = SC.case_reference("halve-8", "d15")
    assert np.array_equal(ref["spec"][2048], ref["spec"][0] * SNP.LD(2.0) ** -128)
    assert (w[~np.isnan(w) & (w > 0)] > 1e-200).all()


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_case_labels_are_the_planners(case):
    cid, N, nG, nE, label, _ = case
    rc, p = SC.plan(N, nG, nE, 0)
    assert rc == 0 and p[:3] == label
    assert p[3] == 24 * nG + 32768 and p[2] == -(-nE // p[1])
    assert (p[2] > 1) == (nE > 64)


def test_epilogue_shapes_are_the_planners():
    for N, nG, nE, Cw in SC.EPILOGUE:
        assert SC.plan(N, nG, nE, 1) == (0, (Cw, 64, 1, 24 * nG + 32768))
    assert {(s[1], s[2]) for s in SC.EPILOGUE} >= {(40, 40), (150, 64), (300, 1), (1366, 40)}
    assert {s[2] for s in SC.EPILOGUE if s[2] in (1, 64)} == {1, 64}


def test_every_variant_of_the_scan_is_a_case():
    """the planner over LATTICE (overrides unset): every (C, one tile | several, epilogue) it
    answers is a case's or an epilogue shape's, all six compiled instances are among them, and so
    is every (C, over 64 KB of LDS, epilogue) -- the launches that raise the kernel's limit"""
    assert "NH_SYN_TW" not in os.environ and "NH_SYN_C" not in os.environ
    seen, lds = SC.scan()
    have = {SC.variant(SC.plan(c[1], c[2], c[3], 0)[1], 0) for c in SC.CASES}
    have |= {SC.variant(SC.plan(N, nG, nE, 1)[1], 1) for N, nG, nE, _ in SC.EPILOGUE}
    assert seen == have
    assert {(c, e) for c, _, e in seen} == {(c, e) for c in (4, 8, 16) for e in (0, 1)}
    assert not (set(SC.NEVER) & seen) and SC.UNREACHED == []
    have_lds = {(p[0], int(p[3] > SC.LDS_LIMIT), 0)
                for p in (SC.plan(c[1], c[2], c[3], 0)[1] for c in SC.CASES)}
    have_lds |= {(p[0], int(p[3] > SC.LDS_LIMIT), 1)
                 for p in (SC.plan(N, nG, nE, 1)[1] for N, nG, nE, _ in SC.EPILOGUE)}
    assert lds == have_lds
    assert (4, 1, 1) not in lds


def _rule_before(N, nG, nE, epi):
    """the launcher's choice as launch_synchrotron made it before the planner existed"""
    nseg = nG - 1
    Cw = 16 if nseg >= 256 else (8 if nseg >= 64 else 4)
    tw = 64
    if nE > 64 and not epi:
        Cw = min(Cw, 8)
        kt = (nE + 32) // 33
        tw = (nE + kt - 1) // kt
    ktiles = (nE + tw - 1) // tw
    if ktiles * N * Cw > 16384 and Cw > 4:
        Cw //= 2
    return Cw, tw, ktiles, (3 * nG + 64 * 64) * 8


# the synchrotron launches of the benchmark's workloads (walkers of a launch, electron grid,
# photon energies): cfg2, cfg3 at three ensemble sizes, cfg4's data and data + seed energies
WORKLOAD_SHAPES = [(64, 300, 179), (256, 300, 179), (128, 570, 64), (256, 570, 64), (512, 570, 64),
                   (128, 869, 261), (128, 869, 361), (512, 869, 361), (1024, 869, 361)]


def test_planner_is_the_rule_the_launcher_had():
    """over LATTICE and the workloads' shapes the planner answers what the launcher's inline
    code answered: the same instance, tile width and LDS for every shape"""
    L = SC.LATTICE
    shapes = [(N, nG, nE) for N in L["N"] for nG in L["nG"] for nE in L["nE"]] + WORKLOAD_SHAPES
    for N, nG, nE in shapes:
        for epi in (0, 1):
            if epi and nE > 64:
                continue
            assert SC.plan(N, nG, nE, epi) == (0, _rule_before(N, nG, nE, epi)), (N, nG, nE, epi)
    print([(s, SC.plan(*s)[1]) for s in WORKLOAD_SHAPES])


def test_planner_refusals():
    """what the entry points refuse by their sizes, the planner refuses: nG < 2, nE < 1, N < 0, the
    epilogue with nE > 64, more than 150 KB of LDS; N = 0 plans nothing"""
    from naima_amd import _lib
    for N, nG, nE, epi in [(16, 1, 40, 0), (16, 100, 0, 0), (-1, 100, 40, 0), (16, 100, 65, 1),
                           (2, 5035, 40, 0), (2, 5035, 40, 1), (2, 2 ** 30, 40, 0)]:
        rc, p = SC.plan(N, nG, nE, epi)
        assert rc != 0 and p == (0, 0, 0, 0), (N, nG, nE, epi)
    assert SC.plan(2, 5034, 40, 0) == (0, (16, 64, 1, 153584))
    assert SC.plan(0, 100, 40, 1) == (0, (0, 0, 0, 0))
    assert SC.plan(16, 100, 65, 0)[0] == 0
    lib = _lib.load()
    o = [C.c_int(7) for _ in range(3)]
    assert lib.nh_synchrotron_plan(16, 100, 40, 0, None, *[C.byref(v) for v in o]) != 0
    assert b"NULL" in lib.nh_last_error()


BALLOT_CASES = ("c4-edge", "c8-min", "c16-min", "tiles-130")


def _ballots(blk):
    """the lanes that meet in one ballot of nh_seg_pos / syn_dlnP1: {(wave, key): [(a, segment)]}
    with key = ("loop", j) for the j-th segment of a chunk taken by the two-per-trip loop and
    ("rem",) for the odd one after it"""
    out = {}
    nA, Cd = blk["nA"], blk["Cd"]
    for ch in range(Cd):
        for a in range(nA):
            s0, s1 = int(blk["s0"][ch, a]), int(blk["s1"][ch, a])
            n = max(0, s1 - s0)
            wave = (ch * nA + a) // 64
            for j in range(n):
                key = ("loop", j) if j < 2 * (n // 2) else ("rem",)
                out.setdefault((wave, key), []).append((a, s0 + j))
    return out


def test_cases_cover_what_they_are_there_for():
    """from the reference's liveness map, across the cases: nA = 0, 1, 64 and values that do not
    divide the workgroup; T / nA > 64 (the cap on chunks); per = 0 and per = 1; chunks of odd and
    of even length, empty chunks behind the last segment; i0 = nG - 1 and nG - 2; a whole tile
    dead beside live ones, a block with every energy live and one with some dead; each form of
    syn_dlnP1 on its grid and all three in one ballot on the mixed one; a planted |dl| < 2^-10
    in one ballot with a lane above it"""
    nAs, pers, lens, capped, idle, empty_chunk = set(), set(), set(), False, False, False
    tails, tile_dead, all_live, some_dead = set(), False, False, False
    forms, mixed_ballot, both_sides = {}, False, False
    for cid, N, nG, nE, label, _ in SC.CASES:
        Cw, tw, kt = label
        for gname in SC.grids_of(nG):
            d = SC.make_case(cid, gname)
            ref = SC.case_reference(cid, gname)
            R = min(N, SC.NDIST)
            for r in range(R):
                if not _good(d["B"][r, 0]):
                    continue
                i0 = ref["i0"][r]
                tails |= set((nG - i0[i0 < nG]).tolist())
                blocks = SC.blocks_of(i0, nG, Cw, tw, kt)
                counts = [b["nA"] for b in blocks]
                tile_dead |= kt > 1 and 0 in counts and max(counts) > 0
                for tile, b in enumerate(blocks):
                    nAs.add(b["nA"])
                    if b["nA"] == 0:
                        continue
                    ntile = len(range(tile, nE, kt))
                    all_live |= b["nA"] == ntile and ntile > 1
                    some_dead |= 0 < b["nA"] < ntile
                    capped |= (64 * Cw) // b["nA"] > 64
                    idle |= b["idle"] > 0 and (64 * Cw) % b["nA"] != 0
                    pers |= set(b["per"].tolist())
                    n = b["s1"] - b["s0"]
                    empty_chunk |= bool((n[:, b["per"] > 0] <= 0).any())
                    lens |= set((n[n > 0] % 2).tolist())
            # the forms of syn_dlnP1 and the planted log-ratios, ballot by ballot, on the blocks
            # of walker 0 and of the walkers with a planted |dl| < 2^-10, at four cases
            if cid not in BALLOT_CASES:
                continue
            for r in sorted({0} | {p[0] for p in d["planted"] if abs(p[3]) < 2.0 ** -10}):
                if not _good(d["B"][r, 0]) or np.isnan(d["dist"][0][r]).any():
                    continue
                _, x, dl = SNP.row_terms(d["dist"][0][r], d["dist"][1][r], d["B"][r, 0], d["gam"],
                                         d["lx"], d["E"])
                P = SNP.P_of(x).astype(np.float64)
                s2 = ((P[:, 1:] - P[:, :-1]) / (P[:, 1:] + P[:, :-1])) ** 2
                cls = np.digitize(s2, [1e-4, 9e-4])
                blocks = SC.blocks_of(ref["i0"][r], nG, Cw, tw, kt)
                mine = [(k, i, t) for rr, k, i, t in d["planted"] if rr == r]
                for tile, b in enumerate(blocks):
                    if b["nA"] == 0:
                        continue
                    for (wave, key), lanes in _ballots(b).items():
                        ks = b["k"][[a for a, _ in lanes]]
                        ss = np.array([s for _, s in lanes])
                        c = set(cls[ks, ss].tolist())
                        forms.setdefault(gname, set()).add(max(c))
                        mixed_ballot |= gname == "mixed" and c == {0, 1, 2}
                        for k, i, t in mine:
                            hit = (ks == k) & (ss == i)
                            if hit.any() and abs(t) < 2.0 ** -10:
                                both_sides |= bool((np.abs(dl[ks, ss]) >= 2.0 ** -10).any())
    assert {0, 1, 64} <= nAs and capped and idle
    assert {0, 1} <= pers and lens == {0, 1} and empty_chunk
    assert {1, 2} <= tails
    assert tile_dead and all_live and some_dead
    # (a ballot takes the form of its coarsest lane; far down the exponential P is flat and
    # every grid is fine)
    assert forms["d100"] == {0} and max(forms["d40"]) == 1 and max(forms["d15"]) == 2
    assert forms["mixed"] == {0, 1, 2} and mixed_ballot
    assert both_sides


@pytest.mark.parametrize("cid,gname", ALL, ids=ALL_IDS)
def test_every_case_takes_its_grids_form(cid, gname):
    """from the largest s^2 among a case's live segments (all walkers): at 100 nodes per decade no
    segment leaves the three-term form, at 40 some need five terms and none the logarithm, at 15
    some need the logarithm, and the mixed grid has segments of all three.  Not the four `high`
    cases on the coarser grids: their energies are live only from x = 0.95 at the last node on,
    down the exponential, where P is flat and s small on any grid"""
    s2 = SC.case_reference(cid, gname)["s2"]
    high = SC.CASES[SC.CASE_IDS.index(cid)][5] == "high"
    if gname == "d100":
        assert 0 < s2[0] < 6e-5 and s2[1] == 0 and s2[2] == 0
    elif gname == "d40":
        assert s2[2] == 0 and (high or 1e-4 < s2[1] < 3.7e-4)
    elif gname == "d15":
        assert high or s2[2] > 9e-4
    else:
        assert s2[0] > 0 and (high or (s2[1] > 1e-4 and s2[2] > 9e-4))


@pytest.mark.parametrize("cid,gname", ALL, ids=ALL_IDS)
def test_underflow_elements_are_few(cid, gname):
    """an element whose S before CS1 is below 2^-960 is held only to 0 <= out <= 2 ref +
    2^-1000 CS1 on the device: at most 5 % of a case's live elements are such, and the energy at
    x = 706 of the edge cases (whose exp(-x) are normal numbers) is not one"""
    ref = SC.case_reference(cid, gname)
    live = ~np.isnan(ref["spec"]) & (ref["S"] > 0)
    under = live & (ref["S_raw"] < UNDER)
    assert under.sum() <= 0.05 * live.sum(), (under.sum(), live.sum())
    case = SC.CASES[SC.CASE_IDS.index(cid)]
    if case[5] == "edge" and case[3] >= 12:
        nG = case[2]
        # (x = 706 at node nG - 2 is 739 at the node before it on the finest grid: live too)
        assert nG - 3 <= ref["i0"][0, 2] <= nG - 2 and live[0, 2] and not under[0, 2]
        assert ref["i0"][0, 0] == nG - 1 and ref["S"][0, 0] == 0
        assert ref["SX"][0, 2] > 500 * ref["S"][0, 2]
