"""The shapes at which nh_synchrotron is tested, each labelled with the launch its launcher picks
-- (C, tw, ktiles), include/naima_hip.h: nh_synchrotron_plan -- and how a case's grids, energies,
fields and weights are made.  test_synchrotron_host.py holds the labels to the planner, the table
to a scan of the planner over a lattice of shapes, and the inputs to the coverage they are there
for (no GPU); test_gpu_synchrotron.py runs every case against tests/synchrotron_np.py.

A case is (id, N, nG, nE, label, energies).  `energies` names where the photon energies lie, as
x = E/Ec at the LAST node of the grid for the middle field B = 10^-4.5 G (fields span 1e-6..1e-3 G,
a factor 31.6 in x either way):
  low   1e-12 .. 10     every energy live for every field (nA = tw)
  mix   1e-14 .. 1e6    live energies, then dead ones; more of them dead at weak fields
  high  30 .. 1e6       all dead at weak fields (nA = 0), a few live at strong ones (T / nA > 64)
  edge  mix, with the first energies moved to where walker 0 has x = 740 at the last node
        (i0 = nG - 1: nothing to integrate), x = 740 and x = 706 at the node before it (i0 = nG - 2:
        one segment), and x = 740 ten and a hundred nodes further down where the grid has them.
        The last weight of every walker is e^25 here, so that the x = 706 energy -- whose nodes'
        exp(-x) are normal numbers -- is held to the full bound, not to the underflow cap"""
import ctypes as C
import functools
import itertools

import numpy as np

import synchrotron_np as SNP

CASES = [
    # the C ladder, one tile
    ("c4-min", 3, 2, 1, (4, 64, 1), "low"),
    ("c4-max", 5, 64, 64, (4, 64, 1), "low"),
    ("c8-min", 5, 65, 64, (8, 64, 1), "mix"),
    ("c8-max", 5, 256, 40, (8, 64, 1), "edge"),
    ("c16-min", 5, 257, 64, (16, 64, 1), "edge"),
    ("c4-edge", 16, 40, 40, (4, 64, 1), "edge"),
    ("c4-high", 16, 64, 7, (4, 64, 1), "high"),
    ("c8-high", 16, 150, 13, (8, 64, 1), "high"),
    ("c16-high", 16, 300, 23, (16, 64, 1), "high"),
    ("c16-low", 9, 300, 64, (16, 64, 1), "low"),
    # plenty of workgroups: half the waves
    ("halve-16-not", 1024, 257, 2, (16, 64, 1), "mix"),
    ("halve-16", 1025, 257, 2, (8, 64, 1), "mix"),
    ("halve-8-not", 2048, 65, 1, (8, 64, 1), "low"),
    ("halve-8", 2049, 65, 1, (4, 64, 1), "low"),
    # several interleaved tiles per walker (nE > 64): at most 8 waves
    ("tiles-65", 5, 257, 65, (8, 33, 2), "mix"),
    ("tiles-66", 5, 257, 66, (8, 33, 2), "mix"),
    ("tiles-67", 5, 257, 67, (8, 23, 3), "mix"),
    ("tiles-130", 16, 257, 130, (8, 33, 4), "mix"),
    ("tiles-361", 9, 257, 361, (8, 33, 11), "edge"),
    ("tiles-65-c4", 5, 40, 65, (4, 33, 2), "mix"),
    ("tiles-66-c4", 5, 40, 66, (4, 33, 2), "mix"),
    ("tiles-67-c4", 5, 40, 67, (4, 23, 3), "mix"),
    ("tiles-130-c4", 16, 40, 130, (4, 33, 4), "high"),
    ("tiles-361-c4", 9, 40, 361, (4, 33, 11), "mix"),
    ("tiles-361-halved", 300, 257, 361, (4, 33, 11), "mix"),
    # dynamic LDS under / over 64 KB (24 nG + 32768 bytes), and the most the launcher takes
    ("lds-under-c16", 3, 1365, 40, (16, 64, 1), "mix"),
    ("lds-over-c16", 3, 1366, 40, (16, 64, 1), "mix"),
    ("lds-under-c8", 3, 1365, 65, (8, 33, 2), "mix"),
    ("lds-over-c8", 3, 1366, 65, (8, 33, 2), "mix"),
    ("lds-over-c4", 1025, 1366, 65, (4, 33, 2), "mix"),
    ("lds-max", 2, 5034, 40, (16, 64, 1), "mix"),
]
CASE_IDS = [c[0] for c in CASES]

# nh_synchrotron_lnprob's shapes (N, nG, nE) and the C of the instance with the epilogue
EPILOGUE = [(32, 40, 40, 4), (32, 150, 64, 8), (32, 300, 1, 16), (8, 1366, 40, 16),
            (32, 40, 1, 4), (32, 40, 64, 4), (32, 150, 1, 8), (32, 300, 64, 16),
            (1025, 1366, 64, 8)]
EPILOGUE_IDS = ["c4", "c8-64", "c16-1", "c16-lds", "c4-1", "c4-64", "c8-1", "c16-64",
                "c8-lds-halved"]

LATTICE = dict(N=(1, 5, 300, 1024, 1025, 2048, 2049, 4097),
               nG=(2, 40, 64, 65, 150, 256, 257, 1365, 1366, 5034),
               nE=(1, 40, 64, 65, 66, 67, 130, 361))

# every compiled instance k_synchrotron<4 / 8 / 16, with / without the epilogue> is reached.  What
# never happens while NH_SYN_TW and NH_SYN_C are unset: 16 waves on several tiles (nE > 64 caps C
# at 8) and the C = 4 instances above 64 KB of LDS with the epilogue (nG >= 1366 starts at 16 and
# is halved once)
UNREACHED = []
NEVER = [(16, "tiles", 0)]

LDS_LIMIT = 64 * 1024


def plan(N, nG, nE, want_epilogue=0):
    """(return code, (C, tw, ktiles, lds_bytes)) of nh_synchrotron_plan"""
    from naima_amd import _lib
    lib = _lib.load()
    o = [C.c_int(-1) for _ in range(4)]
    rc = lib.nh_synchrotron_plan(N, nG, nE, want_epilogue, *[C.byref(v) for v in o])
    return rc, tuple(v.value for v in o)


def variant(p, epi):
    """(C, 'one' | 'tiles', epilogue) of a plan"""
    return (p[0], "one" if p[2] == 1 else "tiles", int(epi))


def scan():
    """{(C, tile class, epilogue)} and {(C, over 64 KB, epilogue)} over LATTICE"""
    seen, lds = set(), set()
    L = LATTICE
    for N, nG, nE, epi in itertools.product(L["N"], L["nG"], L["nE"], (0, 1)):
        rc, p = plan(N, nG, nE, epi)
        if epi and nE > 64:
            assert rc != 0, (N, nG, nE)
            continue
        assert rc == 0, (N, nG, nE, epi)
        seen.add(variant(p, epi))
        lds.add((p[0], int(p[3] > LDS_LIMIT), epi))
    return seen, lds


# ---- grids ----------------------------------------------------------------------------------
MAX_DECADES = 150.0  # (gamma^2 must stay a float64: 15 per decade over 5034 nodes is 335 decades)
DENSITIES = {"d100": 100.0, "d40": 40.0, "d15": 15.0}  # nodes per decade: the 3-term, the
# 5-term and the log() form of syn_dlnP1 (nh_syn.h; max s^2 = 5.9e-5, 3.7e-4, > 9e-4)
MIXED_STEPS = (1 / 100.0, 1 / 40.0, 1 / 15.0)  # the "mixed" grid: runs of three segments of each


def grids_of(nG):
    """the grids a case of nG nodes runs on: the three log-uniform ones (all but 15 per decade at
    nG = 5034, which float64 cannot hold), and the mixed one up to nG = 257"""
    names = [n for n, d in DENSITIES.items() if (nG - 1) / d <= MAX_DECADES]
    if 16 <= nG <= 257:
        names.append("mixed")
    return names


@functools.lru_cache(maxsize=None)
def grid(nG, name):
    """(gam [nG], lx [nG-1]): centred on 1e5 below six decades, from 1e2 up to 9.5 decades
    (1e2..1e8 at least), and ending at 10^11.5 beyond that -- the grid grows DOWNWARDS, below
    gamma = 1, so that the photon energies and CS1 stay where a spectrum is a float64;
    lx = ln(gam[i+1]/gam[i]) rounded once from long double"""
    if name == "mixed":
        steps = np.array([MIXED_STEPS[(i // 3) % 3] for i in range(nG - 1)])
    else:
        steps = np.full(nG - 1, 1.0 / DENSITIES[name])
    span = steps.sum()
    lg0 = 5.0 - span / 2 if span < 6 else (2.0 if span <= 9.5 else 11.5 - span)
    lg = lg0 + np.concatenate([[0.0], np.cumsum(steps)])
    gam = 10.0 ** lg
    g = gam.astype(SNP.LD)
    lx = np.log(g[1:] / g[:-1]).astype(np.float64)
    gam.setflags(write=False), lx.setflags(write=False)
    return gam, lx


# ---- fields, energies, weights -----------------------------------------------------------------
NDIST = 16  # distinct walker rows: row r is distinct row r % 16, its weights times 2^-(r // 16)
B_MID = 10.0 ** -4.5
X_RANGE = {"low": (1e-12, 10.0), "mix": (1e-14, 1e6), "high": (30.0, 1e6), "edge": (1e-14, 1e6)}
BAD_B = {3: 0.0, 4: -1e-5, 5: np.nan, 6: np.inf}  # the bad walkers of a case with N >= 8
NAN_ROW = 7                                        # ... and the one with a NaN weight


def fields(N):
    """B [N][3] (the kernel reads column 0: ldB = 3), 1e-6..1e-3 G; walker 0 has the middle one"""
    R = min(N, NDIST)
    b = 10.0 ** (-4.5 + 1.5 * np.cos(np.arange(R) * 2.4))
    b[0] = B_MID
    if R > 1:
        b[1], b[R - 1] = 1e-6, 1e-3
    if N >= 8:
        for r, v in BAD_B.items():
            b[r] = v
    B = np.full((N, 3), -7.0)  # (a field nobody may read)
    B[:, 0] = b[np.arange(N) % NDIST]
    return B


def ec_ev(B, g):
    return float(3 * SNP._E * SNP._HBAR * SNP.LD(B) * SNP.LD(g) ** 2 / (2 * SNP._ME * SNP._C)
                 / SNP._ERG)


def energies(nE, gam, kind):
    lo, hi = X_RANGE[kind]
    ec = ec_ev(B_MID, gam[-1])
    E = np.geomspace(lo, hi, nE) * ec if nE > 1 else np.array([np.sqrt(lo * min(hi, 10.0)) * ec])
    if kind == "edge":
        nG = len(gam)
        at = [(740.0, nG - 1), (740.0, nG - 2), (706.0, nG - 2)]
        at += [(740.0, nG - 1 - j) for j in (10, 100) if nG - 1 - j > 0]
        for j, (xv, i) in enumerate(at[:max(1, nE // 4)]):
            E[j] = xv * ec_ev(B_MID, gam[i])
    return E


@functools.lru_cache(maxsize=None)
def make_case(cid, gname, seed=0):
    """the inputs of a case on one grid: dict(gam, lx, E, B [N][3], w, dlw [N][nG], dist = the
    distinct rows' (w, dlw, B), nan_node = the interior node where walker 7 has a NaN weight or
    None, planted)"""
    _, N, nG, nE, _, kind = CASES[CASE_IDS.index(cid)]
    return make_inputs(N, nG, nE, kind, gname, seed)


def make_inputs(N, nG, nE, kind, gname, seed=0):
    gam, lx = grid(nG, gname)
    E = energies(nE, gam, kind)
    B = fields(N)
    R = min(N, NDIST)
    d = SNP.make_inputs(seed + nG + 7 * nE, R, B[:R, 0], gam, lx, E,
                        ln_top=25.0 if kind == "edge" else None)
    wd, dlwd = d["w"], d["dlw"]
    nan_node = None
    if N >= 8 and nG >= 5:
        # a NaN weight inside walker 7's grid, between two positive weights (row 7 has no
        # planted zeros): live for some energies, dead for others wherever the case has both
        x = SNP.x_of(B[NAN_ROW, 0], gam, E)
        i0 = SNP.first_live(x)
        some = np.sort(i0[i0 < nG - 2])
        nan_node = int(min(max(some[len(some) // 2] + 1, 1), nG - 2)) if some.size else nG // 2
        wd[NAN_ROW, nan_node] = np.nan
    idx = np.arange(N) % NDIST
    w = wd[idx] * np.ldexp(1.0, -(np.arange(N) // NDIST))[:, None]
    return dict(gam=gam, lx=lx, E=E, B=B, w=w, dlw=dlwd[idx], dist=(wd, dlwd, B[:R, 0]),
                nan_node=nan_node, planted=d["planted"])


def check_x(d):
    """no x within 1e-9 relative of 746: the device's float64 x and the reference's agree on
    which nodes are live"""
    for b in d["dist"][2]:
        if b > 0 and np.isfinite(b):
            x = SNP.x_of(b, d["gam"], d["E"])
            assert np.abs(x / SNP.LD(SNP.X_DEAD) - 1).min() > 1e-9


def reference(d):
    """synchrotron_np.spectrum for every walker of make_inputs' rows: the distinct rows',
    scaled (exactly: long double does not underflow here)"""
    wd, dlwd, Bd = d["dist"]
    ref = SNP.spectrum(wd, dlwd, Bd, d["gam"], d["lx"], d["E"])
    N = len(d["w"])
    idx = np.arange(N) % NDIST
    sc = np.ldexp(SNP.LD(1), -(np.arange(N) // NDIST))[:, None]
    out = {k: ref[k][idx] * sc for k in ("spec", "S", "SX", "S_raw")}
    out["cs1"], out["i0"], out["s2"] = ref["cs1"][idx], ref["i0"][idx], ref["s2"]
    return out


@functools.lru_cache(maxsize=None)
def case_reference(cid, gname):
    d = make_case(cid, gname)
    check_x(d)
    return reference(d)


# ---- the kernel's work distribution, restated (nh_synchrotron.hip: k_synchrotron) -------------
def blocks_of(i0, nG, Cw, tw, ktiles):
    """for one walker's liveness map i0 [nE]: per tile, dict(nA, Cd, k [nA] the live energies in
    lane order, s0, s1 [Cd][nA] the chunk of thread ch * nA + a, idle = threads without a chunk)"""
    nE, T, nseg = len(i0), 64 * Cw, nG - 1
    out = []
    for tile in range(ktiles):
        k = np.arange(tw) * ktiles + tile
        k = k[k < nE]
        k = k[i0[k] < nG]
        nA = len(k)
        if nA == 0:
            out.append(dict(nA=0, Cd=0, k=k, idle=T))
            continue
        Cd = min(T // nA, 64)
        per = (nseg - i0[k] + Cd - 1) // Cd
        s0 = i0[k][None, :] + np.arange(Cd)[:, None] * per[None, :]
        s1 = np.minimum(nseg, s0 + per[None, :])
        out.append(dict(nA=nA, Cd=Cd, k=k, per=per, s0=s0, s1=s1, idle=T - Cd * nA))
    return out
