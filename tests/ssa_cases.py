"""The shapes at which nh_syn_absorption is tested, each labelled with the launch its planner
picks -- (C, tw, ktiles) of nh_syn_absorption_plan -- and how a case's inputs are made.  Grids,
fields, energies and weights are tests/synchrotron_cases.py's (make_inputs: bad fields in rows
3..6, a NaN weight in row 7, zero nodes in rows 1, 2 mod 4); its planted segments, whose total
log-ratio sits around the series threshold 2^-10 of the EMISSION's integrand, are planted again
for the absorption's: dl = dlw - lx + ln(Q2/Q1) - (x2 - x1).  test_ssa_host.py holds the labels to
the planner and the inputs to what they are there for (no GPU); test_gpu_ssa.py runs every case
against tests/ssa_np.py.

The smallest shapes that reach every instance k_syn_absorption<4 / 8 / 16>, one tile and several,
the halving of the waves above 16384 per launch, dynamic LDS over 64 KB and the most the launcher
takes; N >= 9 everywhere, so that every case has the bad-field rows and the NaN-weight row;
nE = 1, 12, 64 and multi-tile values."""
import ctypes as C
import functools

import numpy as np

import ssa_np as ANP
import synchrotron_cases as SC
import synchrotron_np as SNP

CASES = [
    ("c4-1", 9, 40, 1, (4, 64, 1), "low"),
    ("c4-12", 9, 40, 12, (4, 64, 1), "edge"),
    ("c4-64", 9, 64, 64, (4, 64, 1), "mix"),
    ("c8-12", 9, 65, 12, (8, 64, 1), "mix"),
    ("c8-64", 9, 256, 64, (8, 64, 1), "edge"),
    ("c16-12", 9, 257, 12, (16, 64, 1), "high"),
    ("c16-64", 9, 300, 64, (16, 64, 1), "low"),
    ("halve-16", 1025, 257, 1, (8, 64, 1), "mix"),
    ("halve-8", 2049, 65, 1, (4, 64, 1), "low"),
    ("tiles-c8", 9, 257, 67, (8, 23, 3), "mix"),
    ("tiles-c4", 9, 40, 130, (4, 33, 4), "edge"),
    ("lds-over", 9, 1366, 12, (16, 64, 1), "mix"),
    ("lds-max", 9, 5034, 12, (16, 64, 1), "mix"),
]
CASE_IDS = [c[0] for c in CASES]
grids_of = SC.grids_of
NDIST, BAD_B, NAN_ROW = SC.NDIST, SC.BAD_B, SC.NAN_ROW


def plan(N, nG, nE):
    """(return code, (C, tw, ktiles, lds_bytes)) of nh_syn_absorption_plan"""
    from naima_amd import _lib
    lib = _lib.load()
    o = [C.c_int(-1) for _ in range(4)]
    rc = lib.nh_syn_absorption_plan(N, nG, nE, *[C.byref(v) for v in o])
    return rc, tuple(v.value for v in o)


def make_inputs(N, nG, nE, kind, gname, seed=0):
    """synchrotron_cases.make_inputs with every planted segment (r, k, i, target) moved to the
    absorption's integrand: dlw[r][i] changes by what the two integrands' log-ratios differ by,
    and the weights above the segment are scaled by the exponential of the float64 change, in
    long double (a second rounding of those weights: 4 eps between a weight ratio and dlw
    instead of 2)"""
    d = dict(SC.make_inputs(N, nG, nE, kind, gname, seed))
    wd, dlwd, Bd = (np.array(a) for a in d["dist"])
    gam, lx, E = d["gam"], d["lx"], d["E"]
    for r, k, i, target in d["planted"]:
        x = SNP.x_of(Bd[r], gam, E)[k, i:i + 2]
        Q = ANP.Q_of(x)
        rest = np.log1p((Q[1] - Q[0]) / Q[0]) - (x[1] - x[0]) - SNP.LD(lx[i])
        new = np.float64(SNP.LD(target) - rest)
        scale = np.exp(SNP.LD(new) - SNP.LD(dlwd[r, i]))
        dlwd[r, i] = new
        wd[r, i + 1:] = (wd[r, i + 1:].astype(SNP.LD) * scale).astype(np.float64)
    idx = np.arange(N) % NDIST
    d["dist"] = (wd, dlwd, Bd)
    d["w"] = wd[idx] * np.ldexp(1.0, -(np.arange(N) // NDIST))[:, None]
    d["dlw"] = dlwd[idx]
    return d


@functools.lru_cache(maxsize=None)
def make_case(cid, gname):
    _, N, nG, nE, _, kind = CASES[CASE_IDS.index(cid)]
    return make_inputs(N, nG, nE, kind, gname)


def reference(d):
    """ssa_np.kappa for every walker of make_inputs' rows: the distinct rows', scaled"""
    wd, dlwd, Bd = d["dist"]
    ref = ANP.kappa(wd, dlwd, Bd, d["gam"], d["lx"], d["E"])
    N = len(d["w"])
    idx = np.arange(N) % NDIST
    sc = np.ldexp(SNP.LD(1), -(np.arange(N) // NDIST))[:, None]
    out = {k: ref[k][idx] * sc for k in ("kappa", "S", "SX", "S_raw")}
    out["pref"], out["i0"], out["s2"] = ref["pref"][idx], ref["i0"][idx], ref["s2"]
    return out


@functools.lru_cache(maxsize=None)
def case_reference(cid, gname):
    d = make_case(cid, gname)
    SC.check_x(d)
    return reference(d)


# ---- nh_ssa_apply: optical depths on both sides of every crossover -----------------------------
# tau from 1e-12 to 1e4; around the sphere's hand-over to its series at tau = 1 (and the same
# values for the slab, which has none); 0 exactly
APPLY_TAU = np.concatenate([
    [0.0], np.geomspace(1e-12, 1e4, 33),
    [1 - 2.0 ** -52, 1.0, 1 + 2.0 ** -51, 0.999, 1.001, 0.5, 0.75, 0.9, 1.1, 2.0, 30.0, 700.0,
     745.0, 800.0]])
