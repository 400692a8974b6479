"""The shapes at which nh_integrate_tables is tested, each labelled with the kernel variant its
launcher picks -- (rows_kernel, C, W, staged), include/naima_hip.h: nh_integrate_tables_plan --
and how a case's inputs are made.  test_integrate_host.py holds the labels to the planner and
the table to a scan of the planner over a lattice of shapes (no GPU); test_gpu_integrate.py runs
every case against tests/integrate_np.py.

A case is (id, N, nG, nK, nsplit, label).  The first groups are the smallest shapes that select
each variant; the "reach" group holds one shape for every other variant the scan finds."""
import ctypes as C
import itertools

import numpy as np

import integrate_np as INP

ROWS = (1, 0, 0, 0)

CASES = [
    # the C ladder at W = 1 (nG = 13..16: remainder loops of 0, 1, 2, 3 segments after 3 trips)
    ("c1-rem0", 16, 13, 64, 1, (0, 1, 1, 1)),
    ("c1-rem1", 16, 14, 64, 1, (0, 1, 1, 1)),
    ("c1-rem2", 16, 15, 64, 1, (0, 1, 1, 1)),
    ("c1-rem3", 16, 16, 64, 1, (0, 1, 1, 1)),
    ("c2", 16, 17, 64, 1, (0, 2, 1, 1)),
    ("c4", 16, 33, 64, 1, (0, 4, 1, 1)),
    ("c8", 16, 65, 64, 1, (0, 8, 1, 1)),
    ("c16", 16, 129, 64, 1, (0, 16, 1, 1)),
    ("w1-staged-max", 16, 3072, 64, 1, (0, 16, 1, 1)),
    ("w1-unstaged", 16, 3073, 64, 1, (0, 16, 1, 0)),
    # W = 2: 64 KB of LDS at C = 16 / the first unstaged grid, even and odd walker counts
    ("w2-staged-max", 512, 1536, 64, 1, (0, 16, 2, 1)),
    ("w2-unstaged", 512, 1537, 64, 1, (0, 16, 2, 0)),
    ("w2-odd-staged-max", 513, 1536, 64, 1, (0, 16, 2, 1)),
    ("w2-odd-unstaged", 513, 1537, 64, 1, (0, 16, 2, 0)),
    ("w2-one-column", 1024, 100, 1, 1, (0, 8, 2, 1)),
    # W = 4: two tiles, the second of one column, and a walker tail of one
    ("w4-c1", 4097, 15, 65, 1, (0, 1, 4, 1)),
    ("w4-c8", 4097, 65, 65, 1, (0, 8, 4, 1)),
    ("w4-unstaged", 4097, 769, 65, 1, (0, 8, 4, 0)),
    # partial 64-column tiles
    ("tile-63", 17, 40, 63, 1, (0, 4, 1, 1)),
    ("tile-65", 16, 40, 65, 1, (0, 4, 1, 1)),
    ("tile-130", 9, 40, 130, 1, (0, 4, 1, 1)),
    # planes: nseg no multiple of nsplit; fewer segments than planes
    ("split2", 16, 100, 64, 2, (0, 4, 1, 1)),
    ("split3", 16, 101, 64, 3, (0, 4, 1, 1)),
    ("split8", 16, 150, 65, 8, (0, 2, 1, 1)),
    ("split8-empty-planes", 16, 6, 64, 8, (0, 1, 1, 1)),
    ("split8-two-empty", 16, 13, 64, 8, (0, 1, 1, 1)),
    # k_integrate_rows: the edge shape, several workgroups with a lane loop, planes to zero
    ("rows", 3, 12, 5, 1, ROWS),
    ("rows-long", 15, 150, 64, 1, ROWS),
    ("rows-split3", 3, 6, 5, 3, ROWS),
    # reach: the remaining variants of the scan
    ("reach-w1-c8-unstaged", 16, 3073, 64, 2, (0, 8, 1, 0)),
    ("reach-w1-c4-unstaged", 511, 3073, 40, 8, (0, 4, 1, 0)),
    ("reach-w2-c1", 512, 15, 64, 1, (0, 1, 2, 1)),
    ("reach-w2-c2", 512, 17, 64, 1, (0, 2, 2, 1)),
    ("reach-w2-c4", 512, 33, 64, 1, (0, 4, 2, 1)),
    ("reach-w2-c8-unstaged", 512, 1537, 64, 2, (0, 8, 2, 0)),
    ("reach-w2-c4-unstaged", 511, 1537, 65, 8, (0, 4, 2, 0)),
    ("reach-w2-c2-unstaged", 511, 1537, 130, 8, (0, 2, 2, 0)),
    ("reach-w2-c1-unstaged", 4096, 1537, 1, 8, (0, 1, 2, 0)),
    ("reach-w4-c2", 4097, 17, 65, 1, (0, 2, 4, 1)),
    ("reach-w4-c4", 4097, 33, 65, 1, (0, 4, 4, 1)),
    ("reach-w4-c4-unstaged", 4097, 769, 65, 2, (0, 4, 4, 0)),
    ("reach-w4-c2-unstaged", 4097, 769, 65, 3, (0, 2, 4, 0)),
    ("reach-w4-c1-unstaged", 4097, 769, 65, 8, (0, 1, 4, 0)),
]
CASE_IDS = [c[0] for c in CASES]

# nh_integrate_tables_lnprob's shapes (N, nG, nK) and the (C, W) of the fused instance
FUSED = [(32, 150, 40, (16, 1)), (32, 100, 40, (8, 1)), (512, 150, 40, (16, 2)),
         (513, 100, 40, (8, 2))]
NOT_FUSED = [(32, 150, 65), (12, 150, 40)]  # two tiles; test_abi_last_producer_epilogues' shape

LATTICE = dict(N=(1, 15, 16, 511, 512, 513, 4096, 4097, 8192), nK=(1, 40, 63, 64, 65, 130),
               nG=(2, 13, 14, 15, 16, 17, 33, 65, 100, 129, 150, 768, 769, 1536, 1537, 3072, 3073),
               nsplit=(1, 2, 3, 8))

# compiled instances k_integrate_tables<C, W, *, staged> that no shape selects while NH_INT_W and
# NH_INT_C are unset: W = 4 means >= 2048 workgroups, which stop the C loop at 8; W = 1 means
# < 4096 workgroups and unstaged rows nG > 3072, which carry the C loop to 4 at least
UNREACHED = [(16, 4, 1), (16, 4, 0), (1, 1, 0), (2, 1, 0)]


def plan(N, nG, nK, nsplit=1, want_epilogue=0):
    """(return code, (rows_kernel, C, W, staged, fused)) of nh_integrate_tables_plan"""
    from naima_amd import _lib
    lib = _lib.load()
    o = [C.c_int(-1) for _ in range(5)]
    rc = lib.nh_integrate_tables_plan(N, nG, nK, nsplit, want_epilogue, *[C.byref(v) for v in o])
    return rc, tuple(v.value for v in o)


def scan():
    """{(rows_kernel, C, W, staged)}, {(C, W) of fused launches} over LATTICE"""
    seen, fused = set(), set()
    L = LATTICE
    for N, nK, nG, ns in itertools.product(L["N"], L["nK"], L["nG"], L["nsplit"]):
        rc, p = plan(N, nG, nK, ns, 1)
        assert rc == 0, (N, nG, nK, ns)
        seen.add(p[:4])
        if p[4]:
            fused.add(p[1:3])
    return seen, fused


# ---- inputs -------------------------------------------------------------------------------
NDIST = 8  # distinct walker rows: row r is distinct row r % 8 times 2^(r // 8 - 256), exactly


def row_scale(N):
    return np.ldexp(1.0, np.arange(N) // NDIST - 256)


def make_case(N, nG, nK, signed, seed=0):
    """the inputs of a case: dict(w, dlw [N][nG], lx, Kt, dlnKt, scale [nK], dist = the distinct
    rows' (w, dlw), nan_row = the walker whose w holds a NaN or None).  Non-negative contract
    unless `signed`."""
    R = min(N, NDIST)
    d = INP.make_inputs(seed + 1000 * signed, R, nG, nK)
    INP.plant_zeros(d, seed + 1)
    if signed and R >= 3:
        INP.plant_signed(d, seed + 2)
    idx = np.arange(N) % NDIST
    sc = row_scale(N)[:, None]
    w, dlw = d["w"][idx] * sc, d["dlw"][idx].copy()
    nan_row = None
    if signed and N >= 3:
        # an odd walker in the middle: second of a W = 2 pair, second of a W = 4 group.  Its NaN
        # sits at the node nearest the middle of the grid where no column has the segment AFTER
        # it ended by a zero node while the segment before it is live (there the forms differ in
        # whether a NaN u2 alone reaches the term) and some column has it live; node 0 has no
        # segment before it
        nan_row = (N // 2) | 1
        if nan_row >= N - 1:
            nan_row = 1
        u = w[nan_row][:, None] * d["Kt"]
        ok = [i for i in range(1, nG - 1)
              if not ((u[i + 1] == 0) & (u[i - 1] != 0)).any() and (u[i + 1] != 0).any()]
        node = min(ok, key=lambda i: abs(i - nG // 2)) if ok else 0
        w[nan_row, node] = np.nan
    scale = np.random.default_rng(seed + 3).uniform(0.5, 2.0, nK)
    return dict(w=w, dlw=dlw, lx=d["lx"], Kt=d["Kt"], dlnKt=d["dlnKt"], scale=scale,
                dist=(d["w"], d["dlw"]), nan_row=nan_row)


def reference(d, N, nsplit, scale):
    """(planes, S) [nsplit][N][nK] in long double for every walker of make_case's inputs: the
    reference of the distinct rows, scaled; of the NaN walker, on its own row"""
    wd, dlwd = d["dist"]
    p8, s8 = INP.integrate(wd, dlwd, d["lx"], d["Kt"], d["dlnKt"], scale, nsplit)
    idx = np.arange(N) % NDIST
    sc = row_scale(N).astype(INP.LD)[None, :, None]
    planes, S = p8[:, idx] * sc, s8[:, idx] * sc
    r = d["nan_row"]
    if r is not None:
        pn, sn = INP.integrate(d["w"][r:r + 1], d["dlw"][r:r + 1], d["lx"], d["Kt"], d["dlnKt"],
                               scale, nsplit)
        planes[:, r], S[:, r] = pn[:, 0], sn[:, 0]
    return planes, S
