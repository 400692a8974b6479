"""Case lists of the cooled-electron tests (tests/test_cooling_host.py, tests/test_gpu_cooling.py)."""
import numpy as np

YR = 31557600.0

# ---- the closed form: PowerLaw injection, synchrotron losses only ----------------------------
CF = dict(Q0=1e36, e0=1e12, alpha=2.3, B_G=1e-4, Emin=1e9, Emax=510.998e12, npd=100)
# ages [s]: the steady state; the break in the middle of the grid (t_cool = 1.25e3 yr at
# 1 TeV in 100 uG); so short that E* lies in E_i's own segment at every node and the
# first-order departure from Q age, a age Emax = 1.3e-15, is below rounding
CF_AGES = (np.inf, 1.25e3 * YR, 1e-7)

# ---- injections of the restatement-against-quad test and of the kernel test -------------------
# (kind, rows as nh_particle_weights takes them: [A, e0, alpha, e_cutoff, beta, e_break, alpha_2, -])
INJECTIONS = {
    "PowerLaw": (0, [1e36, 1e12, 2.3, 0, 1, 0, 0, 0]),
    "ECPL": (1, [1e36, 1e12, 2.0, 5e13, 1.0, 0, 0, 0]),
    "BPL": (2, [1e36, 1e12, 1.5, 0, 1, 3.3e11, 2.5, 0]),
    "ECBPL": (3, [1e36, 1e12, 1.5, 8e13, 2.0, 3.3e11, 2.5, 0]),
    "LogParabola": (4, [1e36, 1e12, 2.0, 0, 0.15, 0, 0, 0]),
    # the cut-off far below the grid: exp(-(E/e_c)^beta) underflows, every node is an exact zero
    # above a few hundred e_c and the whole grid is zero for this one
    "ECPL_cut_below_grid": (1, [1e36, 1e12, 2.0, 1e5, 1.0, 0, 0, 0]),
    # the same with zeros at the upper nodes only
    "ECPL_zeros_on_top": (1, [1e36, 1e12, 2.0, 2e9, 1.0, 0, 0, 0]),
}


def injection_np(kind, p, e):
    """the five distributions of models.py in NumPy (the oracle's formulas)"""
    A, e0, al, ec, be, eb, a2 = p[:7]
    x = e / e0
    with np.errstate(all="ignore"):
        if kind == 0:
            return A * x ** -al
        if kind == 1:
            return A * x ** -al * np.exp(-(e / ec) ** be)
        if kind in (2, 3):
            f = np.where(e < eb, A * x ** -al, A * (eb / e0) ** (a2 - al) * x ** -a2)
            return f * np.exp(-(e / ec) ** be) if kind == 3 else f
        return A * x ** (-al - be * np.log(x))


# ---- shapes of the kernel test ------------------------------------------------------------------
KERNEL_N = (1, 3, 65)
KERNEL_NC = (2, 3, 64, 65, 257, 2048)
KERNEL_NF = (0, 1, 3)


def kernel_grid(nC):
    return np.logspace(9.0, np.log10(510.998e12), nC)


def synthetic_loss(nf, e):
    """positive loss tables with a Klein-Nishina-like roll-off, eV/s per erg/cm3"""
    out = np.empty((nf, e.size))
    for f in range(nf):
        ek = 10.0 ** (12.5 + f)
        out[f] = 2.1e-2 * (e / 511e3) ** 2 / (1.0 + e / ek) ** 1.5
    return out


def walker_values(N, nf, seed=0):
    """B [G], age [s], u[nf][N] (erg/cm3): ages from far below to far above the cooling times"""
    rng = np.random.default_rng(seed + 7 * N + nf)
    B = 10.0 ** rng.uniform(-6, -3.5, N)
    age = 10.0 ** rng.uniform(0.0, 7.0, N) * YR
    if N >= 3:
        age[1] = np.inf
        age[2] = 1e-4 * YR
    u = 10.0 ** rng.uniform(-13, -11, (nf, N))
    return B, age, u
