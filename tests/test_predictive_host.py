"""The host side of naima_amd.predictive (no GPU needed): the NumPy restatement of the kernels'
algorithms (tests/predictive_np.py) against Random123's known answers and against the moments of
the distribution it draws from, the example that motivates the runs statistic, the argument errors
that come before any device work, and the declarations of the entry points."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import predictive_np as R  # noqa: E402

NAMES = ("nh_ppc_rows", "nh_ppc_counts", "nh_pit_columns")
KERNELS = ("k_ppc_rows", "k_ppc_counts", "k_pit_sum", "k_pit_fin")
M, NE, SEED = 4000, 24, 12345


def power_law():
    """the 24-point E^-2 table of the prototype: elo = 0.10 flux, ehi = 0.25 flux, no limits"""
    flux = 1e-12 * np.logspace(0.0, -4.0, NE)
    return dict(flux=flux, elo=0.10 * flux, ehi=0.25 * flux, ul=np.zeros(NE, bool))


def bump():
    """(spectra [M][NE], observed [NE]): 4000 posterior spectra scattered 2 % around the power
    law, and observed points with a smooth bump the model cannot make, inside the error bars"""
    t = power_law()
    g = np.random.default_rng(1).standard_normal((M, 1))
    k = np.arange(NE)
    return t["flux"] * (1.0 + 0.02 * g), t["flux"] * (1.0 + 0.3 * np.sin(np.pi * k / 23) - 0.19)


# ---------------------------------------------------------------------------------------
# 1. the random stream and the draw
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(v) for v in R.philox4x32(ctr, key)) == want


def test_the_draw_has_the_split_normals_moments():
    t = power_law()
    x = np.tile(t["flux"], (M, 1))
    Y, T, below = R.ppc_rows(x, 1.0, t["flux"], t["elo"], t["ehi"], t["ul"], seed=SEED)
    n = M * NE
    p = 0.25 / 0.35
    frac = below.mean()
    chi2 = T[:, 1].mean()
    pit = R.split_normal_cdf(Y, x, t["elo"], t["ehi"]).mean()
    print("below %.5f (%.5f)  mean chi2_rep %.3f  mean PIT %.5f" % (frac, p, chi2, pit))
    assert abs(frac - p) < 6.0 * math.sqrt(p * (1.0 - p) / n)
    assert abs(chi2 - NE) < 6.0 * math.sqrt(2.0 * NE / M)
    assert abs(pit - 0.5) < 6.0 / math.sqrt(12.0 * n)
    # the replicate lies on the side its bit says, by a * the scale of that side
    a, b2 = R.draw(M, NE, t["elo"], t["ehi"], seed=SEED)
    assert np.array_equal(b2, below) and np.array_equal(Y < x, below) and np.all(a > 0)
    assert a.max() <= 8.6
    # a value depends on (seed, row, k) alone
    Y2, T2, _ = R.ppc_rows(x[:100], 1.0, t["flux"], t["elo"], t["ehi"], t["ul"], seed=SEED, row0=50)
    assert np.array_equal(Y2[:50], Y[50:100]) and np.array_equal(T2[:50], T[50:100])


def test_runs_sees_the_bump_that_chi2_does_not():
    t = power_law()
    spectra, observed = bump()
    _, T, _ = R.ppc_rows(spectra, 1.0, observed, t["elo"], t["ehi"], t["ul"], seed=SEED)
    p_chi2, p_max, p_runs, n_bad = R.p_values(T)
    print("p_chi2 %.4f  p_max %.4f  p_runs %.4f  mean chi2_obs %.2f" % (p_chi2, p_max, p_runs,
                                                                        T[:, 0].mean()))
    assert n_bad == 0
    assert p_chi2 > 0.5 and p_runs < 0.05
    # chi2_obs is -2 x the likelihood's sum
    d = spectra - observed
    sg = np.where(d > 0, t["ehi"], t["elo"])
    np.testing.assert_allclose(T[:, 0], (d * d / (sg * sg)).sum(axis=1), rtol=1e-12)


def test_counts_leave_out_rows_that_are_not_finite():
    T = np.array([[1.0, 2.0, 1.0, 0.5, 3.0, 3.0],      # chi2 yes, max no, runs yes (a tie)
                  [2.0, 2.0, 1.0, 1.0, 2.0, 5.0],      # ties: yes, yes; runs no
                  [np.nan, 9.0, 0.0, 9.0, 9.0, 0.0],   # bad
                  [1.0, 2.0, 1.0, np.inf, 3.0, 3.0]])  # bad
    assert R.ppc_counts(T).tolist() == [2, 1, 1, 2]
    assert R.p_values(T) == (1.0, 0.5, 0.5, 2)
    assert R.runs(np.array([[True, True, False, True], [False] * 4])).tolist() == [3.0, 1.0]
    ul = np.ones(3, bool)
    Y, T, _ = R.ppc_rows(np.ones((2, 3)), 2.0, np.ones(3), np.ones(3), np.ones(3), ul)
    assert np.all(T == 0.0) and np.all(Y == 2.0)


def test_pit_of_a_far_point_is_positive():
    # 30 sigma below the model, in the lower tail: 2 ehi / (elo + ehi) Phi(-30)
    f = R.split_normal_cdf(1.0 - 30.0 * 0.25, 1.0, 0.1, 0.25)
    want = 2.0 * 0.25 / 0.35 * 0.5 * math.erfc(30.0 / math.sqrt(2.0))
    assert 0.0 < f < 1e-190 and abs(f / want - 1.0) < 1e-12
    # continuous at the model, 1 far above
    assert R.split_normal_cdf(1.0, 1.0, 0.1, 0.25) == pytest.approx(0.25 / 0.35, rel=1e-15)
    assert R.split_normal_cdf(1.0 + 1e-12, 1.0, 0.1, 0.25) == pytest.approx(0.25 / 0.35, rel=1e-9)
    assert R.split_normal_cdf(9.0, 1.0, 0.1, 0.25) == pytest.approx(1.0, rel=1e-15)
    out = R.pit_columns(np.array([[1.0, 1.0], [3.0, 3.0]]), 1.0, np.array([2.0, 2.0]),
                        np.ones(2), np.ones(2), np.array([False, True]))
    assert out[0][0] == pytest.approx(0.5) and np.isnan(out[0][1])
    assert np.isnan(out[1][0]) and out[1][1] == 0.5


# ---------------------------------------------------------------------------------------
# 2. errors before any device work
# ---------------------------------------------------------------------------------------
def test_errors_come_before_a_context_exists():
    from naima_amd import _lib
    from naima_amd import predictive as P
    from naima_amd import units as u
    before = (_lib._lib, dict(_lib._default))
    unit = "1/(s cm2 TeV)"
    data = {"flux": u.Quantity(np.ones(3), unit), "ul": np.zeros(3, bool)}
    good = u.Quantity(np.ones((5, 3)), unit)
    for fn in (P.posterior_predictive, P.ppc, P.pit):
        with pytest.raises(ValueError, match="energies"):
            fn(u.Quantity(np.ones((5, 4)), unit), data)
        with pytest.raises(ValueError, match="2-D"):
            fn(u.Quantity(np.ones(3), unit), data)
        with pytest.raises(ValueError, match="no samples"):
            fn(u.Quantity(np.ones((0, 3)), unit), data)
        with pytest.raises(ValueError, match="unit"):
            fn(np.ones((5, 3)), data)
        with pytest.raises(ValueError, match="contradicts"):
            fn(good, data, unit="erg/(s cm2)")
    for fn in (P.posterior_predictive, P.ppc):
        for seed in (-1, 2 ** 64, 1.5, "x", None, True):
            with pytest.raises(ValueError, match="seed"):
                fn(good, data, seed=seed)
    for row0 in (-1, 2 ** 63, 0.5):
        with pytest.raises(ValueError, match="row0"):
            P.posterior_predictive(good, data, row0=row0)
    only = {"flux": u.Quantity(np.ones(3), unit), "ul": np.ones(3, bool)}
    with pytest.raises(ValueError, match="every data point is an upper limit"):
        P.ppc(good, only)
    for q in ([], [-0.1], [1.5], [[0.1, 0.2]], [np.nan]):
        with pytest.raises(ValueError, match="quantiles"):
            P.predictive_quantiles(np.ones((5, 3)), q)
    for bad in (np.zeros((2, 3, 4)), np.zeros((0, 3)), 1.0):
        with pytest.raises(ValueError):
            P.predictive_quantiles(bad, [0.5])

    class NoSpectrum(P.PredictiveMixin):
        data = {"energy": u.Quantity(np.ones(3), "TeV")}
        blob_units = [u.Unit("erg"), None, u.Unit(unit)]

        def get_blobs(self, discard=0, thin=1):
            return [np.ones((4, 2)), np.ones((4, 2, 3)), np.ones((4, 2, 5))]

    for idx in (0, 1, 2, 3):  # a scalar, no unit, other energies, not there
        with pytest.raises(TypeError, match="Model %d has wrong blob format" % idx):
            NoSpectrum().ppc(modelidx=idx)
        with pytest.raises(TypeError, match="Model %d has wrong blob format" % idx):
            NoSpectrum().get_posterior_predictive(modelidx=idx)
    with pytest.raises(ValueError, match="seed"):
        NoSpectrum().ppc(seed=-1)
    assert (_lib._lib, dict(_lib._default)) == before


def test_importing_creates_no_context():
    code = ("import sys; import naima_amd; from naima_amd import _lib, predictive; "
            "from naima_amd.sampler import EnsembleSampler; from naima_amd.analysis import _Result; "
            "assert _lib._lib is None and not _lib._default; "
            "assert 'matplotlib' not in sys.modules; "
            "assert naima_amd.predictive is predictive and callable(naima_amd.plot_ppc); "
            "assert all(hasattr(c, m) for c in (EnsembleSampler, _Result) "
            "for m in ('get_posterior_predictive', 'ppc', 'loo')); "
            "print(sorted(predictive.__all__))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode()
    assert "posterior_predictive" in out and "ppc" in out and "predictive_quantiles" in out


def test_header_ctypes_mirror_and_exports_hold_the_entry_points():
    from naima_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "naima_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        sig = _lib._SIGS[name]
        assert len(sig) == len(args), name
        for a, t in zip(args, sig):
            if a.startswith("int "):
                assert t is C.c_int, (name, a)
            elif a.startswith("long long "):
                assert t is C.c_longlong, (name, a)
            elif a.startswith("unsigned long long "):
                assert t is C.c_ulonglong, (name, a)
            else:
                assert "*" in a and t is C.c_void_p, (name, a)
        assert name in _lib.EXPORTS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
        assert name in integration


# ---------------------------------------------------------------------------------------
# 3. the new kernels hold no private memory
# ---------------------------------------------------------------------------------------
def test_new_kernels_hold_no_private_memory(tmp_path):
    """the metadata notes of the built library's code object: no private segment and no spilled
    VGPR in any of the new kernels"""
    from naima_amd import _lib
    from test_infocrit_host import device_code_objects
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(_lib.LIB_PATH), "build the library first"
    found = {}
    for i, co in enumerate(device_code_objects(_lib.LIB_PATH)):
        if b"k_ppc_rows" not in co:
            continue
        f = tmp_path / ("co%d" % i)
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True,
                               check=True).stdout
        for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            hit = [k for k in KERNELS if k + "E" in name]
            if hit:
                found[hit[0]] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                                 int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)))
    assert sorted(found) == sorted(KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
