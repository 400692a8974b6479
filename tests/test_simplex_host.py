"""Host-side checks of the lock-step simplex searches (naima_amd/optimize.py): the NumPy
restatement the GPU tests compare the kernels with against the sequential oracle, the interval
and clustering arithmetic, and the argument errors that come before any device work."""
import os
import re
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose

from simplex_cases import (FROZEN_OPTS, OPTION_SETS, f3, fb3, frozen42, starts37)
from simplex_np import minimize_lockstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal_to_oracle(res, i, seq, free=None):
    x = res["x"][i] if free is None else res["x"][i][free]
    assert np.array_equal(x, seq["x"]), i
    assert res["fun"][i] == seq["fun"], i
    assert (res["nfev"][i], res["nit"][i], res["status"][i]) == \
        (seq["nfev"], seq["nit"], seq["status"]), i


def test_lockstep_restatement_is_the_sequential_oracle():
    """37 simplexes in lock-step end, each of them, exactly where oracle.minimize_sequential
    ends from the same start: x, fun, nfev, nit and status equal.  No sort meets a tie, so the
    oracle's unstable argsort is not in play; under the three option sets the statuses are
    37 x 0, 37 x 1 and 35 x 0 + 2 x 1: finished and unfinished simplexes share a batch."""
    from oracle.neldermead_np import minimize_sequential
    starts = starts37()
    assert starts.shape == (37, 3) and starts[5, 2] == 0.0
    want = ([37], [0, 37], [35, 2])
    for opts, counts in zip(OPTION_SETS, want):
        res = minimize_lockstep(fb3, starts, **opts)
        assert res["ties"] == 0
        assert np.bincount(res["status"]).tolist() == counts
        for i, x0 in enumerate(starts):
            _equal_to_oracle(res, i, minimize_sequential(f3, x0, **opts))


def test_frozen_coordinates_are_the_reduced_function():
    """x2 frozen at 7 values from 6 starts: every simplex is the oracle on the two-dimensional
    function of the other two coordinates, and the frozen coordinate keeps its value exactly"""
    from oracle.neldermead_np import minimize_sequential
    starts, frozen, values = frozen42()
    res = minimize_lockstep(fb3, starts, frozen, values, **FROZEN_OPTS)
    assert res["ties"] == 0 and np.bincount(res["status"]).tolist() == [42]
    assert np.array_equal(res["x"][:, 2], values[:, 2])
    for i in range(42):
        v = values[i, 2]
        seq = minimize_sequential(lambda y: f3([y[0], y[1], v]), starts[i, :2], **FROZEN_OPTS)
        _equal_to_oracle(res, i, seq, free=[0, 1])


def _profile(grid, lnl, mlx, mlfun):
    from naima_amd import optimize as O
    grid = np.asarray(grid, dtype=float)
    return O.ProfileResult(0, "a", grid, np.asarray(lnl, dtype=float), None, None,
                           O._Point(np.array([mlx]), mlfun))


def test_interval_on_an_exact_parabola():
    """lnl = top - (x - c)^2 / (2 s^2) on an uneven grid whose points miss the vertex: the
    crossings are c -+ z s, z = Phi^-1((1 + cl) / 2), to rounding"""
    from statistics import NormalDist
    c, s, top = 5.3, 0.7, 41.0
    grid = np.sort(np.concatenate([np.linspace(2.0, 8.5, 14), [5.05, 6.9]]))
    pr = _profile(grid, top - 0.5 * ((grid - c) / s) ** 2, 5.05, top - 0.5 * ((5.05 - c) / s) ** 2)
    assert_allclose(pr.lnl_max, top, rtol=1e-13)
    for cl in (0.683, 0.954, 0.5):
        z = NormalDist().inv_cdf(0.5 * (1 + cl))
        lo, hi = pr.interval(cl)
        assert_allclose([lo, hi], [c - z * s, c + z * s], rtol=1e-12)
    assert_allclose(pr.delta_chi2, ((grid - c) / s) ** 2, rtol=1e-10, atol=1e-11)
    with pytest.raises(ValueError, match="cl must lie"):
        pr.interval(1.0)


def test_interval_on_a_grid_that_does_not_bracket():
    """a side without a grid value below the level is nan, with a warning that names it"""
    grid = np.linspace(5.0, 8.0, 13)
    pr = _profile(grid, 10.0 - 0.5 * ((grid - 5.3) / 0.7) ** 2, 5.25, 10.0)
    with pytest.warns(UserWarning, match="does not bracket the lower"):
        lo, hi = pr.interval(0.683)
    assert np.isnan(lo)
    assert_allclose(hi, 5.3 + 0.7 * 1.0006418287624492, rtol=1e-9)
    pr = _profile(grid[:5], 10.0 - 0.5 * ((grid[:5] - 5.3) / 0.7) ** 2, 5.25, 10.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lo, hi = pr.interval(0.954)
    assert np.isnan(lo) and np.isnan(hi) and len(w) == 2
    # a value the prior forbids (-inf) ends the interval at the last allowed grid point
    lnl = 10.0 - 0.5 * ((grid - 5.3) / 0.1) ** 2
    lnl[2:] = -np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert _profile(grid, lnl, 5.25, 10.0).interval(0.683)[1] == grid[1]


def test_modes_clustering():
    from naima_amd.optimize import cluster_modes
    x = np.array([[1.0, -2.0], [1.0004, -2.0], [3.0, 4.0], [1.0, -2.0019], [0.0, 1.0], [9.0, 9.0]])
    fun = np.array([5.0, 4.0, 6.0, 4.5, np.nan, -np.inf])
    modes = cluster_modes(x, fun, rtol=1e-3)
    assert [m["count"] for m in modes] == [1, 3]
    assert modes[0]["fun"] == 6.0 and np.array_equal(modes[0]["x"], [3.0, 4.0])
    assert modes[1]["fun"] == 5.0 and modes[1]["members"] == [0, 3, 1]
    assert [m["count"] for m in cluster_modes(x, fun, rtol=1e-4)] == [1, 1, 1, 1]
    # a coordinate that is exactly zero in the representative matches only zero
    z = cluster_modes([[0.0, 1.0], [0.0, 1.0], [1e-300, 1.0]], [3.0, 2.0, 1.0])
    assert [m["count"] for m in z] == [2, 1]
    with pytest.raises(ValueError, match="x must be"):
        cluster_modes(np.zeros((3, 2)), np.zeros(2))


def test_argument_errors_come_before_device_work():
    """every check below raises before a context exists (no library is loaded either)"""
    from naima_amd import _lib
    from naima_amd import optimize as O
    loaded = _lib._lib

    def fn(p):
        raise AssertionError("evaluated")

    with pytest.raises(ValueError, match="more than the 64"):
        O.minimize_many(fn, np.ones((2, 65)))
    with pytest.raises(ValueError, match="every coordinate frozen"):
        O.minimize_many(fn, np.ones((2, 3)), frozen=[[0, 0, 1], [1, 1, 1]])
    with pytest.raises(ValueError, match="frozen must be"):
        O.minimize_many(fn, np.ones((2, 3)), frozen=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="values without frozen"):
        O.minimize_many(fn, np.ones((2, 3)), values=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="finite"):
        O.minimize_many(fn, [[1.0, np.nan]])
    with pytest.raises(ValueError, match="batch must be"):
        O.minimize_many(fn, np.ones((2, 3)), batch=3)
    with pytest.raises(ValueError, match="starts must be"):
        O.minimize_many(fn, np.ones((2, 3, 1)))
    with pytest.raises(ValueError, match="needs starts"):
        O.fit_ml(None, None)
    with pytest.raises(ValueError, match="needs ml"):
        O.profile_likelihood(None, None, 0)
    with pytest.raises(ValueError, match="starts_per_point"):
        O.profile_likelihood(None, None, 0, ml=np.ones(3), starts_per_point=0)
    assert _lib._lib is loaded and (loaded is not None or not _lib._default)
    assert O._par_indices("b", 3, ["a", "b", "c"]) == ([1], False)
    assert O._par_indices([-1, "a"], 3, ["a", "b", "c"]) == ([2, 0], True)
    with pytest.raises(ValueError, match="labelled"):
        O._par_indices("z", 3, ["a", "b", "c"])
    with pytest.raises(ValueError, match="outside"):
        O._par_indices(3, 3, None)
    from naima_amd.sampler import EnsembleSampler
    assert hasattr(EnsembleSampler, "fit_ml") and hasattr(EnsembleSampler, "profile_likelihood")


def test_entry_points_are_declared_bound_and_built():
    import ctypes as C

    from naima_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "naima_hip.h")).read()
    names = ["nh_simplex_init_points", "nh_simplex_adopt", "nh_simplex_propose",
             "nh_simplex_update", "nh_simplex_counts", "nh_simplex_shrink_points",
             "nh_simplex_shrink_adopt", "nh_simplex_result"]
    lib = C.CDLL(_lib.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names + ["nh_simplex_bytes"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert name in integration, name
    for name in names:
        assert name in _lib._SIGS
    assert int(re.search(r"#define\s+NH_SIMPLEX_MAX_DIM\s+(\d+)", hdr).group(1)) \
        == _lib.NH_SIMPLEX_MAX_DIM == 64
    src = open(os.path.join(ROOT, "naima_amd", "csrc", "nh_simplex.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "#pragma clang fp contract(off)" in code and "atomic" not in code.lower()
    assert "nh_simplex.hip" in open(os.path.join(ROOT, "naima_amd", "csrc", "build.sh")).read()
    # host arithmetic only: the size of the state
    lib.nh_simplex_bytes.restype = C.c_longlong
    lib.nh_simplex_bytes.argtypes = [C.c_int] * 3
    S, D, n = 37, 3, 3
    ints = (n + 1) * S + D * S + 8 * S + 2
    assert lib.nh_simplex_bytes(S, D, n) == 8 * ((n + 1) * D * S + (n + 1) * S) + \
        4 * ((ints + 1) // 2 * 2)
    assert lib.nh_simplex_bytes(S, 65, 3) == 0 and lib.nh_simplex_bytes(S, 3, 4) == 0
    assert lib.nh_simplex_bytes(0, 3, 3) == 0 and lib.nh_simplex_bytes(2 ** 22, 64, 64) == 0


KERNELS = ("k_sx_init", "k_sx_adopt", "k_sx_propose", "k_sx_update", "k_sx_scan",
           "k_sx_shrink_points", "k_sx_shrink_adopt", "k_sx_result")


def test_simplex_kernels_hold_no_private_memory(tmp_path):
    """the metadata notes of the built library's code object: the order of a simplex is a
    permutation in HBM, so no kernel has a private segment or a spilled VGPR"""
    import subprocess

    from naima_amd import _lib
    from test_infocrit_host import device_code_objects
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(_lib.LIB_PATH), "build the library first"
    found = {}
    for i, co in enumerate(device_code_objects(_lib.LIB_PATH)):
        if b"k_sx_propose" not in co:
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
