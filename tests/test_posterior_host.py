"""The host side of naima_amd.posterior: the ABI of the three reductions, the contour rule, the
edges and the argument errors that come before any device work (no GPU needed)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("nh_column_moments", "nh_hist_columns", "nh_kde_columns")


def _header():
    return open(os.path.join(ROOT, "include", "naima_hip.h")).read()


def test_header_ctypes_mirror_and_exports_hold_the_entry_points():
    import ctypes as C

    from naima_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args[:5] == ["nh_ctx* ctx", "const double* x", "long long M", "int ncol",
                            "long long ld"]
        sig = _lib._SIGS[name]
        assert len(sig) == len(args)
        for a, t in zip(args, sig):
            if a.startswith("int "):
                assert t is C.c_int, (name, a)
            elif a.startswith("long long "):
                assert t is C.c_longlong, (name, a)
            elif a == "const int* pairs":
                assert t is C.POINTER(C.c_int)
            else:
                assert "*" in a and t is C.c_void_p, (name, a)
        assert name in _lib.EXPORTS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)


def test_caps_are_published_and_mirrored():
    from naima_amd import _lib
    caps = dict(re.findall(r"#define\s+(NH_HIST_MAX_\w+)\s+(\d+)", _header()))
    assert set(caps) == {"NH_HIST_MAX_COLS", "NH_HIST_MAX_PAIRS", "NH_HIST_MAX_BINS_1D",
                         "NH_HIST_MAX_BINS_2D"}
    for k, v in caps.items():
        assert getattr(_lib, k) == int(v), k
    assert _lib.NH_HIST_MAX_BINS_2D >= 100
    # every i < j of the widest matrix is one call
    n = _lib.NH_HIST_MAX_COLS
    assert _lib.NH_HIST_MAX_PAIRS == n * (n - 1) // 2


def test_importing_needs_no_device_and_no_matplotlib():
    import subprocess
    code = ("import sys; import naima_amd.posterior as P; from naima_amd import _lib; "
            "assert _lib._lib is None and not _lib._default; "
            "assert 'matplotlib' not in sys.modules; print(sorted(P.__all__))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode()
    assert "histogram_pairs" in out


def test_contour_thresholds_of_a_hand_worked_example():
    from naima_amd.posterior import DEFAULT_LEVELS, contour_thresholds
    H = np.array([[0, 1, 2], [3, 10, 4], [1, 2, 1]])
    # descending 10 4 3 2 2 1 1 1 0; cumulative /24: .4167 .5833 .7083 .7917 .875 .9167 .9583 1 1
    np.testing.assert_array_equal(contour_thresholds(H, [0.5]), [10])
    np.testing.assert_array_equal(contour_thresholds(H, [0.6, 0.8, 0.9]), [4, 2, 2])
    np.testing.assert_array_equal(contour_thresholds(H, [0.3]), [10])  # (not even the largest)
    np.testing.assert_array_equal(contour_thresholds(H, [1.0, 0.96]), [0, 1])  # (levels' order)
    np.testing.assert_array_equal(contour_thresholds(H, [10 / 24.0 + 1e-12]), [10])
    np.testing.assert_allclose(DEFAULT_LEVELS,
                               [1 - np.exp(-0.5 * s * s) for s in (0.5, 1.0, 1.5, 2.0)], rtol=1e-15)
    np.testing.assert_array_equal(contour_thresholds(H), contour_thresholds(H, DEFAULT_LEVELS))
    with pytest.raises(ValueError):
        contour_thresholds(np.zeros((3, 3)))


def test_edges_are_numpy_s():
    from naima_amd.posterior import _edges, _range
    rng = np.random.default_rng(2)
    x = np.stack([rng.normal(size=100), 7 + 1e-3 * rng.normal(size=100),
                  -200 + 50 * rng.normal(size=100)], 1)
    for nb in (1, 2, 20, 37, 100):
        e = _edges(x.min(0), x.max(0), nb)
        assert e.shape == (3, nb + 1)
        for c in range(3):
            want = np.histogram(x[:, c], bins=nb, range=(x[:, c].min(), x[:, c].max()))[1]
            np.testing.assert_array_equal(e[c], want)
    # lo == hi widens by a half on each side, as np.histogram does
    e = _edges([3.0, 0.0], [3.0, 1.0], 4)
    np.testing.assert_array_equal(e[0], np.histogram(np.full(5, 3.0), bins=4)[1])
    np.testing.assert_array_equal(e[0], np.linspace(2.5, 3.5, 5))
    np.testing.assert_array_equal(e[1], np.linspace(0.0, 1.0, 5))
    lo, hi = _range((-1.0, 2.0), 3)
    np.testing.assert_array_equal(lo, [-1.0] * 3)
    np.testing.assert_array_equal(hi, [2.0] * 3)
    lo, hi = _range([(0, 1), (2, 3), (4, 5)], 3)
    np.testing.assert_array_equal(hi, [1.0, 3.0, 5.0])
    for bad in ((1.0, 0.0), (0.0, np.inf), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            _edges(*_range(bad, 2), 10)
    with pytest.raises(ValueError):
        _range([(0, 1), (2, 3)], 3)


def test_bandwidths_are_scipy_s():
    from naima_amd.posterior import _bandwidths
    n, var = np.array([4099, 50]), np.array([2.0, 1e-6])
    np.testing.assert_allclose(_bandwidths(None, n, var), n ** -0.2 * np.sqrt(var), rtol=1e-15)
    np.testing.assert_array_equal(_bandwidths("scott", n, var), _bandwidths(None, n, var))
    np.testing.assert_allclose(_bandwidths("silverman", n, var),
                               (0.75 * n) ** -0.2 * np.sqrt(var), rtol=1e-15)
    np.testing.assert_allclose(_bandwidths(0.3, n, var), 0.3 * np.sqrt(var), rtol=1e-15)
    scipy_stats = pytest.importorskip("scipy.stats")
    x = np.random.default_rng(0).normal(size=50)
    for bw in (None, "silverman", 0.3):
        k = scipy_stats.gaussian_kde(x, bw_method=bw)
        np.testing.assert_allclose(_bandwidths(bw, [50], [np.var(x, ddof=1)])[0],
                                   np.sqrt(k.covariance[0, 0]), rtol=1e-14)


def test_argument_errors_come_before_any_device_work():
    from naima_amd import _lib
    from naima_amd import posterior as P
    x = np.random.default_rng(1).normal(size=(50, 3))
    contexts = dict(_lib._default)
    with pytest.raises(ValueError, match="at least 1"):
        P.histogram(x, bins=0)
    with pytest.raises(ValueError, match="at least 1"):
        P.histogram_pairs(x, bins=-3)
    with pytest.raises(ValueError, match="more than"):
        P.histogram(x, bins=_lib.NH_HIST_MAX_BINS_1D + 1)
    with pytest.raises(ValueError, match="more than"):
        P.histogram_pairs(x, bins=_lib.NH_HIST_MAX_BINS_2D + 1)
    with pytest.raises(ValueError, match="integer"):
        P.histogram(x, bins=[0.0, 1.0])
    with pytest.raises(ValueError, match="outside"):
        P.histogram_pairs(x, pairs=[(0, 3)])
    with pytest.raises(ValueError, match="outside"):
        P.histogram_pairs(x, pairs=[(-1, 1)])
    with pytest.raises(ValueError, match="range"):
        P.histogram(x, range=[(0, 1), (0, 1)])
    with pytest.raises(ValueError, match="bw_method"):
        P.gaussian_kde(x, [0.0], bw_method="wide")
    with pytest.raises(ValueError, match="positive variance"):
        P._bandwidths(None, [50, 50], [1.0, 0.0])  # (what a zero-variance column's KDE raises)
    with pytest.raises(ValueError, match="more than"):
        P.corner(x, bins=_lib.NH_HIST_MAX_BINS_2D + 1)
    assert _lib._default == contexts  # no context was made
