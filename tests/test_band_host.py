"""Band-integrated flux and luminosity per walker (``utils.trapz_loglog`` of a device spectrum):
what can be checked without a GPU -- the new entry points' declarations against their ctypes
mirrors, and that a device matrix is never integrated on the host."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nh_trapz_loglog_comps", "nh_trapz_loglog_comps_intervals")


def _declared_args(name):
    hdr = open(os.path.join(ROOT, "include", "naima_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_header_and_ctypes_mirror_agree(name):
    import ctypes as C

    from naima_amd import _lib
    want = ["nh_ctx* ctx", "const nh_comp* comps", "int ncomp", "const double* colfac",
            "const nh_lazy* rowfac", "const double* x", "int N", "int n", "double* out", "int ldo"]
    assert _declared_args(name) == want
    # the mirror: a pointer where the header has one, an int where it has an int
    sig = _lib._SIGS[name]
    assert sig == [C.c_int if a.startswith("int ") else C.c_void_p for a in want]
    assert name in _lib.EXPORTS
    # the same description nh_lincomb takes, with the abscissa between the row factor and N
    lin = _declared_args("nh_lincomb")
    assert want[:5] == lin[:5] and want[6] == lin[5] and want[8:] == lin[7:]


def test_library_exports_the_entry_points():
    import ctypes as C

    from naima_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_axis_and_length_are_checked_before_anything_runs():
    from naima_amd import units as u
    from naima_amd.darray import DMat
    from naima_amd.utils import trapz_loglog
    m = DMat(None, [(None, 0, 7, 1.0)], (3, 7))
    x = np.geomspace(1.0, 10.0, 7)
    for axis in (0, -2, 2):
        with pytest.raises(ValueError, match="axis"):
            trapz_loglog(m, x, axis=axis)
        with pytest.raises(ValueError, match="axis"):
            trapz_loglog(u.Quantity(m, "1/(s eV)"), x * u.eV, axis=axis)
    with pytest.raises(ValueError, match="different lengths"):
        trapz_loglog(m, x[:-1])
    with pytest.raises(ValueError, match="one-dimensional"):
        trapz_loglog(m, x[None, :])


def test_no_cpu_fallback_for_a_device_matrix():
    """without a GPU the integral of a device matrix raises: it is never downloaded (there is
    nothing to download here) and never computed with NumPy"""
    from naima_amd import _lib
    from naima_amd.darray import DMat
    from naima_amd.utils import trapz_loglog
    try:
        _lib.get_context()
    except _lib.NaimaHipError:
        pass
    else:
        pytest.skip("a GPU is present")
    m = DMat(None, [(None, 0, 7, 1.0)], (3, 7))
    x = np.geomspace(1.0, 10.0, 7)
    for kw in ({}, dict(intervals=True), dict(axis=1)):
        with pytest.raises(_lib.NaimaHipError):
            trapz_loglog(m, x, **kw)
