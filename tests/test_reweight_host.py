"""The host side of naima_amd.reweight (no GPU needed): the entry points in the header, the ctypes
mirror and the built library; no context on import; the argument errors that come before any
device work; and self-checks of the NumPy restatement the GPU tests compare with
(tests/reweight_np.py)."""
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

import reweight_np as R  # noqa: E402
from naima_amd import reweight as RW  # noqa: E402  (every test here is of that module)

NAMES = ("nh_row_sums_select", "nh_psis_weights", "nh_weighted_moments", "nh_weighted_select",
         "nh_resample_systematic", "nh_gather_rows")


def test_header_ctypes_mirror_and_exports_hold_the_entry_points():
    import ctypes as C

    from naima_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "naima_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    build = open(os.path.join(ROOT, "naima_amd", "csrc", "build.sh")).read()
    assert "nh_reweight.hip" in build
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
            elif a.startswith("double "):
                assert t is C.c_double, (name, a)
            else:  # a pointer: a device address, or a host array of the pointed-to type
                assert "*" in a, (name, a)
                host = {"const int* cols": C.POINTER(C.c_int), "const double* q": C.POINTER(C.c_double)}
                assert t is host.get(a, C.c_void_p) or t == host.get(a, C.c_void_p), (name, a)
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_importing_creates_no_context():
    code = ("import sys; import naima_amd; from naima_amd import _lib, reweight; "
            "from naima_amd.sampler import EnsembleSampler; from naima_amd.analysis import _Result; "
            "assert _lib._lib is None and not _lib._default; "
            "assert 'matplotlib' not in sys.modules; "
            "assert all(hasattr(c, m) for c in (EnsembleSampler, _Result) "
            "for m in ('reweight', 'influence')); "
            "print(sorted(reweight.__all__))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode()
    for name in ("psis_weights", "weighted_stats", "weighted_quantiles", "resample",
                 "resample_index", "drop_points", "add_points", "summary", "Weights", "Reweighted"):
        assert "'%s'" % name in out, name


class FakeMatrix:
    ncol, ld, ptr = 2, 2, 0


def fake_weights(M=10, K=2):
    from naima_amd.reweight import Weights
    return Weights(FakeMatrix(), np.zeros(K), np.zeros(K, np.int64), np.full(K, 4.4), np.zeros(K),
                   2, M)


def test_errors_come_before_a_context_exists():
    from naima_amd import _lib
    from naima_amd import units as u
    before = (_lib._lib, dict(_lib._default))
    # psis_weights
    for bad in (np.zeros((2, 3, 4)), np.zeros((0, 3)), 1.0):
        with pytest.raises(ValueError):
            RW.psis_weights(bad)
    for reff in (0.0, -1.0, np.nan, np.inf, "x", None):
        with pytest.raises(ValueError, match="reff"):
            RW.psis_weights(np.zeros(10), reff=reff)
    with pytest.raises(ValueError, match="thin"):
        RW.psis_weights(np.zeros((1864136, 1)))
    # the reductions
    w = fake_weights()
    x = np.zeros((10, 3))
    for fn in (RW.weighted_stats, RW.resample, RW.summary):
        with pytest.raises(ValueError, match="rows"):
            fn(np.zeros((9, 3)), w)
        with pytest.raises(ValueError, match="targets"):
            fn(x, w, k=2)
        with pytest.raises(ValueError, match="psis_weights"):
            fn(x, np.zeros(10))
    with pytest.raises(ValueError, match="targets"):
        RW.weighted_quantiles(x, w, [0.5], k=-1)
    with pytest.raises(ValueError, match="rows"):
        RW.weighted_quantiles(np.zeros(7), w, [0.5])
    for q in ([], [-0.1], [1.1], [np.nan], "x", [[0.1]]):
        with pytest.raises(ValueError, match="q must"):
            RW.weighted_quantiles(x, w, q)
    for n in (0, -3, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="n must"):
            RW.resample(x, w, n=n)
        with pytest.raises(ValueError, match="n must"):
            RW.resample_index(w, n=n)
    with pytest.raises(ValueError, match="labels"):
        RW.summary(x, w, labels=["a"])
    # the log-ratios of points
    L = np.zeros((10, 4))
    for fn in (RW.drop_points, RW.add_points):
        with pytest.raises(ValueError, match="not one of the 4"):
            fn(L, [[0, 4]])
        with pytest.raises(ValueError, match="not one of the 4"):
            fn(L, [[-1]])
        with pytest.raises(ValueError, match="no group"):
            fn(L, [])
        with pytest.raises(ValueError, match="2-D"):
            fn(np.zeros(10), [[0]])
        with pytest.raises(ValueError, match="groups must"):
            fn(L, [["a"]])

    # the sampler's surface
    class Run(RW.ReweightMixin):
        data = {"energy": u.Quantity(np.ones(3), "TeV"), "group": np.array([0, 0, 0])}
        blob_units = [u.Unit("1/(s cm2 TeV)")]
        modelfn = None

        def get_chain(self, flat=False, discard=0, thin=1):
            return np.zeros((8, 2))

        def get_blobs(self, discard=0, thin=1):
            return [np.ones((4, 2, 3))]

    r = Run()
    for kw in ({}, dict(drop=[0], log_ratio=np.zeros(8)), dict(drop=[0], new_data={}),
               dict(drop=[0], new_data={}, log_ratio=np.zeros(8))):
        with pytest.raises(ValueError, match="exactly one"):
            r.reweight(**kw)
    with pytest.raises(ValueError, match="not one of the 3"):
        r.reweight(drop=[3])
    with pytest.raises(ValueError, match="no group"):
        r.reweight(drop={"group": 7})
    with pytest.raises(ValueError, match="group"):
        r.reweight(drop={"groups": 0})
    with pytest.raises(ValueError, match="reff"):
        r.reweight(drop=[0], reff=0.0)
    with pytest.raises(ValueError, match="modelfn"):
        r.reweight(new_data={"energy": u.Quantity(np.ones(1), "TeV")})
    with pytest.raises(ValueError, match="8 rows"):
        r.reweight(log_ratio=np.zeros(7))
    with pytest.raises(ValueError, match="8 rows"):
        r.reweight(log_ratio=np.zeros((8, 2)))
    with pytest.raises(ValueError, match="one group"):
        r.influence()
    assert (_lib._lib, dict(_lib._default)) == before


def test_restatement_uniform_weights_and_no_points():
    # equal ratios: uniform weights, nothing above the cutoff, k = +inf, ESS = M, mean ratio = it
    for M in (6, 100, 1000):
        r = R.psis_weights_np(np.full(M, -3.5), R.tail_length(M))
        np.testing.assert_allclose(r["lw"][:, 0], -np.log(M), rtol=1e-14)
        assert np.isposinf(r["pareto_k"][0]) and r["n_tail"][0] == 0 and r["status"][0] == 0
        np.testing.assert_allclose(r["ess"][0], M, rtol=1e-12)
        np.testing.assert_allclose(r["lmean"][0], -3.5, rtol=1e-14)
    # leaving no point out is a log-ratio of zeros
    L = np.random.default_rng(0).normal(size=(20, 5))
    assert np.all(R.row_sums(L, [[]], -1) == 0.0)
    np.testing.assert_array_equal(R.row_sums(L, [[1, 3], [2]], -1),
                                  np.column_stack([-(L[:, 1] + L[:, 3]), -L[:, 2]]))
    np.testing.assert_array_equal(R.row_sums(L, [[1, 3]], +1)[:, 0], L[:, 1] + L[:, 3])


def test_restatement_weights_are_normalised_and_bad_columns_have_none():
    rng = np.random.default_rng(1)
    lr = rng.normal(0.0, 1.5, size=(2000, 3))
    lr[::3, 1] = -np.inf
    r = R.psis_weights_np(lr, R.tail_length(2000))
    np.testing.assert_allclose(np.exp(r["lw"]).sum(axis=0), 1.0, rtol=1e-12)
    assert np.all(np.isneginf(r["lw"][::3, 1])) and np.all(r["n_tail"] == R.tail_length(2000))
    assert np.all(np.isfinite(r["pareto_k"])) and np.all(r["ess"] < 2000)
    # Mt = 0: plain self-normalised weights
    p = R.psis_weights_np(lr, 0)
    np.testing.assert_allclose(p["lw"], lr - R.logsumexp(lr, axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p["lmean"], R.logsumexp(lr, axis=0) - np.log(2000), rtol=1e-14)
    for v, count in ((np.nan, 2), (np.inf, 2)):
        b = lr.copy()
        b[[5, 9], 0] = v
        r = R.psis_weights_np(b, 95)
        assert np.all(np.isnan(r["lw"][:, 0])) and r["status"].tolist() == [count, 0, 0]
        assert np.isnan(r["pareto_k"][0]) and np.isnan(r["ess"][0]) and r["n_tail"][0] == 0
    r = R.psis_weights_np(np.full(50, -np.inf), 10)
    assert r["status"][0] == 50 and np.all(np.isnan(r["lw"]))


def test_restatement_weighted_reductions():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(400, 3))
    lw = np.log(rng.random(400))
    lw -= R.logsumexp(lw)
    lw[::7] = -np.inf
    x[::7] = np.nan  # zero-weight rows may hold anything
    n, mean, var = R.weighted_moments_np(x, lw)
    live = ~np.isneginf(lw)
    np.testing.assert_allclose(mean, np.average(x[live], axis=0, weights=np.exp(lw[live])), rtol=1e-12)
    assert np.all(n == live.sum()) and np.all(var > 0)
    # uniform weights: the order statistic of rank ceil(q M) - 1
    u = np.full(64, -np.log(64.0))
    v = rng.normal(size=64)
    got, margin = R.weighted_quantile_np(v, u, [0.0, 0.25, 0.5, 1.0])
    np.testing.assert_array_equal(got, np.sort(v)[[0, 15, 31, 63]])
    assert margin == 0.0  # (exact running sums sit ON q C: a power of two is the exact case)
    # systematic resampling: floor or ceil of n w draws of every row, ascending
    idx, _ = R.systematic_np(lw, 0.37, 1000)
    cnt = np.bincount(idx, minlength=400)
    nw = 1000 * np.exp(lw) / np.exp(lw).sum()
    assert np.all(np.diff(idx) >= 0) and np.all(cnt[~live] == 0)
    assert np.all((cnt >= np.floor(nw)) & (cnt <= np.ceil(nw)))


KERNELS = ("k_rw_row_sums", "k_rw_max", "k_rw_max_fin", "k_rw_split", "k_rw_tail", "k_rw_write",
           "k_rw_ess", "k_rw_wsum", "k_rw_wmean", "k_rw_wsq", "k_rw_wvar", "k_rw_tile_sums",
           "k_rw_tile_scan", "k_rw_pick", "k_rw_keys", "k_rw_cumsum", "k_rw_draw", "k_rw_gather")


def test_new_kernels_hold_no_private_memory(tmp_path):
    """the metadata notes of the built library's code object: no private segment and no spilled
    VGPR in any of the new kernels, and the tail workgroup's LDS within a CU's 160 KiB"""
    from test_infocrit_host import device_code_objects

    from naima_amd import _lib
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(_lib.LIB_PATH), "build the library first"
    found, lds = {}, {}
    for i, co in enumerate(device_code_objects(_lib.LIB_PATH)):
        if b"k_rw_tail" not in co:
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
                lds[hit[0]] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1))
    assert sorted(found) == sorted(KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
    assert max(lds.values()) == lds["k_rw_tail"] <= 160 * 1024, lds
