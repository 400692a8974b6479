"""The shared geometry of the column reductions (csrc/nh_colred.h) through its six entry points --
nh_column_moments, nh_lnl_column_stats, nh_psis_columns, nh_pit_columns, nh_psis_weights and
nh_weighted_moments -- at the shapes where it can go wrong: one column (256 row lanes), three
(an idle column lane), 65 (a second tile of one column); one row, fewer rows than row lanes, three
chunks with a short last one.  Expected values are the NumPy restatements of test_gpu_posterior,
test_gpu_infocrit, test_gpu_predictive and test_gpu_reweight at those files' tolerances; every
case is called twice for equal bytes, and once without the NaN padding of ld = ncol + 2, which
must change no bit either."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import colred_cases as K  # noqa: E402
import infocrit_np as RI  # noqa: E402
import predictive_np as RP  # noqa: E402
import reweight_np as RW  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RTOL, ATOL = 1e-9, 1e-12
shapes = pytest.mark.parametrize("M,ncol", [(M, n) for M in K.MS for n in K.NCOLS])


def outputs(entry, x):
    """the entry point's outputs for x; called again, and without padding: the same bytes"""
    got = K.CALLS[entry](x)
    for other in (K.CALLS[entry](x), K.CALLS[entry](x, 0)):
        assert sorted(other) == sorted(got)
        for k, v in got.items():
            assert other[k].tobytes() == v.tobytes(), (entry, k)
    return got


def check_pareto_k(got, want):
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL)


@shapes
def test_column_moments(M, ncol):
    """n, n_nan, min and max exact; mean within M eps mean(|x|), var within max(1e-12, M eps)"""
    x = K.moments_input(M, ncol)
    got = outputs("column_moments", x)
    (n, n_nan), (lo, hi, mean, var) = got["counts"], got["stats"]
    for c in range(ncol):
        f = x[:, c][np.isfinite(x[:, c])]
        assert n[c] == f.size and n_nan[c] == np.isnan(x[:, c]).sum()
        assert lo[c] == f.min() and hi[c] == f.max()
        assert abs(mean[c] - np.mean(f)) <= M * EPS * np.mean(np.abs(f))
        if f.size > 1:
            np.testing.assert_allclose(var[c], np.var(f, ddof=1), rtol=max(1e-12, M * EPS), atol=0)
        else:
            assert np.isnan(var[c])


@shapes
def test_lnl_column_stats(M, ncol):
    L = K.lnl_input(M, ncol)
    got = outputs("lnl_column_stats", L)["stats"]
    want = RI.column_stats(L)
    for i, k in enumerate(("max", "mean", "var", "lse", "min")):
        np.testing.assert_allclose(got[i], want[k], rtol=RTOL, atol=ATOL, err_msg=k)
    assert np.all(np.isfinite(got[3]))
    if M == 1:
        assert np.all(np.isnan(got[2]))
    elif ncol > 1:
        assert got[2][1] == 0.0 and got[1][1] == -3.25


@shapes
def test_psis_columns(M, ncol):
    L = K.lnl_input(M, ncol)
    got = outputs("psis_columns", L)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = RI.loo(L)
    np.testing.assert_array_equal(got["n_tail"], want["n_tail"])
    check_pareto_k(got["pareto_k"], want["pareto_k"])
    np.testing.assert_allclose(got["elpd"], want["elpd_loo_i"], rtol=RTOL, atol=ATOL)
    if M > 1 and ncol > 1:
        assert got["n_tail"][1] == 0 and np.isposinf(got["pareto_k"][1])  # the constant column


@shapes
def test_pit_columns(M, ncol):
    x, t = K.pit_input(M, ncol)
    got = outputs("pit_columns", (x, t))["out"]
    want = RP.pit_columns(x, t["conv"], t["flux"], t["flux_error_lo"], t["flux_error_hi"], t["ul"])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(np.isnan(got[0]), t["ul"]) and np.array_equal(np.isnan(got[1]), ~t["ul"])


@shapes
def test_psis_weights(M, ncol):
    lr = K.ratio_input(M, ncol)
    got = outputs("psis_weights", lr)
    with np.errstate(all="ignore"):
        want = RW.psis_weights_np(lr, RW.tail_length(M))
    assert np.all(got["lw"][:, ncol] == K.POISON)  # the block's last column is untouched
    np.testing.assert_array_equal(got["status"], want["status"])
    bad = K.bad_ratio_column(M, ncol)  # that column: its offenders counted, NaN in every row
    for c in range(ncol):
        assert got["status"][c] == ((2 if M > 1 else 1) if c == bad else 0)
    if bad is not None:
        assert np.all(np.isnan(got["lw"][:, bad])) and got["n_tail"][bad] == 0
        assert all(np.isnan(got[k][bad]) for k in ("pareto_k", "ess", "lmean"))
    np.testing.assert_array_equal(got["n_tail"], want["n_tail"])
    check_pareto_k(got["pareto_k"], want["pareto_k"])
    np.testing.assert_allclose(got["lw"][:, :ncol], want["lw"], rtol=RTOL, atol=ATOL)
    for k in ("ess", "lmean"):
        np.testing.assert_allclose(got[k], want[k], rtol=RTOL, atol=ATOL, err_msg=k)


@shapes
def test_weighted_moments(M, ncol):
    x, lw = K.weighted_input(M, ncol)
    got = outputs("weighted_moments", (x, lw))["out"]
    n, mean, var = RW.weighted_moments_np(x, lw)
    np.testing.assert_array_equal(got[0], n.astype(float))
    np.testing.assert_allclose(got[1], mean, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got[2], var, rtol=RTOL, atol=ATOL)
    if ncol > 2:
        assert got[1][2] == 1.25 and got[2][2] == 0.0  # exactly
