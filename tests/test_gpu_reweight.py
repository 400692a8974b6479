"""naima_amd.reweight on the GPU against its NumPy restatement (tests/reweight_np.py):
nh_psis_weights, nh_weighted_select, nh_weighted_moments, nh_resample_systematic, nh_gather_rows
and nh_row_sums_select at the shapes where their kernels take another path, then a whole fit
(cfg3, 64 walkers x 30 steps on the device loop) through sampler.reweight / influence, save_run /
read_run and the posterior reductions.

RTOL, ATOL are the values tests/test_gpu_infocrit.py holds nh_psis_columns to against the same
generalised-Pareto restatement.  The weighted order statistics and the resampled rows are compared
EXACTLY, under a condition asserted on the NumPy side first: no running sum of the reference lies
within 1e-9 C of a threshold (reweight_np.weighted_quantile_np names the two pairs that cannot)."""
import ctypes as C
import math
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reweight_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
RT_MODEL = 1e-9  # the spectrum tolerance of the loop tests (test_gpu_shapes.py)
MARGIN = 1e-9
POISON = -7.25e33
Q = [0.0, 1e-6, 0.16, 0.5, 0.84, 1.0]


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


# ---------------------------------------------------------------------------------------
# 1. nh_psis_weights
# ---------------------------------------------------------------------------------------
def psis_gpu(lr, Mt, ld=None, ldw=None):
    """nh_psis_weights of host lr [M][K] in a matrix of row stride ld, lw of stride ldw, both
    poisoned behind the K columns: (dict as reweight_np.psis_weights_np, lw block [M][ldw])"""
    c = ctx()
    M, K = lr.shape
    ld, ldw = ld or K + 2, ldw or K + 1
    x = np.full((M, ld), POISON)
    x[:, :K] = lr
    dx = c.array(x)
    lsel = c.empty((1, K))
    c.call("nh_column_select", dx, M, K, ld, (C.c_int * 1)(M - Mt - 1), 1, lsel)
    lw = c.array(np.full((M, ldw), POISON))
    k, n, ess, lm = c.empty((K,)), c.empty((K,), np.int64), c.empty((K,)), c.empty((K,))
    st = c.empty((K,), np.int32)
    c.call("nh_psis_weights", dx, M, K, ld, Mt, lsel, lw, ldw, k, n, ess, lm, st)
    block = lw.get()
    return dict(lw=block[:, :K], pareto_k=k.get(), n_tail=n.get(), ess=ess.get(), lmean=lm.get(),
                status=st.get()), block


def ratio_columns(rng, M):
    """the kinds of log-ratio column the kernel must take, by name"""
    logn = rng.normal(0.0, 1.5, M)
    ties = np.round(rng.normal(0.0, 1.0, M) * 2) / 2  # heavy ties, at the cutoff too
    spike = rng.normal(0.0, 0.5, M)
    spike[M // 3] += 700.0
    third = rng.normal(0.0, 1.0, M)
    third[::3] = -np.inf
    if not np.any(np.isfinite(third)):
        third[0] = 0.0
    return dict(logn=logn, ties=ties, equal=np.full(M, -2.5), spike=spike, third=third)


def check_psis(got, want):
    np.testing.assert_array_equal(got["status"], want["status"])
    np.testing.assert_array_equal(got["n_tail"], want["n_tail"])
    np.testing.assert_array_equal(np.isposinf(got["pareto_k"]), np.isposinf(want["pareto_k"]))
    np.testing.assert_array_equal(np.isnan(got["pareto_k"]), np.isnan(want["pareto_k"]))
    fin = np.isfinite(want["pareto_k"])
    np.testing.assert_allclose(got["pareto_k"][fin], want["pareto_k"][fin], rtol=RTOL, atol=ATOL)
    for key in ("lw", "ess", "lmean"):
        np.testing.assert_allclose(got[key], want[key], rtol=RTOL, atol=ATOL, err_msg=key)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("M", [6, 25, 64, 65, 1000, 2 ** 17 + 3])
def test_psis_weights_against_the_restatement(M, K):
    rng = np.random.default_rng(31 * M + K)
    cols = ratio_columns(rng, M)
    names = list(cols)
    Mt = R.tail_length(M)
    for a in range(0, len(names), K):
        pick = (names[a:a + K] + names)[:K]
        lr = np.column_stack([cols[n] for n in pick])
        for mt in (Mt, 0):
            with np.errstate(all="ignore"):
                want = R.psis_weights_np(lr, mt)
            got, block = psis_gpu(lr, mt)
            fin = np.isfinite(want["lw"])
            print(M, K, pick, mt, "k", got["pareto_k"], want["pareto_k"], "n", got["n_tail"],
                  "max |dlw|", np.max(np.abs(got["lw"][fin] - want["lw"][fin]), initial=0.0))
            check_psis(got, want)
            assert np.all(block[:, K:] == POISON)  # the padding columns are untouched
            if mt == 0:
                assert np.all(np.isposinf(got["pareto_k"])) and np.all(got["n_tail"] == 0)
    # two calls are bit-identical
    lr = np.column_stack([cols[n] for n in (names * 3)[:K]])
    a, _ = psis_gpu(lr, Mt)
    b, _ = psis_gpu(lr, Mt)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_psis_weights_bad_columns_get_nothing():
    rng = np.random.default_rng(4)
    M = 1000
    lr = rng.normal(0.0, 1.0, (M, 4))
    lr[[5, 700], 0] = np.nan
    lr[[1, 2, 999], 1] = np.inf
    lr[:, 2] = -np.inf
    lr[7, 3] = -np.inf
    got, block = psis_gpu(lr, R.tail_length(M))
    want = R.psis_weights_np(lr, R.tail_length(M))
    assert got["status"].tolist() == [2, 3, M, 0] == want["status"].tolist()
    for c in (0, 1, 2):
        assert np.all(np.isnan(got["lw"][:, c]))
        assert np.isnan(got["pareto_k"][c]) and np.isnan(got["ess"][c]) and np.isnan(got["lmean"][c])
        assert got["n_tail"][c] == 0
    check_psis(got, want)
    assert np.isneginf(got["lw"][7, 3]) and np.all(block[:, 4:] == POISON)


def test_psis_weights_follow_a_row_permutation():
    rng = np.random.default_rng(9)
    M = 5000
    lr = np.column_stack([rng.normal(0, 1.5, M), np.round(rng.normal(0, 1, M) * 2) / 2])
    perm = rng.permutation(M)
    a, _ = psis_gpu(lr, R.tail_length(M))
    b, _ = psis_gpu(lr[perm], R.tail_length(M))
    # column 0 has no ties: its weights move with their rows
    np.testing.assert_allclose(b["lw"][:, 0], a["lw"][perm, 0], rtol=0, atol=1e-12)
    # column 1 ties in the tail: rows of one ratio take the smoothed values in row order, so a
    # permutation may hand them round among those rows -- and nowhere else
    la, lb = a["lw"][:, 1], b["lw"][:, 1]
    np.testing.assert_allclose(lb[np.lexsort((lb, lr[perm, 1]))], la[np.lexsort((la, lr[:, 1]))],
                               rtol=0, atol=1e-12)
    np.testing.assert_array_equal(a["n_tail"], b["n_tail"])
    np.testing.assert_allclose(a["pareto_k"], b["pareto_k"], rtol=1e-12)


def test_psis_weights_reject_bad_arguments():
    from naima_amd import _lib
    c = ctx()
    d = c.array(np.zeros((10, 2)))
    o = [c.empty((2,)) for _ in range(3)]
    n, st, sel, lw = c.empty((2,), np.int64), c.empty((2,), np.int32), c.empty((2,)), c.empty((10, 2))
    for M, ncol, ld, Mt, ldw, msg in ((0, 2, 2, 0, 2, "M == 0"), (2 ** 31, 2, 2, 0, 2, "2\\^31"),
                                      (10, 0, 2, 0, 2, "ncol"), (10, 3, 2, 0, 3, "ncol > ld"),
                                      (10, 2, 2, 0, 1, "ncol > ldw"), (10, 2, 2, 10, 2, "Mt outside"),
                                      (10, 2, 2, -1, 2, "Mt outside"),
                                      (10 ** 6, 2, 2, 4097, 2, "NH_PSIS_MAX_TAIL")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_psis_weights", d, M, ncol, ld, Mt, sel, lw, ldw, o[0], n, o[1], o[2], st)
    with pytest.raises(_lib.NaimaHipError, match="null"):
        c.call("nh_psis_weights", d, 10, 2, 2, 0, sel, None, 2, o[0], n, o[1], o[2], st)


# ---------------------------------------------------------------------------------------
# 2. nh_weighted_select and nh_weighted_moments
# ---------------------------------------------------------------------------------------
def nasty(rng, M, ld):
    """tests/test_gpu_bands.py's columns, restated: lognormal with ties, +-inf, +-0, subnormals
    (the NaNs are placed by the caller: under zero weight, and in one column under positive)"""
    x = np.exp(rng.normal(-20, 4, size=(M, ld))) * np.where(rng.random((M, ld)) < 0.3, -1, 1)
    k = max(1, M // 50)
    for v in (np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-310):
        idx = rng.integers(0, M, size=(k, ld))
        np.put_along_axis(x, idx, v, axis=0)
    x[:, 0] = np.round(x[:, 0] * 1e9) / 1e9  # heavy ties
    if ld > 2:
        x[:, 2] = 1.25  # all equal
    return x


def log_weights(rng, M, zero_every=4):
    """normalised lognormal log-weights, every zero_every-th row (not the first) of weight zero"""
    lw = rng.normal(0.0, 1.0, M)
    lw[zero_every::zero_every] = -np.inf
    return lw - R.logsumexp(lw)


def select_gpu(x, ncol, lw_block, k, q):
    c = ctx()
    M, ld = x.shape
    dx, dl = c.array(x), c.array(lw_block)
    out = c.empty((len(q), ncol))
    c.call("nh_weighted_select", dx, M, ncol, ld, dl.ptr + 8 * k, lw_block.shape[1],
           (C.c_double * len(q))(*q), len(q), out)
    return out.get()


def moments_gpu(x, ncol, lw_block, k):
    c = ctx()
    M, ld = x.shape
    dx, dl = c.array(x), c.array(lw_block)
    out = c.empty((3, ncol))
    c.call("nh_weighted_moments", dx, M, ncol, ld, dl.ptr + 8 * k, lw_block.shape[1], out)
    return out.get()


def weighted_case(M, ncol, seed):
    """(x [M][ncol + 3], the weight block [M][3] whose column 1 is the weights, lw): NaNs and the
    columns' extremes under zero weight"""
    rng = np.random.default_rng(seed)
    x = nasty(rng, M, ncol + 3)
    lw = log_weights(rng, M)
    dead = np.isneginf(lw)
    x[dead] = np.where(rng.random((int(dead.sum()), ncol + 3)) < 0.5, np.nan,
                       np.where(rng.random((int(dead.sum()), ncol + 3)) < 0.5, 1e300, -1e300))
    block = np.full((M, 3), POISON)
    block[:, 1] = lw
    return x, block, lw


def margin_seed(M, ncol):
    """the first weight seed for which no running sum of any column lies within MARGIN of a
    threshold: the weights are the test's to choose, the condition is checked on the CPU"""
    for seed in range(1000 * M + ncol, 1000 * M + ncol + 50):
        x, block, lw = weighted_case(M, ncol, seed)
        want, ok = np.empty((len(Q), ncol)), True
        for c in range(ncol):
            want[:, c], margin = R.weighted_quantile_np(x[:, c], lw, Q)
            ok = ok and margin > MARGIN
        if ok:
            return x, block, lw, want
    raise AssertionError("no seed keeps the running sums away from the thresholds")


@pytest.mark.parametrize("ncol", [1, 5, 64])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 1000, 2 ** 17 + 3])
def test_weighted_select_is_exact(M, ncol):
    x, block, lw, want = margin_seed(M, ncol)
    got = select_gpu(x, ncol, block, 1, Q)
    np.testing.assert_array_equal(got, want)  # (-0.0 == +0.0)
    live = ~np.isneginf(lw)
    for c in range(ncol):  # zero-weight rows never appear, though they hold the extremes
        assert np.all(np.isin(got[:, c], x[live, c]))
    assert not np.any(np.abs(got) == 1e300) and not np.any(np.isnan(got))
    # a NaN under positive weight gives a NaN column, and only that one
    x2 = x.copy()
    c = ncol // 2
    x2[np.flatnonzero(live)[-1], c] = np.nan
    got2 = select_gpu(x2, ncol, block, 1, Q)
    assert np.all(np.isnan(got2[:, c]))
    np.testing.assert_array_equal(np.delete(got2, c, axis=1), np.delete(want, c, axis=1))
    # two calls are bit-identical
    assert select_gpu(x, ncol, block, 1, Q).tobytes() == got.tobytes()


@pytest.mark.parametrize("M", [64, 1024, 2 ** 17])
def test_uniform_weights_on_a_power_of_two_are_column_select(M):
    """those running sums are exact: the weighted statistic at q is rank ceil(q M) - 1.  The equal
    log-weights are 0: exp(0) is 1 in any libm, where exp(-log M) need not be 2^-k to the last
    bit, and the selection does not depend on the weights' common scale."""
    rng = np.random.default_rng(M)
    ncol = 5
    x = nasty(rng, M, ncol + 3)
    block = np.zeros((M, 1))
    got = select_gpu(x, ncol, block, 0, Q)
    ranks = [max(0, int(math.ceil(q * M)) - 1) for q in Q]
    c = ctx()
    out = c.empty((len(ranks), ncol))
    c.call("nh_column_select", c.array(x), M, ncol, ncol + 3, (C.c_int * len(ranks))(*ranks),
           len(ranks), out)
    np.testing.assert_array_equal(got, out.get())
    np.testing.assert_array_equal(got, np.sort(x[:, :ncol], axis=0)[ranks])


def test_weighted_select_in_groups_of_columns(monkeypatch):
    """a scratch budget below one call's columns: the groups give what one launch gives"""
    x, block, lw, want = margin_seed(1000, 5)
    monkeypatch.setenv("NAIMA_AMD_RANK_SCRATCH_KIB", "40")  # two columns of 1000 rows per group
    np.testing.assert_array_equal(select_gpu(x, 5, block, 1, Q), want)


@pytest.mark.parametrize("ncol", [1, 5, 64])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 1000, 2 ** 17 + 3])
def test_weighted_moments(M, ncol):
    rng = np.random.default_rng(77 * M + ncol)
    x = rng.normal(3.0, 2.0, (M, ncol + 3)) * np.exp(rng.normal(0, 1, ncol + 3))
    lw = log_weights(rng, M)
    dead = np.isneginf(lw)
    x[dead] = np.nan  # zero-weight rows are ignored whatever they hold
    if ncol > 2:
        x[~dead, 2] = 1.25  # all equal
    block = np.full((M, 3), POISON)
    block[:, 1] = lw
    got = moments_gpu(x, ncol, block, 1)
    n, mean, var = R.weighted_moments_np(x[:, :ncol], lw)
    np.testing.assert_array_equal(got[0], n.astype(float))
    np.testing.assert_allclose(got[1], mean, rtol=RTOL, atol=ATOL)
    print(M, ncol, "largest relative differences: mean",
          np.max(np.abs(got[1] - mean) / np.abs(mean)), "var",
          np.max(np.abs(got[2] - var) / np.where(var > 0, var, 1.0)))
    np.testing.assert_allclose(got[2], var, rtol=RTOL, atol=ATOL)
    if ncol > 2:
        assert got[1][2] == 1.25 and got[2][2] == 0.0  # exactly
    for v in (np.nan, np.inf):  # under positive weight: that column's mean and variance are NaN
        x2 = x.copy()
        x2[np.flatnonzero(~dead)[0], 0] = v
        g2 = moments_gpu(x2, ncol, block, 1)
        assert np.isnan(g2[1][0]) and np.isnan(g2[2][0]) and g2[0][0] == n[0]
        np.testing.assert_array_equal(g2[:, 1:], got[:, 1:])
    assert moments_gpu(x, ncol, block, 1).tobytes() == got.tobytes()


def test_weighted_reductions_reject_bad_arguments():
    from naima_amd import _lib
    c = ctx()
    d, lw, out = c.array(np.zeros((4, 3))), c.array(np.zeros(4)), c.empty((16, 3))
    q1 = (C.c_double * 1)(0.5)
    for M, ncol, ld, ldw, msg in ((0, 3, 3, 1, "M == 0"), (2 ** 31, 3, 3, 1, "2\\^31"),
                                  (4, 0, 3, 1, "ncol"), (4, 4, 3, 1, "ncol > ld"),
                                  (4, 3, 3, 0, "ldw")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_weighted_moments", d, M, ncol, ld, lw, ldw, out)
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_weighted_select", d, M, ncol, ld, lw, ldw, q1, 1, out)
    for q, msg in (([-0.1], "outside"), ([1.5], "outside"), ([float("nan")], "outside"),
                   ([0.5] * 17, "nq"), ([], "nq")):
        arr = (C.c_double * max(len(q), 1))(*q)
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_weighted_select", d, 4, 3, 3, lw, 1, arr, len(q), out)
    with pytest.raises(_lib.NaimaHipError, match="null"):
        c.call("nh_weighted_moments", d, 4, 3, 3, None, 1, out)


# ---------------------------------------------------------------------------------------
# 3. nh_resample_systematic, nh_gather_rows, nh_row_sums_select
# ---------------------------------------------------------------------------------------
def draw_gpu(lw_block, k, u0, n_out):
    c = ctx()
    dl = c.array(lw_block)
    idx = c.empty((n_out,), np.int64)
    c.call("nh_resample_systematic", dl.ptr + 8 * k, lw_block.shape[1], lw_block.shape[0], u0,
           n_out, idx)
    return idx


@pytest.mark.parametrize("M", [1, 7, 1000, 5000])
def test_systematic_resampling_and_the_gather(M):
    for n_out in sorted({1, M, 3 * M, 4096}):
        for seed in range(100 * M + n_out, 100 * M + n_out + 50):
            rng = np.random.default_rng(seed)
            lw = log_weights(rng, M, zero_every=3)
            u0 = float(rng.random())
            want, margin = R.systematic_np(lw, u0, n_out)
            if margin > MARGIN:
                break
        else:
            raise AssertionError("no seed keeps the running sums away from the thresholds")
        block = np.full((M, 2), POISON)
        block[:, 1] = lw
        didx = draw_gpu(block, 1, u0, n_out)
        idx = didx.get()
        np.testing.assert_array_equal(idx, want)
        assert np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < M
        cnt = np.bincount(idx, minlength=M)
        nw = n_out * np.exp(lw)  # (normalised; exp(-inf) = 0)
        # floor or ceil of n w, up to the rounding of n w itself at an integer
        assert np.all((cnt >= np.floor(nw * (1 - 1e-12))) & (cnt <= np.ceil(nw * (1 + 1e-12))))
        assert np.all(cnt[np.isneginf(lw)] == 0)
        assert draw_gpu(block, 1, u0, n_out).get().tobytes() == idx.tobytes()
        # the gather, ld != ldo, padding untouched
        c = ctx()
        x = rng.normal(size=(M, 6))
        x[0, 0], x[-1, 3] = np.nan, -0.0
        out = c.array(np.full((n_out, 5), POISON))
        c.call("nh_gather_rows", c.array(x), 6, didx, n_out, 4, out, 5)
        got = out.get()
        assert got[:, :4].tobytes() == np.ascontiguousarray(x[idx, :4]).tobytes()
        assert np.all(got[:, 4] == POISON)


def test_resampling_without_a_positive_weight_and_bad_arguments():
    from naima_amd import _lib
    c = ctx()
    assert np.all(draw_gpu(np.full((10, 1), -np.inf), 0, 0.5, 7).get() == -1)
    lw, idx = c.array(np.zeros(4)), c.empty((4,), np.int64)
    for ldw, M, u0, n, msg in ((1, 0, 0.5, 4, "M == 0"), (1, 2 ** 31, 0.5, 4, "2\\^31"),
                               (0, 4, 0.5, 4, "ldw"), (1, 4, 1.0, 4, "u0"), (1, 4, -0.1, 4, "u0"),
                               (1, 4, 0.5, 0, "n_out"), (1, 4, 0.5, 2 ** 31, "n_out")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_resample_systematic", lw, ldw, M, u0, n, idx)
    x, out = c.array(np.zeros((4, 3))), c.empty((4, 3))
    for ld, n, ncol, ldo, msg in ((3, 0, 3, 3, "n_out"), (3, 4, 0, 3, "ncol"), (2, 4, 3, 3, "ncol > ld"),
                                  (3, 4, 3, 2, "ncol > ldo")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_gather_rows", x, ld, idx, n, ncol, out, ldo)


@pytest.mark.parametrize("M", [1, 257, 70000])
def test_row_sums_of_chosen_columns(M):
    from naima_amd import _lib
    from naima_amd import reweight as RW
    rng = np.random.default_rng(M)
    ncol = 70
    L = -rng.random((M, ncol)) * 10
    groups = [[3, 1, 3], [], list(range(ncol)) + list(range(ncol - 1, -1, -1)), [69]]
    for fn, sign in ((RW.drop_points, -1), (RW.add_points, +1)):
        got = fn(L, groups)
        assert (got.M, got.ncol) == (M, len(groups))
        np.testing.assert_array_equal(got.get(), R.row_sums(L, groups, sign))  # the same order
    c = ctx()
    d, out = c.array(L), c.empty((M,))
    for n, cols, sign, ldo, msg in ((1, [70], 1, 1, "outside"), (1, [-1], 1, 1, "outside"),
                                    (-1, [0], 1, 1, "negative"), (1, [0], 0, 1, "sign"),
                                    (1, [0], 1, 0, "ldo")):
        with pytest.raises(_lib.NaimaHipError, match=msg):
            c.call("nh_row_sums_select", d, M, ncol, ncol, (C.c_int * 1)(*cols), n, sign, out, ldo)


# ---------------------------------------------------------------------------------------
# 4. the module on host arrays
# ---------------------------------------------------------------------------------------
def test_module_functions_against_the_restatement():
    from naima_amd import reweight as RW
    rng = np.random.default_rng(12)
    M = 3000
    lr = np.column_stack([rng.normal(0, 1.0, M), rng.normal(0, 0.3, M)])
    lr[::5, 1] = -np.inf
    x = rng.normal(size=(M, 4))
    x[::5] = np.nan
    w = RW.psis_weights(lr)
    want = R.psis_weights_np(lr, R.tail_length(M))
    assert (w.tail_length, w.n_samples, w.n_targets) == (R.tail_length(M), M, 2)
    check_psis(dict(lw=w.lw.get(), pareto_k=w.pareto_k, n_tail=w.n_tail, ess=w.ess,
                    lmean=w.log_mean_ratio, status=np.zeros(2, np.int32)), want)
    st = RW.weighted_stats(x, w, k=1)
    # (the moments under the weights the device itself holds: the restatement's differ from them
    # by up to RTOL each, which a mean of values of both signs would show without any bound)
    n, mean, var = R.weighted_moments_np(x, w.lw.get()[:, 1])
    np.testing.assert_array_equal(st["n_used"], n)
    np.testing.assert_allclose(st["mean"], mean, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"], var, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["sd"], np.sqrt(var), rtol=RTOL, atol=ATOL)
    assert np.all(np.isnan(RW.weighted_stats(x, w, k=0)["mean"]))  # NaNs under positive weight
    q = RW.weighted_quantiles(x, w, np.linspace(0.01, 0.99, 21), k=1)
    assert q.shape == (21, 4) and np.all(np.diff(q, axis=0) >= 0)
    idx = RW.resample_index(w, seed=3, k=1)
    assert len(idx) == max(1, int(round(w.ess[1]))) and not np.any(idx % 5 == 0)
    r = RW.resample(x, w, seed=3, k=1)
    assert r.get().tobytes() == np.ascontiguousarray(x[idx]).tobytes()
    plain = RW.psis_weights(lr[:, 0], smooth=False)
    assert plain.tail_length == 0 and np.isposinf(plain.pareto_k[0])
    np.testing.assert_allclose(plain.lw.get()[:, 0], lr[:, 0] - R.logsumexp(lr[:, 0]), rtol=RTOL,
                               atol=ATOL)
    bad = lr.copy()
    bad[[1, 2, 3], 0] = np.nan
    with pytest.raises(ValueError, match="3 of the"):
        RW.psis_weights(bad)
    # +inf warns where a tail exists but is too short to fit (one row carries the weight), and
    # does not where no row lies above the cutoff (equal ratios)
    spike = np.zeros(6)
    spike[2] = 50.0
    with pytest.warns(UserWarning, match="1 of the 1 targets"):
        one = RW.psis_weights(spike)
    assert np.isposinf(one.pareto_k[0]) and one.n_tail[0] == 1 and one.ess[0] < 1.0 + 1e-9
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isposinf(RW.psis_weights(np.full(50, 1.5)).pareto_k[0])
    heavy = np.column_stack([8.0 * rng.standard_normal(M) ** 2, lr[:, 0]])
    with pytest.warns(UserWarning, match="1 of the 2 targets"):
        assert RW.psis_weights(heavy).pareto_k[0] > 0.7


# ---------------------------------------------------------------------------------------
# 5. a whole fit
# ---------------------------------------------------------------------------------------
NW, NSTEPS = 64, 30


@pytest.fixture(scope="module")
def fit():
    import naima_amd as na
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    data["group"] = (data["energy"].to("eV").value > 1e9).astype(int)  # X-ray | VHE
    s = EnsembleSampler(NW, p0.size, na.lnprob, args=[data, model, prior], seed=5,
                        naima_style=True, device=True)
    start = p0 * (1 + 0.01 * np.random.default_rng(1).standard_normal((NW, p0.size)))
    s.run_mcmc(start, NSTEPS)
    s.data, s.labels, s.modelfn = data, list(labels), model
    return s


def host_pointwise(s):
    """the restatement of the pointwise matrix on the downloaded blobs (test_gpu_infocrit.py)"""
    import infocrit_np as IN
    from naima_amd.core import _conversion_to_data
    b = np.asarray(s.get_blobs()[0], dtype=float)
    d = s.data
    unit = d["flux"].unit
    cl = np.concatenate([d["cl"], d["cl"][-1:]])
    return IN.pointwise_lnl(b.reshape(-1, b.shape[2]), _conversion_to_data(s.blob_units[0], d),
                            d["flux"].value, d["flux_error_lo"].to(unit).value,
                            d["flux_error_hi"].to(unit).value, d["ul"], cl)


def test_dropping_nothing_changes_nothing(fit):
    from naima_amd import plot as P
    from naima_amd import posterior as PO
    M = NW * NSTEPS
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (equal ratios are no heavy tail: no warning)
        rw = fit.reweight(drop=[])
    w = rw.weights
    assert w.n_samples == M and np.isposinf(w.pareto_k[0]) and w.n_tail[0] == 0
    np.testing.assert_allclose(w.lw.get()[:, 0], -math.log(M), rtol=1e-14)
    np.testing.assert_allclose(w.ess[0], M, rtol=1e-12)
    assert rw.log_evidence_ratio == 0.0
    chain = fit.get_chain(flat=True)
    sm = rw.summary()
    st = PO.column_stats(chain)
    ranks = [int(q * (M - 1)) for q in (0.5, 0.16, 0.84)]
    sel = P.column_select(chain, ranks)
    assert sm["labels"] == fit.labels
    np.testing.assert_array_equal(sm["mean_unweighted"], st["mean"])
    np.testing.assert_array_equal(sm["sd_unweighted"], np.sqrt(st["var"]))
    for j, key in enumerate(("median", "q16", "q84")):
        np.testing.assert_array_equal(sm[key + "_unweighted"], sel[j])
        np.testing.assert_array_equal(sm[key], sel[j])  # equal weights: the same order statistic
    np.testing.assert_allclose(sm["mean"], st["mean"], rtol=1e-12)
    np.testing.assert_allclose(sm["sd"], np.sqrt(st["var"] * (M - 1) / M), rtol=1e-9)
    np.testing.assert_allclose(sm["shift"], 0.0, atol=1e-9)
    assert np.all(sm["n_used"] == M)
    for confs in ([3, 1], [2, 0.5]):
        mx, CI = rw.bands(confs=confs)
        mx0, CI0 = P._calc_CI(fit, 0, confs=confs)
        assert np.array_equal(mx.value, mx0.value) and len(CI) == len(CI0)
        for (lo, hi), (lo0, hi0) in zip(CI, CI0):
            assert lo.unit == lo0.unit
            np.testing.assert_array_equal(lo.value, lo0.value)
            np.testing.assert_array_equal(hi.value, hi0.value)


def test_dropping_a_group_and_influence(fit):
    from naima_amd import posterior as PO
    # Two references.  (a) The restatement on the host pointwise matrix LH, for the weights
    # WITHOUT smoothing: the device's matrix is held to LH at RTOL, ATOL (as
    # tests/test_gpu_infocrit.py does), a ratio is a sum of len(cols) of its entries, so the
    # ratios differ by at most eps = sum_k (RTOL |LH_k| + ATOL) per row, and
    # lw = lr - logsumexp(lr) by at most 2 eps.  (b) For the SMOOTHED weights the restatement is
    # fed with the device's matrix L, so that both sides fit the same tail: behind a generalised-
    # Pareto fit an input error of 1e-9 |L| has no bound of its own.
    LH = host_pointwise(fit)
    L = fit.get_pointwise_log_likelihood().get()
    np.testing.assert_allclose(L, LH, rtol=RTOL, atol=ATOL)
    M = L.shape[0]
    groups = np.asarray(fit.data["group"])
    chain = fit.get_chain(flat=True)
    Mt = R.tail_length(M)
    st = PO.column_stats(chain)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        infl = fit.influence()
        assert [r["group"] for r in infl] == [0, 1]
        for g in (0, 1):
            cols = [int(c) for c in np.flatnonzero(groups == g)]
            with np.errstate(all="ignore"):
                want = R.psis_weights_np(R.row_sums(L, [cols], -1), Mt)
            rw = fit.reweight(drop={"group": g})
            w = rw.weights
            print("group", g, "k", w.pareto_k, want["pareto_k"], "ess", w.ess, want["ess"])
            check_psis(dict(lw=w.lw.get(), pareto_k=w.pareto_k, n_tail=w.n_tail, ess=w.ess,
                            lmean=w.log_mean_ratio, status=np.zeros(1, np.int32)), want)
            assert rw.log_evidence_ratio == w.log_mean_ratio[0]
            assert fit.reweight(drop=cols).weights.lw.get().tobytes() == w.lw.get().tobytes()
            eps = (RTOL * np.abs(LH[:, cols]) + ATOL).sum(axis=1).max()
            plain = fit.reweight(drop={"group": g}, smooth=False).weights
            ph = R.psis_weights_np(R.row_sums(LH, [cols], -1), 0)
            print("unsmoothed, host matrix: eps", eps, "largest |dlw|",
                  np.max(np.abs(plain.lw.get() - ph["lw"])))
            np.testing.assert_allclose(plain.lw.get(), ph["lw"], rtol=RTOL, atol=2 * eps + ATOL)
            np.testing.assert_allclose(plain.log_mean_ratio, ph["lmean"], rtol=RTOL, atol=eps + ATOL)
            # the moments under the weights the device holds (the restatement's own differ by RTOL)
            n, mean, var = R.weighted_moments_np(chain, w.lw.get()[:, 0])
            sm = rw.summary()
            np.testing.assert_allclose(sm["mean"], mean, rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(sm["sd"], np.sqrt(var), rtol=RTOL, atol=ATOL)
            r = infl[g]
            assert r["n_points"] == len(cols)
            # column by column: K = 2 columns are tiled otherwise than one, so sums over the rows
            # may differ in their last bits; pareto_k depends on the sorted tail alone
            assert r["pareto_k"] == w.pareto_k[0]
            np.testing.assert_allclose(r["ess"], w.ess[0], rtol=1e-12)
            sd = np.sqrt(st["var"])
            print("shift", r["shift"], sm["shift"], (mean - st["mean"]) / sd)
            # (the two calls' weights agree to 1e-12 relative -- the ESS above --, and the chain's
            # values are of one sign: the means do, and a shift is a mean over sd)
            assert np.all(np.abs(r["shift"] - sm["shift"]) <= 1e-12 * np.abs(st["mean"]) / sd)
            # shift = (mean - fitted mean) / sd with the mean held to RTOL, ATOL
            assert np.all(np.abs(sm["shift"] - (mean - st["mean"]) / sd)
                          <= (RTOL * np.abs(mean) + ATOL) / sd)


def test_new_data_equal_to_three_of_the_tables_points(fit):
    from naima_amd import reweight as RW
    from naima_amd import units as u
    from naima_amd.core import _conversion_to_data
    d = fit.data
    pts = [int(i) for i in np.flatnonzero(~np.asarray(d["ul"]))[[1, 4, -2]]]
    new = {k: u.Quantity(d[k].value[pts], d[k].unit)
           for k in ("energy", "flux", "flux_error_lo", "flux_error_hi")}
    new["ul"], new["cl"] = np.zeros(3, bool), np.asarray(d["cl"])[pts]
    lr_got = RW._new_data_ratio(fit, new, 0, 1, 0).get()[:, 0]
    lr_ref = RW.add_points(fit.get_pointwise_log_likelihood(), [pts]).get()[:, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = fit.reweight(new_data=new)
        ref = fit.reweight(log_ratio=lr_got)
    assert got.weights.lw.get().tobytes() == ref.weights.lw.get().tobytes()
    assert got.weights.pareto_k.tobytes() == ref.weights.pareto_k.tobytes()
    b = np.asarray(fit.get_blobs()[0], dtype=float).reshape(-1, len(d["energy"]))[:, pts]
    m = b * _conversion_to_data(fit.blob_units[0], d)[pts]
    dd = m - d["flux"].value[pts]
    unit = d["flux"].unit
    sg = np.where(dd > 0, d["flux_error_hi"].to(unit).value[pts], d["flux_error_lo"].to(unit).value[pts])
    tol = np.sum(RT_MODEL * np.abs(m) * (np.abs(dd) + RT_MODEL * np.abs(m)) / sg ** 2, axis=1)
    print("largest |difference| / tolerance", np.max(np.abs(lr_got - lr_ref) / tol))
    assert np.all(np.abs(lr_got - lr_ref) <= tol)


def test_a_saved_run_reweights_bit_identically(fit, tmp_path):
    import naima_amd as na
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        back = na.read_run(na.save_run(str(tmp_path / "run.npz"), fit))
        a, b = fit.reweight(drop={"group": 1}), back.reweight(drop={"group": 1})
        for key in ("pareto_k", "n_tail", "ess", "log_mean_ratio"):
            assert getattr(a.weights, key).tobytes() == getattr(b.weights, key).tobytes(), key
        assert a.weights.lw.get().tobytes() == b.weights.lw.get().tobytes()
        sa, sb = a.summary(), b.summary()
        for key in ("mean", "sd", "median", "q16", "q84", "shift"):
            assert sa[key].tobytes() == sb[key].tobytes(), key
        assert [r["pareto_k"] for r in back.influence()] == [r["pareto_k"] for r in fit.influence()]
        with pytest.raises(ValueError, match="modelfn"):
            back.reweight(new_data={})


def test_a_resampled_chain_feeds_the_posterior_reductions(fit):
    from naima_amd import plot as P
    from naima_amd import posterior as PO
    from naima_amd.dview import DeviceMatrix
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rw = fit.reweight(drop={"group": 1})
    r = rw.resample(n=500, seed=2)
    assert isinstance(r, DeviceMatrix) and (r.M, r.ncol) == (500, fit.get_chain().shape[-1])
    host = r.get()
    chain = fit.get_chain(flat=True)
    from naima_amd import reweight as RW
    np.testing.assert_array_equal(host, chain[RW.resample_index(rw.weights, n=500, seed=2)])
    h, edges = PO.histogram(r, bins=12)
    for c in range(r.ncol):
        np.testing.assert_array_equal(h[c], np.histogram(host[:, c], bins=12,
                                                         range=(host[:, c].min(), host[:, c].max()))[0])
    np.testing.assert_array_equal(P.column_select(r, [0, 250, 499]), np.sort(host, axis=0)[[0, 250, 499]])
    n = rw.resample()
    assert n.M == max(1, int(round(rw.weights.ess[0])))
    q = rw.quantiles([0.16, 0.5, 0.84])
    assert q.shape == (3, r.ncol) and np.all(np.diff(q, axis=0) >= 0)


# ---------------------------------------------------------------------------------------
# 6. the example
# ---------------------------------------------------------------------------------------
def test_the_example_weighs_the_data_sets():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "rxj1713_influence", os.path.join(ROOT, "examples", "rxj1713_influence.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    infl, added = ex.main(nwalkers=32, nburn=5, nrun=20, verbose=False, prefit=False)
    assert [r["group"] for r in infl] == [0, 1] and sum(r["n_points"] for r in infl) > 5
    assert all(r["shift"].shape == (5,) for r in infl)
    assert added.weights.n_samples == 32 * 10 and np.isfinite(added.log_evidence_ratio)
    assert added.summary()["labels"] == ex.LABELS
