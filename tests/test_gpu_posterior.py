"""Posterior reductions on the GPU (naima_amd.posterior: nh_column_moments, nh_hist_columns,
nh_kde_columns) against NumPy and scipy on the host: integer equality of the histograms with
np.histogram / np.histogram2d, the moments and the KDE within the rounding of their sums,
determinism, and the figures built on them (the built-in corner plot, plot_chain's posterior
panel)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
MS = [1, 2, 63, 64, 65, 257, 4099, 70001]
NBS = [1, 2, 20, 37, 100]
KDE_RTOL, KDE_ATOL = 1e-11, 1e-300


def column(rng, kind, M):
    """columns of very different scale: N(0,1); 7 +- 1e-3 rounded to 4 decimals (ties);
    -200 +- 50"""
    if kind % 3 == 0:
        return rng.normal(0.0, 1.0, M) * (1 + kind // 3)
    if kind % 3 == 1:
        return np.round(7.0 + 1e-3 * rng.normal(size=M), 4)
    return -200.0 + 50.0 * rng.normal(size=M)


def samples(M, ncol, nb, seed=0):
    """[M][ncol]: with samples exactly on the edges np.linspace(min, max, nb+1) of every column
    (as many as fit), one NaN and one +inf"""
    rng = np.random.default_rng(1000 * seed + 7 * M + 13 * ncol + nb)
    x = np.stack([column(rng, c, M) for c in range(ncol)], 1)
    if M >= 5:
        k = min(nb + 1, M - 4)
        for c in range(ncol):
            lo, hi = x[:, c].min(), x[:, c].max()
            x[0, c], x[1, c] = lo, hi
            x[2:2 + k, c] = np.linspace(lo, hi, nb + 1)[:k]
        x[M - 1, 0] = np.nan
        x[M - 2, ncol - 1] = np.inf
    return x


def on_device(x, pad=2):
    """x [M][ncol] inside a device matrix of ld = ncol + pad, the padding NaN"""
    from naima_amd import _lib
    M, ncol = x.shape
    host = np.full((M, ncol + pad), np.nan)
    host[:, :ncol] = x
    return (_lib.get_context().array(host), M, ncol, ncol + pad)


def finite_range(col):
    f = col[np.isfinite(col)]
    return f.min(), f.max()


def check_hist1d(h1, edges, x, rng_of=finite_range):
    for c in range(x.shape[1]):
        col = x[:, c][np.isfinite(x[:, c])]
        want, e = np.histogram(col, bins=h1.shape[1], range=rng_of(x[:, c]))
        np.testing.assert_array_equal(edges[c], e)
        np.testing.assert_array_equal(h1[c], want)


def check_hist2d(H, pairs, edges, x):
    assert H.dtype == np.int64 and H.shape == (len(pairs),) + (edges.shape[1] - 1,) * 2
    for p, (i, j) in enumerate(pairs):
        ok = np.isfinite(x[:, i]) & np.isfinite(x[:, j])
        want = np.histogram2d(x[ok, i], x[ok, j], bins=[edges[i], edges[j]])[0]
        np.testing.assert_array_equal(H[p], want.astype(np.int64))
        inside = ok & (x[:, i] >= edges[i][0]) & (x[:, i] <= edges[i][-1]) \
            & (x[:, j] >= edges[j][0]) & (x[:, j] <= edges[j][-1])
        assert H[p].sum() == inside.sum()


# ---------------------------------------------------------------------------------------
# histograms
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
def test_histograms_equal_numpy_s(M):
    from naima_amd import posterior as P
    for ncol in (1, 3, 7):
        for nb in NBS:
            x = samples(M, ncol, nb)
            d = on_device(x)
            h1, edges = P.histogram(d, bins=nb)
            assert h1.dtype == np.int64 and h1.shape == (ncol, nb)
            check_hist1d(h1, edges, x)
            H, pairs, e2 = P.histogram_pairs(d, bins=nb)
            assert pairs == [(i, j) for i in range(ncol) for j in range(i + 1, ncol)]
            np.testing.assert_array_equal(e2, edges)
            check_hist2d(H, pairs, edges, x)


def test_host_arrays_and_one_dimensional_input():
    from naima_amd import posterior as P
    x = samples(257, 3, 20)
    h1, edges = P.histogram(x, bins=20)
    check_hist1d(h1, edges, x)
    h0, e0 = P.histogram(x[:, 0], bins=20)
    np.testing.assert_array_equal(h0, h1[:1])
    np.testing.assert_array_equal(e0, edges[:1])
    H, pairs, _ = P.histogram_pairs(x[:, 0], bins=20)
    assert H.shape == (0, 20, 20) and pairs == []


def test_pair_histograms_in_several_groups_do_not_depend_on_the_grouping():
    """12 columns at 40 bins: 66 pair histograms of 1600 counters, several launches of as many
    as fit a workgroup's LDS"""
    from naima_amd import posterior as P
    x = samples(4099, 12, 40)
    d = on_device(x, pad=1)
    H, pairs, edges = P.histogram_pairs(d, bins=40)
    assert len(pairs) == 66
    check_hist2d(H, pairs, edges, x)
    h1, e1 = P.histogram(d, bins=40)
    check_hist1d(h1, e1, x)
    # the same pairs asked for alone, reversed and in another order
    some = [(3, 9), (9, 3), (0, 11), (5, 5), (10, 11)]
    Hs, ps, _ = P.histogram_pairs(d, bins=40, pairs=some)
    assert ps == some
    np.testing.assert_array_equal(Hs[0], H[pairs.index((3, 9))])
    np.testing.assert_array_equal(Hs[1], Hs[0].T)
    np.testing.assert_array_equal(Hs[2], H[pairs.index((0, 11))])
    np.testing.assert_array_equal(Hs[3], np.diag(h1[5]))
    np.testing.assert_array_equal(Hs[4], H[pairs.index((10, 11))])


def test_a_constant_column_and_an_explicit_range():
    from naima_amd import posterior as P
    x = samples(4099, 3, 20)
    x[:, 1] = 7.3
    d = on_device(x)
    h1, edges = P.histogram(d, bins=20)
    np.testing.assert_array_equal(edges[1], np.histogram(np.full(3, 7.3), bins=20)[1])
    assert edges[1][0] == 7.3 - 0.5 and edges[1][-1] == 7.3 + 0.5
    check_hist1d(h1, edges, x)
    assert h1[1].sum() == 4099 and h1[1].max() == 4099
    H, pairs, e2 = P.histogram_pairs(d, bins=20)
    check_hist2d(H, pairs, e2, x)
    # a range that cuts samples off: one for every column, then one each
    for rng_ in ((-1.0, 1.5), [(-1.0, 1.5), (7.3, 7.3), (-260.0, -100.0)]):
        per = np.tile(rng_, (3, 1)) if np.ndim(rng_) == 1 else np.asarray(rng_)
        h1, edges = P.histogram(d, bins=37, range=rng_)
        for c in range(3):
            col = x[:, c][np.isfinite(x[:, c])]
            want, e = np.histogram(col, bins=37, range=tuple(per[c]))
            np.testing.assert_array_equal(edges[c], e)
            np.testing.assert_array_equal(h1[c], want)
        assert h1[0].sum() < np.isfinite(x[:, 0]).sum()
        H, pairs, e2 = P.histogram_pairs(d, bins=37, range=rng_)
        np.testing.assert_array_equal(e2, edges)
        check_hist2d(H, pairs, e2, x)


def test_the_library_refuses_what_is_beyond_its_caps():
    import ctypes as C

    from naima_amd import _lib
    ctx = _lib.get_context()
    x = ctx.array(np.zeros((8, 2)))
    big = _lib.NH_HIST_MAX_BINS_2D + 1
    edges = ctx.array(np.tile(np.linspace(-1, 1, big + 1), (2, 1)))
    h1, h2 = ctx.empty((2, big), np.int64), ctx.empty((1, big, big), np.int64)
    ctx.call("nh_hist_columns", x, 8, 2, 2, edges, big, None, 0, h1, None)  # (1-D: within its cap)
    np.testing.assert_array_equal(h1.get().sum(1), [8, 8])
    for args in ((x, 8, 2, 2, edges, big, (C.c_int * 2)(0, 1), 1, h1, h2),
                 (x, 8, 2, 2, edges, 20, (C.c_int * 2)(0, 2), 1, h1, h2),
                 (x, 8, 2, 2, edges, 0, None, 0, h1, None),
                 (x, 8, 2, 2, edges, _lib.NH_HIST_MAX_BINS_1D + 1, None, 0, h1, None),
                 (x, 0, 2, 2, edges, 20, None, 0, h1, None),
                 (x, 8, 3, 2, edges, 20, None, 0, h1, None)):
        with pytest.raises(_lib.NaimaHipError, match="nh_hist_columns"):
            ctx.call("nh_hist_columns", *args)


# ---------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
def test_moments(M):
    """n, n_nan, min and max exact; mean within M eps mean(|x|) and var within M eps (1e-12 up
    to M = 4099), the worst case of a sum of M terms"""
    from naima_amd import posterior as P
    for ncol in (1, 3, 7, 70):
        x = samples(M, ncol, 20)
        if M >= 5:
            x[3, ncol // 2] = -np.inf
            x[M - 3, 0] = np.nan
        st = P.column_stats(on_device(x))
        assert st["n"].dtype == np.int64 and st["n_nan"].dtype == np.int64
        for c in range(ncol):
            col = x[:, c]
            f = col[np.isfinite(col)]
            assert st["n"][c] == f.size and st["n_nan"][c] == np.isnan(col).sum()
            assert st["min"][c] == f.min() and st["max"][c] == f.max()
            assert abs(st["mean"][c] - np.mean(f)) <= M * EPS * np.mean(np.abs(f))
            if f.size > 1:
                np.testing.assert_allclose(st["var"][c], np.var(f, ddof=1),
                                           rtol=max(1e-12, M * EPS), atol=0)
            else:
                assert np.isnan(st["var"][c])


def test_moments_of_a_constant_column_are_exact():
    from naima_amd import posterior as P
    x = samples(4099, 3, 20)
    x[:, 1] = 0.1 + 0.2  # (not a sum that rounds back to itself when added 4099 times)
    x[5, 1] = np.nan
    st = P.column_stats(x)
    assert st["var"][1] == 0.0 and st["mean"][1] == 0.1 + 0.2
    assert st["n"][1] == 4098 and st["n_nan"][1] == 1
    assert st["var"][0] > 0 and st["var"][2] > 0
    # no finite value at all
    st = P.column_stats(np.array([np.nan, np.inf, -np.inf]))
    assert st["n"][0] == 0 and st["n_nan"][0] == 1
    assert all(np.isnan(st[k][0]) for k in ("min", "max", "mean", "var"))


# ---------------------------------------------------------------------------------------
# KDE
# ---------------------------------------------------------------------------------------
def kde_formula(col, pts, h):
    f = col[np.isfinite(col)]
    u = (pts[:, None] - f[None, :]) / h
    return np.exp(-0.5 * u * u).sum(1) / (f.size * h * np.sqrt(2 * np.pi))


def factor(bw, n):
    return n ** -0.2 if bw in (None, "scott") else (0.75 * n) ** -0.2 if bw == "silverman" else bw


def check_kde(x, G, bw, pad=2, scipy_too=True):
    from naima_amd import posterior as P
    ncol = x.shape[1]
    pts = np.empty((ncol, G))
    for c in range(ncol):
        f = x[:, c][np.isfinite(x[:, c])]
        pts[c] = np.mean(f) + np.std(f, ddof=1) * np.linspace(-4, 4, G)
    got = P.gaussian_kde(on_device(x, pad), pts, bw_method=bw)
    assert got.shape == (ncol, G)
    for c in range(ncol):
        f = x[:, c][np.isfinite(x[:, c])]
        h = factor(bw, f.size) * np.sqrt(np.var(f, ddof=1))
        np.testing.assert_allclose(got[c], kde_formula(x[:, c], pts[c], h), rtol=KDE_RTOL,
                                   atol=KDE_ATOL)
        if scipy_too:
            # scipy divides data and points by the bandwidth BEFORE it subtracts them: on the
            # 7 +- 1e-3 column that rounds away eps * 7 / h ~ 8e-12 of every argument, several
            # times the bound, in the reference itself.  There scipy gets data and points with
            # 7 taken off, which is exact (Sterbenz: both lie in [3.5, 14]) and leaves the
            # density what it was.
            shift = 7.0 if c % 3 == 1 else 0.0
            assert np.all((f - shift) + shift == f)
            stats = pytest.importorskip("scipy.stats")
            want = stats.gaussian_kde(f - shift, bw_method=bw)(pts[c] - shift)
            np.testing.assert_allclose(got[c], want, rtol=KDE_RTOL, atol=KDE_ATOL)
    return got


@pytest.mark.parametrize("bw", [None, "scott", "silverman", 0.3])
def test_kde_is_the_formula_and_scipy_s(bw):
    """at 101 points over +-4 sigma; M = 4099 spans five row chunks"""
    for M in (2, 65, 257, 4099):
        x = samples(M, 3, 20)
        if M == 2:
            x[:, 1] = [7.0, 7.0001]
        check_kde(x, 101, bw)


def test_kde_point_tiles_stages_and_one_point_for_all_columns():
    from naima_amd import posterior as P
    check_kde(samples(300, 2, 20), 300, None, pad=0)  # (two tiles of 256 points, a ragged one)
    check_kde(samples(257, 3, 20), 37, "silverman")   # (four row lanes per point)
    check_kde(samples(65, 1, 20), 1, 0.5)
    # 32 columns x 70 001 rows: chunks longer than one LDS stage.  (The device adds at most
    # rows per chunk / row lanes + chunks ~ 100 terms in a row, NumPy's pairwise sum fewer: the
    # bound of 1e-11 holds here as it does for M <= 4099.)
    check_kde(samples(70001, 32, 20), 5, None, pad=1, scipy_too=False)
    x = samples(257, 3, 20)
    pts = np.linspace(-300, 10, 50)
    np.testing.assert_array_equal(P.gaussian_kde(x, pts), P.gaussian_kde(x, np.tile(pts, (3, 1))))


def test_kde_of_a_constant_column_raises():
    from naima_amd import posterior as P
    x = samples(257, 3, 20)
    x[:, 2] = 4.0
    with pytest.raises(ValueError, match="positive variance"):
        P.gaussian_kde(x, np.linspace(0, 1, 5))
    with pytest.raises(ValueError, match="positive variance"):
        P.gaussian_kde(np.array([1.0]), [0.0])


# ---------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    from naima_amd import posterior as P
    x = samples(70001, 7, 37)
    d = on_device(x)
    pts = np.linspace(-5, 5, 101)
    runs = []
    for _ in range(2):
        st = P.column_stats(d)
        h1, e = P.histogram(d, bins=37)
        H, _, _ = P.histogram_pairs(d, bins=37)
        k = P.gaussian_kde(d, pts)
        runs.append(b"".join(st[n].tobytes() for n in sorted(st)) + h1.tobytes() + e.tobytes()
                    + H.tobytes() + k.tobytes())
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------
# figures
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg3_run():
    import naima_amd as na
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg3", na)
    nw = 64
    s = EnsembleSampler(nw, p0.size, na.lnprob, args=[data, model, prior], seed=5,
                        naima_style=True, device=True)
    start = p0 * (1 + 0.01 * np.random.default_rng(1).standard_normal((nw, p0.size)))
    s.run_mcmc(start, 10)
    s.data, s.labels, s.modelfn = data, list(labels), model
    return s


def _stairs(ax):
    from matplotlib.patches import StepPatch
    return [p for p in ax.patches if isinstance(p, StepPatch)]


def test_plot_corner_draws_the_built_in_figure(cfg3_run):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.contour import ContourSet

    import naima_amd as na
    from naima_amd import posterior as P
    s = cfg3_run
    chain = np.asarray(s.get_chain(flat=True))
    n = chain.shape[1]
    with pytest.warns(UserWarning, match="corner"):
        f = na.plot_corner(s)
    assert f is not None and len(f.axes) == n * n
    axes = np.array(f.axes).reshape(n, n)
    h1, edges = P.histogram(chain, bins=20)
    H, pairs, e2 = P.histogram_pairs(chain, bins=20)
    np.testing.assert_array_equal(e2, edges)
    for c in range(n):
        want = np.histogram(chain[:, c], bins=20)[0]
        np.testing.assert_array_equal(h1[c], want)
    q = np.percentile(chain, [16, 50, 84], axis=0)
    lp = np.asarray(s.get_log_prob())
    MLp = np.asarray(s.get_chain())[np.unravel_index(np.argmax(lp), lp.shape)]
    for r in range(n):
        for c in range(n):
            ax = axes[r, c]
            if c > r:
                assert not ax.get_visible()
                continue
            assert ax.get_visible()
            if r == c:
                (st,) = _stairs(ax)
                np.testing.assert_array_equal(st.get_data().values, h1[c])
                np.testing.assert_array_equal(st.get_data().edges, edges[c])
                xs = sorted(ln.get_xdata()[0] for ln in ax.lines)
                want = sorted(list(q[:, c]) + [MLp[c]])
                np.testing.assert_allclose(xs, want, rtol=1e-13, atol=0)
            else:
                Hp = H[pairs.index((c, r))]
                sets = [a for a in ax.collections if isinstance(a, ContourSet)]
                assert len(sets) == 1
                np.testing.assert_array_equal(sets[0].levels,
                                              np.unique(P.contour_thresholds(Hp)))
                (mesh,) = [a for a in ax.collections if type(a).__name__ == "QuadMesh"]
                np.testing.assert_array_equal(np.asarray(mesh.get_array()).reshape(20, 20), Hp.T)
            # labels on the outer axes only
            assert ax.get_xlabel() == (s.labels[c] if r == n - 1 else "")
            assert ax.get_ylabel() == (s.labels[r] if c == 0 and r > 0 else "")
    plt.close("all")


def test_save_diagnostic_plots_writes_the_corner_figure(cfg3_run, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    import naima_amd as na
    out = str(tmp_path / "run")
    with pytest.warns(UserWarning, match="corner"):
        na.save_diagnostic_plots(out, cfg3_run)
    assert os.path.getsize(out + "_corner.png") > 0
    plt.close("all")


def test_plot_chain_s_posterior_panel_is_the_device_s(cfg3_run):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    import naima_amd as na
    from naima_amd import posterior as P
    s = cfg3_run
    dist = np.asarray(s.get_chain())[:, :, 0].T.ravel()
    nbins = int(np.clip(np.sqrt(dist.size), 25, 100))
    f = na.plot_chain(s, 0)
    ax = f.axes[1]
    (st,) = _stairs(ax)
    want, edges = np.histogram(dist, bins=nbins, density=True)
    np.testing.assert_array_equal(st.get_data().edges, edges)
    np.testing.assert_allclose(st.get_data().values, want, rtol=1e-12, atol=0)
    (kde,) = [ln for ln in ax.lines if ln.get_label() == "KDE"]
    np.testing.assert_array_equal(kde.get_xdata(), edges)
    np.testing.assert_array_equal(kde.get_ydata(), P.gaussian_kde(dist, edges)[0])
    stats = pytest.importorskip("scipy.stats")
    np.testing.assert_allclose(kde.get_ydata(), stats.gaussian_kde(dist)(edges), rtol=1e-11,
                               atol=1e-300)
    assert ax.get_ylim() == (0, 1.05 * st.get_data().values.max())
    # a scalar blob's distribution goes the same way
    f2 = na.plot_blob(s, 1)
    assert len(_stairs(f2.axes[0])) == 1
    plt.close("all")
