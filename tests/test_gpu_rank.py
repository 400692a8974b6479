"""Ranking whole pooled columns on the GPU (nh_rank_columns, nh_rank_normal_scores,
nh_rank_transform) and the statistics built on it -- posterior.rank_columns / rank_normalize,
rhat(method="rank"), ess, summary and their sampler surface -- against the NumPy / SciPy
restatement of tests/rankdiag_np.py.

Ranks are compared EXACTLY with scipy.stats.rankdata at the smallest shapes at which each part of
the sort can go wrong: one and two rows, the edges of a wave (64) and of a chunk of the scatter
(256), several workgroups per column (a tile is 4096 rows) with ld > ncol, tie runs across tile
boundaries, and the values that exercise the key: negatives, subnormals, the two zeros, a
difference in the lowest mantissa bit (the first radix digit) and in the sign bit (the last)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.special import ndtri
from scipy.stats import rankdata

import rankdiag_np as R
from test_ensembles_host import rhat_numpy

pytestmark = pytest.mark.gpu

# relative tolerances of the suites these statistics are built on: posterior.rhat against NumPy
# (tests/test_gpu_ensembles.py) and integrated_time against the restatement
# (tests/test_gpu_autocorr.py, TAU_RTOL)
RHAT_RTOL = 1e-9
TAU_RTOL = 1e-9

# the largest relative error of nh_rank_normal_scores against scipy.special.ndtri over
# ``score_arguments()``, measured on an MI355X (profiles/NOTES_rank.md); the test asserts four
# times this, which leaves room for contraction differences between builds.  Above 1e-13 it would
# be a defect of the approximation, not a tolerance.
NDTRI_MEASURED = 1.03e-15


@pytest.fixture(scope="module")
def P():
    from naima_amd import _lib, posterior
    _lib.get_context()
    return posterior


def ranks_np(x):
    """rankdata of every column; NaN throughout for a column with a non-finite value"""
    x = np.asarray(x, dtype=float)
    out = np.empty(x.shape)
    for c in range(x.shape[1]):
        out[:, c] = rankdata(x[:, c], method="average") if np.all(np.isfinite(x[:, c])) else np.nan
    return out


# ---------------------------------------------------------------------------------------
# ranks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 257])
def test_ranks_at_wave_and_chunk_edges(P, M):
    rng = np.random.default_rng(M)
    x = np.stack([rng.standard_normal(M), np.round(rng.standard_normal(M), 1)], axis=1)
    assert_array_equal(P.rank_columns(x), ranks_np(x))
    assert_array_equal(P.rank_columns(x[:, 1]), ranks_np(x[:, 1:]))


def test_ranks_over_several_workgroups_with_padding(P):
    """70 001 rows are 18 tiles: the scan across workgroups; ld = 5 > ncol = 3.  Column 1 has 40
    distinct values (tie runs of ~1750 rows across tile boundaries), column 2 short runs"""
    from naima_amd import _lib
    M, ncol, ld = 70001, 3, 5
    rng = np.random.default_rng(70001)
    x = rng.standard_normal((M, ld))
    x[:, 1] = rng.integers(0, 40, M)
    x[:, 2] = np.round(x[:, 2], 2)
    x[:, 3:] = np.nan  # (padding: never read)
    ctx = _lib.get_context()
    got = P.rank_columns((ctx.array(x), M, ncol, ld))
    assert got.shape == (M, ncol)
    assert_array_equal(got, ranks_np(x[:, :ncol]))


def test_ranks_of_constant_and_long_runs(P):
    M = 2 * 4096 + 100
    rng = np.random.default_rng(9)
    x = np.empty((M, 3))
    x[:, 0] = 4.25                                   # constant: one run over three tiles
    x[:, 1] = rng.permutation(np.arange(M) // 1000)  # runs of 1000 that straddle the tiles
    x[:, 2] = np.arange(M) // 3                      # sorted already, runs of three
    want = ranks_np(x)
    assert np.all(want[:, 0] == (M + 1) / 2)
    assert_array_equal(P.rank_columns(x), want)


def test_ranks_of_values_that_exercise_the_key(P):
    up = np.nextafter
    col = np.array([1.0, up(1.0, 2.0), -1.0, 1.0, 5e-324, -5e-324, 0.0, -0.0, 1.1e-308, -1.1e-308,
                    -3.5, 3.5, 1e308, -1e308, up(1.0, 2.0), -0.0, up(1.0, 0.0), -up(1.0, 2.0),
                    2.0 ** -1074 * 3, -2.5, 2.5, up(-2.5, 0.0)])
    x = np.stack([col, -col, np.abs(col)], axis=1)
    want = ranks_np(x)
    zeros = np.flatnonzero(col == 0.0)
    assert len(set(want[zeros, 0])) == 1  # (-0.0 and +0.0 tie in the reference)
    assert_array_equal(P.rank_columns(x), want)
    rng = np.random.default_rng(1)
    big = np.concatenate([col] * 30)
    big = np.stack([rng.permutation(big), rng.permutation(big)], axis=1)
    assert_array_equal(P.rank_columns(big), ranks_np(big))


def test_a_non_finite_value_voids_its_column_only(P):
    from naima_amd import _lib
    M = 300
    x = np.random.default_rng(5).standard_normal((M, 5))
    x[17, 1] = np.nan
    x[250, 3] = np.inf
    x[3, 4], x[4, 4], x[5, 4] = -np.inf, np.nan, np.nan
    got = P.rank_columns(x)
    want = ranks_np(x)
    assert np.all(np.isnan(want[:, [1, 3, 4]])) and np.all(np.isfinite(want[:, [0, 2]]))
    assert_array_equal(got, want)
    ctx = _lib.get_context()
    r, status = ctx.empty((M, 5)), ctx.empty((5,), np.int32)
    ctx.call("nh_rank_columns", ctx.array(x), 0, M, 5, 0, 1, 5, r, status)
    assert status.get().tolist() == [0, 1, 0, 1, 3]
    z = P.rank_normalize(x)
    assert np.all(np.isnan(z[:, [1, 3, 4]])) and np.all(np.isfinite(z[:, [0, 2]]))


def test_columns_ranked_in_groups_are_the_same(P, monkeypatch):
    """a scratch budget below one column's 16 S bytes: one column per group"""
    x = np.round(np.random.default_rng(8).standard_normal((5000, 3)), 2)
    whole = P.rank_columns(x)
    monkeypatch.setenv("NAIMA_AMD_RANK_SCRATCH_KIB", "64")
    assert_array_equal(P.rank_columns(x), whole)
    assert_array_equal(whole, ranks_np(x))


def test_rank_arguments(P):
    from naima_amd import _lib
    ctx = _lib.get_context()
    x, r, st = ctx.array(np.zeros((6, 8))), ctx.empty((12, 4)), ctx.empty((4,), np.int32)
    ok = [x, 0, 6, 8, 4, 2, 4, r, st]
    ctx.call("nh_rank_columns", *ok)
    for i, v in ((1, -1), (2, 0), (5, 0), (6, 0), (4, 3), (4, 5), (3, 7), (2, 1 << 30)):
        bad = list(ok)
        bad[i] = v
        with pytest.raises(_lib.NaimaHipError, match="nh_rank_columns"):
            ctx.call("nh_rank_columns", *bad)
    with pytest.raises(_lib.NaimaHipError, match="layout"):
        ctx.call("nh_rank_normal_scores", r, 6, 2, 4, 7, 8, 4, r)
    with pytest.raises(_lib.NaimaHipError, match="mode"):
        ctx.call("nh_rank_transform", x, 0, 6, 8, 4, 2, 4, ctx.array(np.zeros(4)), 2, r, 8)


# ---------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------
def test_pooling_a_chain_behind_discard(P):
    from naima_amd import _lib
    rng = np.random.default_rng(78)
    chain = np.round(rng.standard_normal((7, 8, 3)), 1)  # (ties)
    want = R.pooled_ranks(chain, discard=2)
    for d in range(3):
        assert_array_equal(want[:, :, d].ravel(), rankdata(chain[2:, :, d].ravel()))
    got = P.rank_columns(chain, discard=2)
    assert got.shape == (5, 8, 3)
    assert_array_equal(got, want)
    # the scores scattered back to the chain's layout, from a host array and from a device block
    z = P.rank_normalize(chain, ensembles=2, discard=2)
    assert z.shape == (5, 8, 3)
    assert_array_equal(rankdata(z[:, :, 1].ravel()), rankdata(chain[2:, :, 1].ravel()))
    ctx = _lib.get_context()
    block = (ctx.array(chain.reshape(7, 24)), 7, 8, 3)
    assert_array_equal(P.rank_normalize(block, ensembles=2, discard=2), z)
    dev, rows, nw, ndim = P.rank_normalize(block, ensembles=2, discard=2, device=True)
    assert (rows, nw, ndim) == (5, 8, 3)
    assert_array_equal(dev.get().reshape(5, 8, 3), z)
    # the pooled layout [S][ncolp] of the entry point is the same memory order
    r, st = ctx.empty((40, 3)), ctx.empty((3,), np.int32)
    ctx.call("nh_rank_columns", block[0], 2, 5, 24, 3, 8, 3, r, st)
    zp = ctx.empty((40, 3))
    ctx.call("nh_rank_normal_scores", r, 5, 8, 3, _lib.NH_RANK_POOLED, 0, 0, zp)
    assert_array_equal(zp.get().reshape(5, 8, 3), z)


# ---------------------------------------------------------------------------------------
# normal scores
# ---------------------------------------------------------------------------------------
def score_arguments():
    """[(ranks, S)]: every rank and half-rank of small S, both ends of S = 2**20, and the ranks of
    the shapes above"""
    out = []
    for S in (1, 2, 5, 63, 64, 65, 255, 257):
        out.append((np.arange(2, 2 * S + 1) / 2.0, S))
    S = 1 << 20
    lo = np.arange(2, 4097) / 2.0
    out.append((np.concatenate([lo, S + 1 - lo]), S))
    rng = np.random.default_rng(70001)
    out.append((rankdata(rng.integers(0, 40, 70001)), 70001))
    out.append((rng.permutation(70001) + 1.0, 70001))
    return out


def normal_scores(r, S):
    """nh_rank_normal_scores of the ranks r as part of a column of S values"""
    from naima_amd import _lib
    ctx = _lib.get_context()
    out = []
    for a in range(0, len(r), S):  # (S decides the denominator: at most S ranks a call)
        full = np.full(S, 1.0)
        part = r[a:a + S]
        full[:len(part)] = part
        z = ctx.empty((S, 1))
        ctx.call("nh_rank_normal_scores", ctx.array(full.reshape(S, 1)), S, 1, 1,
                 _lib.NH_RANK_POOLED, 0, 0, z)
        out.append(z.get()[:len(part), 0])
    return np.concatenate(out)


def ndtri_error():
    """the largest relative error against scipy.special.ndtri over score_arguments()"""
    worst = 0.0
    for r, S in score_arguments():
        z, want = normal_scores(r, S), R.scores(r, S)
        zero = want == 0.0
        assert np.all(z[zero] == 0.0) and np.all(np.isfinite(z))
        if not np.all(zero):
            worst = max(worst, float(np.max(np.abs(z[~zero] - want[~zero]) / np.abs(want[~zero]))))
    return worst


def test_normal_scores_against_ndtri(P):
    err = ndtri_error()
    print("nh_rank_normal_scores against ndtri: largest relative error %.3e" % err)
    assert NDTRI_MEASURED <= 1e-13
    assert err <= 4 * NDTRI_MEASURED
    z = normal_scores(np.array([np.nan, 1.0]), 2)
    assert np.isnan(z[0]) and z[1] == normal_scores(np.array([1.0]), 2)[0]
    assert_allclose(z[1], ndtri(0.625 / 2.25), rtol=4 * NDTRI_MEASURED)


def test_two_calls_give_the_same_bits(P):
    x = np.round(np.random.default_rng(4).standard_normal((9001, 4, 2)), 2)
    a, b = P.rank_normalize(x), P.rank_normalize(x)
    assert a.tobytes() == b.tobytes()
    assert P.rank_columns(x).tobytes() == P.rank_columns(x).tobytes()


# ---------------------------------------------------------------------------------------
# R-hat
# ---------------------------------------------------------------------------------------
_CHAINS = {}


def _chain(name):
    if name not in _CHAINS:
        if name == "heavy":
            _CHAINS[name] = (R.case_heavy_tails(), 2)
        elif name == "scales":
            _CHAINS[name] = (R.case_scales(), 2)
        else:
            rng = np.random.default_rng(40)
            x = np.round(rng.standard_normal((40, 12, 3)), 2) + 0.2 * np.arange(3).repeat(4)[None, :, None]
            _CHAINS[name] = (x, 3)
    return _CHAINS[name]


@pytest.mark.parametrize("name", ["heavy", "scales", "seeded"])
def test_rank_rhat_against_the_restatement(P, name):
    x, k = _chain(name)
    for split in (True, False):
        for folded in (True, False):
            got = P.rhat(x, k, split=split, method="rank", folded=folded)
            want = R.rhat_rank(x, k, split=split, folded=folded)
            print(name, "split", split, "folded", folded, got, want)
            assert_allclose(got, want, rtol=RHAT_RTOL, atol=0)
    assert_allclose(P.rhat(x, k, discard=3, method="rank"), R.rhat_rank(x, k, discard=3),
                    rtol=RHAT_RTOL, atol=0)


def test_rank_rhat_is_right_where_moments_are_not(P):
    x, k = _chain("heavy")
    with np.errstate(all="ignore"):
        mom = P.rhat(x, k)
    rank = P.rhat(x, k, method="rank")
    assert not np.isfinite(mom[0]) or mom[0] > 1.1
    assert rank[0] < 1.01
    x, k = _chain("scales")
    assert P.rhat(x, k)[0] < 1.01
    assert P.rhat(x, k, method="rank")[0] > 1.01
    assert_array_equal(P.rhat(x, k), P.rhat(x, k, method="moments"))
    assert_allclose(P.rhat(x, k), rhat_numpy(x, k), rtol=RHAT_RTOL, atol=0)


# ---------------------------------------------------------------------------------------
# effective sample sizes and the summary
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ar_chain():
    """AR(1), phi = 0.5 and 0.8, 16 walkers; every third row repeats the one before (a rejected
    move of every walker): 400 rows"""
    from test_autocorr_host import ar1
    x = ar1(np.random.default_rng(16), 300, 16, [0.5, 0.8])
    keep = np.sort(np.concatenate([np.arange(300), np.arange(0, 300, 3)]))
    return x[keep]


def test_ess_against_the_restatement(P, ar_chain):
    assert ar_chain.shape == (400, 16, 2)
    for kind in ("bulk", "tail"):
        got, want = P.ess(ar_chain, kind), R.ess(ar_chain, kind)
        print("ess", kind, got, want)
        assert np.all(np.isfinite(want)) and np.all(want > 100) and np.all(want < 6400)
        assert_allclose(got, want, rtol=TAU_RTOL, atol=0)
    assert_allclose(P.ess(ar_chain, "bulk", discard=50, c=4), R.ess(ar_chain, "bulk", 50, 4),
                    rtol=TAU_RTOL, atol=0)
    from naima_amd import _lib
    block = (_lib.get_context().array(ar_chain.reshape(400, 32)), 400, 16, 2)
    assert_array_equal(P.ess(block, "tail", discard=50), P.ess(ar_chain, "tail", discard=50))


def test_ess_of_a_chain_too_short_is_nan(P, ar_chain):
    for kind in ("bulk", "tail"):
        assert np.all(np.isnan(P.ess(ar_chain[:1], kind)))
        assert np.all(np.isnan(R.ess(ar_chain[:1], kind)))
    x = ar_chain.copy()
    x[7, 3, 1] = np.nan
    got = P.ess(x, "bulk")
    assert np.isfinite(got[0]) and np.isnan(got[1])


def test_summary(P, ar_chain):
    x = ar_chain
    flat = x.reshape(-1, 2)
    s = P.summary(x, ensembles=2, discard=0, labels=["a", "b"])
    assert set(s) == {"mean", "sd", "median", "q16", "q84", "ess_bulk", "ess_tail", "tau", "rhat",
                      "rhat_rank", "labels"}
    assert set(P.summary(x)) == {"mean", "sd", "median", "q16", "q84", "ess_bulk", "ess_tail", "tau"}
    assert all(np.shape(s[k]) == (2,) for k in s)
    assert_array_equal(s["rhat"], P.rhat(x, 2))
    assert_array_equal(s["rhat_rank"], P.rhat(x, 2, method="rank"))
    assert_array_equal(s["ess_bulk"], P.ess(x, "bulk"))
    assert_array_equal(s["ess_tail"], P.ess(x, "tail"))
    # np.quantile interpolates between the same two order statistics by another, equally rounded
    # expression: a few ulp of the larger of the two
    q = np.quantile(flat, [0.16, 0.5, 0.84], axis=0)
    tol = 4 * np.finfo(float).eps * np.abs(flat).max()
    for key, want in zip(("q16", "median", "q84"), q):
        assert_allclose(s[key], want, rtol=0, atol=tol)
    assert_allclose(s["mean"], flat.mean(axis=0), rtol=1e-12, atol=1e-14)
    assert_allclose(s["sd"], flat.std(axis=0, ddof=1), rtol=1e-12)
    assert_allclose(s["tau"], R.tau(x), rtol=TAU_RTOL)
    s5 = P.summary(x, ensembles=2, discard=5)
    assert_array_equal(s5["rhat"], P.rhat(x, 2, discard=5))
    assert_array_equal(s5["ess_tail"], P.ess(x, "tail", discard=5))


# ---------------------------------------------------------------------------------------
# the sampler, a saved run and the results table
# ---------------------------------------------------------------------------------------
# cfg1, two ensembles of 8 walkers from the same 0.3 % ball, a check every 20 rows; tol = 3 and
# rtol = 1 let tau pass from the second check on (tests/test_gpu_ensembles.py); the rank R-hat of
# such a run lies far below 1.5 once both halves of both ensembles overlap
def _fit(na):
    from bench import build_problem
    from naima_amd.sampler import EnsembleSampler
    model, p0, raw, data, prior, labels = build_problem("cfg1", na)
    nw, nd, seed = 16, p0.size, 31
    s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=seed, naima_style=True,
                        store_blobs=True, device=True, nan_policy="reject", ensembles=2)
    s.labels = ["norm", "index", "log10(cutoff)"]
    s.run_info = {"ensembles": 2, "seeds": list(s.seeds)}
    s.data = None
    pos = p0 * (1 + 0.003 * np.random.default_rng(seed).standard_normal((nw, nd)))
    return s, pos


def test_sampler_surface(P, tmp_path):
    import naima_amd as na
    s, pos = _fit(na)
    with np.errstate(all="ignore"):
        s.run_until_converged(pos, max_steps=200, check_every=20, tol=3, rtol=1.0, rhat=1.5,
                              rhat_method="rank")
    conv = s.convergence
    print("rank R-hat of the checks:", [(r, np.round(h, 3)) for r, _, h in conv["history"]])
    assert conv["rhat_method"] == "rank" and conv["where"] == "device"
    assert conv["converged"] and conv["rows"] < 200 and s.iteration == conv["rows"]
    assert np.all(conv["rhat"] < 1.5)
    # the whole chain still lies in the history block in HBM: the accessors read it there
    assert s._chain_block() is not None and len(s._chain) == 0
    rh, rh4 = s.get_rhat(method="rank"), s.get_rhat(discard=4, split=False, method="rank")
    eb, et3 = s.get_ess(), s.get_ess(kind="tail", discard=3)
    sm, sm5 = s.get_summary(), s.get_summary(discard=5)
    assert s._chain_block() is not None
    chain = s.get_chain()
    assert s._chain_block() is None and chain.shape == (conv["rows"], 16, 3)
    # the statistic of the check, taken in HBM, is the statistic of the stored chain
    assert_allclose(conv["rhat"], P.rhat(chain, 2, method="rank"), rtol=RHAT_RTOL, atol=0)
    # ... and what the accessors read in HBM is what they give for the chain on the host
    assert_array_equal(rh, P.rhat(chain, 2, method="rank"))
    assert_array_equal(rh4, P.rhat(chain, 2, discard=4, split=False, method="rank"))
    assert_array_equal(eb, P.ess(chain, "bulk"))
    assert_array_equal(et3, P.ess(chain, "tail", discard=3))
    assert_array_equal(s.get_rhat(method="rank"), rh)
    assert_array_equal(s.get_rhat(), P.rhat(chain, 2))
    assert_array_equal(s.get_rhat(discard=4, split=False, method="rank"), rh4)
    assert_array_equal(s.get_ess(), eb)
    assert_array_equal(s.get_ess(kind="tail", discard=3, thin=2), P.ess(chain[3::2], "tail"))
    for got, want in ((sm, P.summary(chain, 2, labels=s.labels)),
                      (sm5, P.summary(chain, 2, discard=5, labels=s.labels)),
                      (s.get_summary(), sm), (s.get_summary(discard=5), sm5)):
        assert set(got) == set(want)
        for key in want:
            assert_array_equal(got[key], want[key])
    back = na.read_run(na.save_run(str(tmp_path / "run"), s))
    sb = back.get_summary()
    assert set(sb) == set(sm)
    for key in sm:
        assert_array_equal(sb[key], sm[key])
    assert_array_equal(back.get_ess(kind="tail"), s.get_ess(kind="tail"))

    plain = na.save_results_table(str(tmp_path / "plain"), s, include_blobs=False)
    assert list(plain["meta"]) == ["n_samples", "ML_pars", "MaxLogLikelihood", "ensembles", "seeds"]
    diag = na.save_results_table(str(tmp_path / "diag"), s, include_blobs=False, diagnostics=True)
    assert list(diag["meta"]) == ["n_samples", "ML_pars", "MaxLogLikelihood", "ESS_bulk", "ESS_tail",
                                  "Rhat_rank", "ensembles", "seeds"]
    assert_array_equal(diag["meta"]["ESS_bulk"], sm["ess_bulk"])
    assert_array_equal(diag["meta"]["ESS_tail"], sm["ess_tail"])
    assert_array_equal(diag["meta"]["Rhat_rank"], sm["rhat_rank"])
    for key in ("label", "median", "unc_lo", "unc_hi"):
        assert_array_equal(diag[key], plain[key])
    text = open(str(tmp_path / "diag_results.ecsv")).read()
    assert "ESS_bulk" in text and "Rhat_rank" in text
    assert "ESS_bulk" not in open(str(tmp_path / "plain_results.ecsv")).read()
