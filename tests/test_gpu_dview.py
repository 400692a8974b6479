"""Every input form of the analysis functions gives the same bits (naima_amd.dview): a host
array, the legacy tuple and a typed view for a chain; a matrix stored with a stride, its padding
NaN, against the contiguous host matrix; bridge sampling from host arrays against a DeviceChain
that carries its log-probabilities."""
import warnings

import numpy as np
import pytest

import rankdiag_np as R

pytestmark = pytest.mark.gpu


def ctx():
    from naima_amd import _lib
    return _lib.get_context()


def same(a, b):
    """bit-identical, NaNs included, through dicts, tuples and arrays"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "fiub":
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return a.shape == b.shape and bool(np.all(a == b))


def floats(v):
    """every float array of a result"""
    if isinstance(v, dict):
        v = list(v.values())
    if isinstance(v, (tuple, list)):
        return [a for x in v for a in floats(x)]
    a = np.asarray(v)
    return [a] if a.dtype.kind == "f" else []


# ---------------------------------------------------------------------------------------
# a chain: host array, legacy tuple, DeviceChain
# ---------------------------------------------------------------------------------------
def chain_forms():
    from naima_amd.dview import as_chain
    x = np.random.default_rng(21).normal(size=(12, 8, 3))
    x[:, 4:] += 0.3                       # (two ensembles that differ a little)
    x[7] = x[6]                           # a repeated row: ties in every pooled column
    block = ctx().array(x.reshape(12, 24))
    return x, {"host": x, "tuple": (block, 12, 8, 3), "view": as_chain((block, 12, 8, 3))}


CHAIN_CALLS = {
    "group_moments": lambda P, c: P.group_moments(c, 2, discard=2, nsplit=2),
    "rhat_moments_split": lambda P, c: P.rhat(c, 2, discard=2),
    "rhat_moments": lambda P, c: P.rhat(c, 2, discard=2, split=False),
    "rhat_rank_split": lambda P, c: P.rhat(c, 2, discard=2, method="rank"),
    "rhat_rank": lambda P, c: P.rhat(c, 2, discard=2, split=False, method="rank"),
    "rank_normalize": lambda P, c: P.rank_normalize(c, 2, discard=2),
    "ess_bulk": lambda P, c: P.ess(c, "bulk", discard=2),
    "ess_tail": lambda P, c: P.ess(c, "tail", discard=2),
    "summary": lambda P, c: P.summary(c, 2, discard=2),
    "covariance": lambda P, c: P.covariance(c, discard=2),
}


@pytest.mark.parametrize("name", sorted(CHAIN_CALLS))
def test_chain_forms_agree_to_the_bit(name):
    from naima_amd import posterior as P
    x, forms = chain_forms()
    got = {k: CHAIN_CALLS[name](P, v) for k, v in forms.items()}
    assert same(got["host"], got["tuple"]), (name, got["host"], got["tuple"])
    assert same(got["host"], got["view"]), (name, got["host"], got["view"])
    if name != "ess_tail":   # (ten rows: a walker that never went below q05 makes that one NaN)
        first = floats(got["host"])[0]
        assert np.all(np.isfinite(first)), (name, first)


def test_a_device_chain_is_ranked_as_the_host_chain_is():
    """``rank_columns`` of a DeviceChain: every parameter over all walkers and rows, the result in
    the chain's shape -- not the matrix [rows][nwalkers * ndim] its memory also is"""
    from naima_amd import posterior as P
    x, forms = chain_forms()
    want = P.rank_columns(x, discard=2)
    got = P.rank_columns(forms["view"], discard=2)
    assert got.shape == (10, 8, 3) and got.tobytes() == want.tobytes()
    assert np.array_equal(got, R.pooled_ranks(x[2:]))
    as_matrix = P.rank_columns((forms["tuple"][0], 12, 24, 24), discard=2)   # the tuple's reading
    assert as_matrix.shape == (10, 24) and as_matrix.max() == 10.0
    z = P.rank_normalize(forms["view"].behind(2), 2)   # a sub-view is the chain behind discard
    assert z.tobytes() == P.rank_normalize(x, 2, discard=2).tobytes()


# ---------------------------------------------------------------------------------------
# a matrix with a stride, its padding NaN
# ---------------------------------------------------------------------------------------
def matrix_forms():
    from naima_amd.dview import as_matrix
    m = np.random.default_rng(22).normal(size=(40, 3))
    m[5] = m[4]
    pad = np.full((40, 5), np.nan)
    pad[:, :3] = m
    block = ctx().array(pad)
    return m, {"tuple": (block, 40, 3, 5), "view": as_matrix((block, 40, 3, 5))}


MATRIX_CALLS = {
    "column_stats": lambda P, IC, PR, s: P.column_stats(s),
    "histogram": lambda P, IC, PR, s: P.histogram(s, bins=7),
    "histogram_pairs": lambda P, IC, PR, s: P.histogram_pairs(s, bins=5),
    "gaussian_kde": lambda P, IC, PR, s: P.gaussian_kde(s, np.linspace(-2.0, 2.0, 9)),
    "rank_columns": lambda P, IC, PR, s: P.rank_columns(s, discard=2),
    "waic": lambda P, IC, PR, s: IC.waic(s),
    "loo": lambda P, IC, PR, s: IC.loo(s),
    "predictive_quantiles": lambda P, IC, PR, s: PR.predictive_quantiles(s, [0.05, 0.5, 0.95]),
}


@pytest.mark.parametrize("name", sorted(MATRIX_CALLS))
def test_strided_matrix_equals_the_contiguous_host_matrix(name):
    from naima_amd import infocrit as IC, posterior as P, predictive as PR
    m, forms = matrix_forms()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (loo: Pareto k of 40 rows)
        want = MATRIX_CALLS[name](P, IC, PR, m)
        got = {k: MATRIX_CALLS[name](P, IC, PR, v) for k, v in forms.items()}
    for k, v in got.items():   # (a view that used the wrong stride has read a NaN)
        assert same(want, v), (name, k, want, v)
    assert not any(np.any(np.isnan(a)) for a in floats(want)), want


def test_strided_matrix_covariance_and_scores():
    """``covariance`` and ``rank_normalize`` read a tuple as a chain: the strided matrix goes to
    them as a DeviceMatrix, and stays a matrix"""
    from naima_amd import posterior as P
    m, forms = matrix_forms()
    want, got = P.covariance(m, discard=2), P.covariance(forms["view"], discard=2)
    assert same(want, got) and np.all(np.isfinite(got[1]))
    np.testing.assert_allclose(got[1], np.cov(m[2:], rowvar=False), rtol=1e-9, atol=1e-12)
    z = P.rank_normalize(forms["view"], discard=2)
    assert z.shape == (38, 3) and z.tobytes() == P.rank_normalize(m, discard=2).tobytes()
    sub = forms["view"].rows(2, 40)
    assert same(P.column_stats(sub), P.column_stats(m[2:]))
    assert sub.get().tobytes() == m[2:].tobytes()


# ---------------------------------------------------------------------------------------
# bridge sampling: host arrays against a DeviceChain with logp
# ---------------------------------------------------------------------------------------
def lnp(theta):
    return -0.5 * np.sum(np.atleast_2d(theta) ** 2, axis=1)


def gaussian_chain():
    """a Metropolis chain (40, 8, 2) of a standard normal that starts at the mode"""
    rng = np.random.default_rng(11)
    c = np.zeros((40, 8, 2))
    c[0] = 0.01 * rng.normal(size=(8, 2))
    for t in range(1, 40):
        prop = c[t - 1] + 0.8 * rng.normal(size=(8, 2))
        acc = np.log(rng.uniform(size=8)) < lnp(prop) - lnp(c[t - 1])
        c[t] = np.where(acc[:, None], prop, c[t - 1])
    return c, lnp(c.reshape(-1, 2)).reshape(40, 8)


def test_bridge_sampling_from_a_device_chain_with_logp():
    from naima_amd import evidence as EV
    from naima_amd.dview import as_chain
    c, lp = gaussian_chain()
    want = EV.bridge_sampling(c, lp, lnp, seed=5, discard=2)
    assert want["converged"] and np.isfinite(want["logz"]) and want["n_post"] == 19 * 8
    block, lblock = ctx().array(c.reshape(40, 16)), ctx().array(lp)
    view = as_chain((block, 40, 8, 2), logp=lblock.get())       # logp uploaded with the chain
    got = EV.bridge_sampling(view, None, lnp, seed=5, discard=2)
    assert same(want, got), (want, got)
    for log_prob in (lblock, (lblock, 40, 8)):                     # the documented legacy forms
        assert same(want, EV.bridge_sampling((block, 40, 8, 2), log_prob, lnp, seed=5, discard=2))
    # a view behind two rows is the chain with discard=2
    assert same(want, EV.bridge_sampling(view.behind(2), None, lnp, seed=5))
    with pytest.raises(ValueError, match="both be host arrays or both device blocks"):
        EV.bridge_sampling(view, lp, lnp)
    with pytest.raises(ValueError, match="both be host arrays or both device blocks"):
        EV.bridge_sampling(c, lblock, lnp)
