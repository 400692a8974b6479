"""The rank-normalised statistics without a GPU: argument errors come before any device work,
``method="moments"`` is the R-hat it always was, and the NumPy / SciPy restatement the GPU tests
compare with (tests/rankdiag_np.py) has the properties that make the comparison meaningful."""
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

import rankdiag_np as R
from test_ensembles_host import gauss, rhat_numpy

from naima_amd.sampler import EnsembleSampler


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to make a GPU context fails the test"""
    from naima_amd import _lib

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_lib, "get_context", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_import_creates_no_gpu_context():
    code = ("import naima_amd.posterior as P, naima_amd._lib as L; "
            "assert L._lib is None and not L._default, 'GPU touched'; "
            "assert P.rank_columns and P.rank_normalize and P.ess and P.summary; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_new_names_are_exported():
    from naima_amd import _lib, posterior
    for name in ("rank_columns", "rank_normalize", "ess", "summary"):
        assert name in posterior.__all__
    for name in ("nh_rank_columns", "nh_rank_normal_scores", "nh_rank_transform"):
        assert name in _lib.EXPORTS


def test_argument_errors_come_before_device_work(no_device):
    from naima_amd import posterior as P
    x = np.zeros((10, 12, 2))
    with pytest.raises(ValueError, match="method must be"):
        P.rhat(x, 2, method="ranks")
    with pytest.raises(ValueError, match="do not split"):
        P.rhat(x, 5, method="rank")
    with pytest.raises(ValueError, match="two at least"):
        P.rhat(x, 2, discard=7, method="rank")  # three rows behind it: split needs four
    with pytest.raises(ValueError, match="at least 2"):
        P.rhat(x, 1, method="rank")
    with pytest.raises(ValueError, match="kind must be"):
        P.ess(x, kind="middle")
    with pytest.raises(ValueError, match="needed at least"):
        P.ess(x, discard=10)
    with pytest.raises(ValueError, match="rows, nwalkers, ndim"):
        P.ess(x[0])
    with pytest.raises(ValueError, match="do not split"):
        P.rank_normalize(x, ensembles=5)
    with pytest.raises(ValueError, match="needed at least"):
        P.rank_normalize(x, discard=10)
    with pytest.raises(ValueError, match="behind discard"):
        P.rank_columns(np.zeros((4, 2)), discard=4)
    with pytest.raises(ValueError, match="do not split"):
        P.summary(x, ensembles=5)
    with pytest.raises(ValueError, match="two at least"):
        P.summary(x, ensembles=2, discard=7)
    with pytest.raises(ValueError, match="labels"):
        P.summary(x, labels=["a"])
    s = EnsembleSampler(16, 2, gauss, ensembles=2)
    with pytest.raises(ValueError, match="method must be"):
        s.get_rhat(method="rnk")
    with pytest.raises(ValueError, match="kind must be"):
        s.get_ess(kind="both")
    with pytest.raises(ValueError, match="method must be"):
        s.run_until_converged(np.zeros((16, 2)), 10, rhat=1.01, rhat_method="rnk")
    with pytest.raises(ValueError, match="ensembles >= 2"):
        EnsembleSampler(16, 2, gauss).get_rhat(method="rank")


def test_method_moments_is_the_rhat_it_was(monkeypatch):
    """``rhat(x, k)`` and ``rhat(x, k, method="moments")`` go through ``group_moments`` with the
    arguments they always went with and apply ``rhat_from_moments``: with the device's moments
    replaced by NumPy's on a seeded chain, both are the restatement's R-hat"""
    from naima_amd import posterior as P
    from test_ensembles_host import sequences_numpy
    rng = np.random.default_rng(12)
    x = rng.normal(size=(31, 12, 3)) + 0.3 * np.arange(3).repeat(4)[None, :, None]
    calls = []

    def moments(chain, ensembles, discard=0, nsplit=1):
        calls.append((ensembles, discard, nsplit))
        seq = sequences_numpy(chain, ensembles, discard, nsplit == 2)
        shape = (nsplit, ensembles, chain.shape[2])
        return dict(n=np.full(shape, seq.shape[1]), mean=seq.mean(axis=1).reshape(shape),
                    var=seq.var(axis=1, ddof=1).reshape(shape), draws=seq.shape[1])
    monkeypatch.setattr(P, "group_moments", moments)
    for split in (True, False):
        want = rhat_numpy(x, 3, 4, split)
        a = P.rhat(x, 3, 4, split)
        b = P.rhat(x, 3, discard=4, split=split, method="moments")
        assert np.array_equal(a, b)
        assert_allclose(a, want, rtol=1e-13)
    assert calls == [(3, 4, 2), (3, 4, 2), (3, 4, 1), (3, 4, 1)]


def test_restatement_ranks_and_scores():
    x = np.array([3.0, 1.0, 3.0, -0.0, 0.0, 2.0]).reshape(3, 2, 1)
    assert np.array_equal(R.pooled_ranks(x)[:, :, 0], [[5.5, 3.0], [5.5, 1.5], [1.5, 4.0]])
    z = R.rank_normalize(x)
    assert z.shape == x.shape and z[0, 0, 0] == z[1, 0, 0] and z[1, 1, 0] == z[2, 0, 0]
    assert_allclose(R.scores([1, 2, 3], 3), [-R.scores(3, 3), 0.0, R.scores(3, 3)], atol=1e-16)
    x[1, 1, 0] = np.nan
    assert np.all(np.isnan(R.rank_normalize(x)))


def test_rank_rhat_ignores_heavy_tails_where_moments_fail():
    """(a) of tests/rankdiag_np.py; the seed is fixed so that the restatement satisfies this here,
    on the CPU"""
    x = R.case_heavy_tails()
    with np.errstate(all="ignore"):
        mom = rhat_numpy(x, 2)
    rank = R.rhat_rank(x, 2)
    print("heavy tails: moments", mom, "rank", rank)
    assert not np.isfinite(mom[0]) or mom[0] > 1.1
    assert rank[0] < 1.01


def test_folded_rank_rhat_sees_a_difference_in_scale():
    """(b) of tests/rankdiag_np.py; the seed is fixed so that the restatement satisfies this here,
    on the CPU"""
    x = R.case_scales()
    mom, rank = rhat_numpy(x, 2), R.rhat_rank(x, 2)
    print("scales 1 and 3: moments", mom, "rank, folded", rank,
          "not folded", R.rhat_rank(x, 2, folded=False))
    assert mom[0] < 1.01
    assert rank[0] > 1.01


def test_restatement_ess_of_independent_draws_is_about_their_number():
    x = np.random.default_rng(3).standard_normal((400, 16, 2))
    S = 400 * 16
    for kind in ("bulk", "tail"):
        e = R.ess(x, kind)
        assert np.all(e > 0.6 * S) and np.all(e < 1.6 * S), (kind, e)
    assert np.all(np.isnan(R.ess(x[:1], "bulk")))
