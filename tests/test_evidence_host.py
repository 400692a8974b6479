"""The host side of naima_amd.evidence (no GPU needed): the NumPy restatement of the kernels and
of bridge sampling (tests/evidence_np.py) against closed-form evidences with independent draws,
the overflow-safe forms of the iteration's terms, the proposal stream, the argument errors that
come before any device work, and the declarations of the entry points."""
import math
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

import evidence_np as E  # noqa: E402
import predictive_np as R  # noqa: E402

NAMES = ("nh_chain_cov", "nh_mvn_draw", "nh_mvn_logpdf", "nh_bridge_l2", "nh_bridge_sums")
N = 4096  # posterior draws in each half, and proposals
SEEDS = (1, 2, 3)


# ---------------------------------------------------------------------------------------
# targets with a known evidence: (2 N independent posterior draws, lnprob, log Z)
# ---------------------------------------------------------------------------------------
def gaussian(d, seed):
    rng = np.random.default_rng(100 + d)
    A = rng.normal(size=(d, d))
    cov = A @ A.T + d * np.eye(d)
    m, c = rng.normal(size=d), 1.7
    P = np.linalg.inv(cov)

    def fn(t):
        return c - 0.5 * np.einsum("ni,ij,nj->n", t - m, P, t - m)

    x = m + np.random.default_rng(seed).normal(size=(2 * N, d)) @ np.linalg.cholesky(cov).T
    return x, fn, c + 0.5 * d * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(cov)[1]


def banana(b, seed):
    c = -0.3

    def fn(t):
        return c - 0.5 * t[:, 0] ** 2 - 0.5 * (t[:, 1] - b * t[:, 0] ** 2) ** 2

    g = np.random.default_rng(seed)
    t1 = g.normal(size=2 * N)
    return np.stack([t1, b * t1 ** 2 + g.normal(size=2 * N)], 1), fn, c + math.log(2 * math.pi)


BOX = dict(sg=np.array([1.0, 0.5]), m=np.array([0.3, -0.2]), lo=np.array([-0.5, -0.6]),
           hi=np.array([1.5, 0.1]))


def box_lnprob(t):
    b = BOX
    inside = ((t >= b["lo"]) & (t <= b["hi"])).all(axis=1)
    return np.where(inside, -0.5 * (((t - b["m"]) / b["sg"]) ** 2).sum(axis=1), -np.inf)


def box(seed):
    """an unnormalised Gaussian cut by a box prior: Z is a product of erf differences"""
    b = BOX
    x = b["m"] + b["sg"] * np.random.default_rng(seed).normal(size=(60000, 2))
    x = x[np.isfinite(box_lnprob(x))][:2 * N]
    assert len(x) == 2 * N

    def Phi(z):
        return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))

    Z = 1.0
    for i in range(2):
        Z *= b["sg"][i] * math.sqrt(2 * math.pi) * (Phi((b["hi"][i] - b["m"][i]) / b["sg"][i])
                                                    - Phi((b["lo"][i] - b["m"][i]) / b["sg"][i]))
    return x, box_lnprob, math.log(Z)


def estimate(target, seed):
    x, fn, exact = target
    return E.bridge_sampling(x[:N], x[N:], fn(x[N:]), fn, seed=seed), exact


def is_error(l2):
    """the relative standard error of the importance-sampling mean of exp(l2)"""
    w = np.exp(l2 - l2[np.isfinite(l2)].max())
    return w.std(ddof=1) / (w.mean() * math.sqrt(len(w)))


# ---------------------------------------------------------------------------------------
# 1. the estimator against closed forms
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("d", [1, 2, 5])
def test_correlated_gaussian(d, seed):
    o, exact = estimate(gaussian(d, seed), seed)
    print("d=%d seed=%d logz=%.6f exact=%.6f err=%.2g it=%d" % (d, seed, o["logz"], exact,
                                                                  o["logz_err"], o["iterations"]))
    assert o["converged"] and o["iterations"] <= 10
    assert abs(o["logz"] - exact) <= 4 * o["logz_err"]
    assert o["logz_err"] < 0.01  # (a normal proposal fits a normal posterior)
    assert abs(o["logz_is"] - exact) <= 4 * is_error(o["l2"])
    assert o["forbidden_fraction"] == 0.0 and o["n_post"] == N and o["n_draws"] == N


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("b", [0.5, 1.0])
def test_banana(b, seed):
    o, exact = estimate(banana(b, seed), seed)
    print("b=%g seed=%d logz=%.6f exact=%.6f err=%.2g it=%d" % (b, seed, o["logz"], exact,
                                                                 o["logz_err"], o["iterations"]))
    assert o["converged"] and o["iterations"] <= 10
    assert abs(o["logz"] - exact) <= 4 * o["logz_err"]
    assert 0.002 < o["logz_err"] < 0.03
    se = is_error(o["l2"])
    assert se > o["logz_err"]  # (the cross-check scatters more widely)
    assert abs(o["logz_is"] - exact) <= 4 * se


@pytest.mark.parametrize("seed", SEEDS)
def test_gaussian_cut_by_a_box_prior(seed):
    o, exact = estimate(box(seed), seed)
    print("seed=%d logz=%.6f exact=%.6f err=%.2g forbidden=%.3f" % (seed, o["logz"], exact,
                                                                   o["logz_err"],
                                                                   o["forbidden_fraction"]))
    assert o["converged"]
    assert abs(o["logz"] - exact) <= 4 * o["logz_err"]
    assert 0.02 < o["forbidden_fraction"] < 0.5  # (the proposal reaches over the bounds)
    assert np.all(o["l2"][~np.isfinite(o["l2"])] == -np.inf)
    assert abs(o["logz_is"] - exact) <= 4 * is_error(o["l2"])


def test_log_prior_norm_neff_and_n_draws():
    x, fn, exact = banana(0.5, 4)
    a = E.bridge_sampling(x[:N], x[N:], fn(x[N:]), fn, seed=4)
    b = E.bridge_sampling(x[:N], x[N:], fn(x[N:]), fn, seed=4, log_prior_norm=2.5, n_draws=1000,
                          neff=N / 3.0)
    assert b["n_draws"] == 1000 and b["neff"] == N / 3.0
    assert b["s1"] == pytest.approx((N / 3.0) / (N / 3.0 + 1000), rel=1e-15)
    assert abs(b["logz"] + 2.5 - exact) <= 4 * b["logz_err"]
    assert b["logz_err"] > a["logz_err"]  # (fewer draws)
    # an autocorrelated posterior sample inflates its share of the error, and only that
    c = E.bridge_sampling(x[:N], x[N:], fn(x[N:]), fn, seed=4, tau=9.0)
    assert c["logz"] == a["logz"] and c["logz_err"] > a["logz_err"]


# ---------------------------------------------------------------------------------------
# 2. the terms of the iteration
# ---------------------------------------------------------------------------------------
def test_overflow_safe_terms():
    s1, s2, r = 0.4, 0.6, 2.5
    l = np.array([800.0, -800.0, -np.inf, 0.0, 1e-3, -1e-3, 30.0, -30.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):  # (e^-800 may underflow)
        f, _ = E.bridge_terms(l, l, 0.0, s1, s2, r)
        _, g = E.bridge_terms(l, l, 0.0, s1, s2, r)
    assert f[0] == 1.0 / s1 and g[0] == 0.0          # x = +800: e^-x underflows to 0
    assert f[1] == 0.0 and g[1] == 1.0 / (s2 * r)    # x = -800
    assert f[2] == 0.0 and g[2] == 1.0 / (s2 * r)    # a proposal the prior forbids: exactly 0
    assert f[3] == 1.0 / (s1 + s2 * r) and g[3] == f[3]
    # both forms are the same function: the textbook one where it does not overflow
    x = l[3:]
    np.testing.assert_allclose(f[3:], np.exp(x) / (s1 * np.exp(x) + s2 * r), rtol=1e-14)
    np.testing.assert_allclose(g[3:], 1.0 / (s1 * np.exp(x) + s2 * r), rtol=1e-14)
    num, den = E.bridge_sums(l, l, 0.0, s1, s2, r)
    assert num == f.sum() and den == g.sum()
    # lstar shifts x, nothing else
    f2, g2 = E.bridge_terms(l + 5.0, l + 5.0, 5.0, s1, s2, r)
    np.testing.assert_allclose(f2, f, rtol=1e-12)  # ((x + 5) - 5 rounds)
    np.testing.assert_allclose(g2, g, rtol=1e-12)
    assert np.isnan(E.bridge_terms([np.nan], [np.nan], 0.0, s1, s2, r)[0][0])


def test_fixed_point_is_the_ratio_of_normalising_constants():
    # p = 3 N(0, 1) (unnormalised), g = N(0.2, 1.3^2): r -> 3 whatever lstar and neff are
    rng = np.random.default_rng(7)
    xp, xg = rng.normal(size=20000), 0.2 + 1.3 * rng.normal(size=20000)

    def lp(t):
        return math.log(3.0) - 0.5 * t * t - 0.5 * math.log(2 * math.pi)

    def lg(t):
        return -0.5 * ((t - 0.2) / 1.3) ** 2 - math.log(1.3) - 0.5 * math.log(2 * math.pi)

    o = E.bridge_from_l(lp(xp) - lg(xp), lp(xg) - lg(xg), neff=20000.0)
    assert abs(o["logz"] - math.log(3.0)) <= 4 * o["logz_err"] and o["logz_err"] < 0.01


# ---------------------------------------------------------------------------------------
# 3. the proposal: covariance, draws, density
# ---------------------------------------------------------------------------------------
def test_chain_cov_is_numpys_and_spreads_a_nan_over_its_row_and_column():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(257, 5)) @ rng.normal(size=(5, 5)) + 10.0
    mean, cov = E.chain_cov(x)
    np.testing.assert_allclose(mean, x.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(cov, np.cov(x, rowvar=False), rtol=1e-11, atol=1e-13)
    x[100, 3] = np.nan
    mean, cov = E.chain_cov(x)
    bad = np.zeros((5, 5), bool)
    bad[3, :] = bad[:, 3] = True
    assert np.isnan(mean[3]) and np.array_equal(np.isnan(cov), bad)
    keep = [0, 1, 2, 4]
    np.testing.assert_allclose(cov[np.ix_(keep, keep)], np.cov(x[:, keep], rowvar=False),
                               rtol=1e-11, atol=1e-13)
    with np.errstate(all="ignore"):
        assert np.all(np.isnan(E.chain_cov(x[:1, :2])[1]))  # one row: 0 / 0


def test_pooled_rows_are_the_chains():
    rng = np.random.default_rng(4)
    chain = rng.normal(size=(7, 4, 3))
    got = E.pooled(chain, 2, 5, 12, 3, 4, 3)
    np.testing.assert_array_equal(got, chain[2:].reshape(-1, 3))
    m = rng.normal(size=(6, 5))  # a matrix with padding: npool = 1
    np.testing.assert_array_equal(E.pooled(m, 1, 5, 5, 0, 1, 3), m[1:, :3])


def test_draws_are_standard_normal_and_cut_anywhere():
    z = E.normals(20000, 5, seed=11)
    assert abs(z.mean()) < 4 / math.sqrt(z.size)
    assert abs((z * z).mean() - 1.0) < 4 * math.sqrt(2.0 / z.size)
    assert abs((z ** 4).mean() - 3.0) < 4 * math.sqrt(96.0 / z.size)
    c = np.corrcoef(z, rowvar=False)
    assert np.max(np.abs(c - np.eye(5))) < 4 / math.sqrt(len(z))  # (also the cos / sin pairs)
    np.testing.assert_array_equal(E.normals(7, 5, seed=11, row0=100), z[100:107])
    assert not np.any(E.normals(100, 5, seed=12) == z[:100])
    rng = np.random.default_rng(5)
    A = rng.normal(size=(3, 3))
    L, mean = np.linalg.cholesky(A @ A.T + np.eye(3)), np.array([1.0, -2.0, 0.5])
    th, z2 = E.mvn_draw(mean, L, 50000, seed=2)
    np.testing.assert_allclose(np.cov(th, rowvar=False), L @ L.T, atol=0.08)
    np.testing.assert_allclose(th.mean(axis=0), mean, atol=0.03)
    np.testing.assert_allclose(z2, (np.linalg.solve(L, (th - mean).T) ** 2).sum(axis=0),
                               rtol=1e-9)


def test_the_proposal_stream_is_not_the_replicates():
    # the same seed in predictive and here: different counter words, unrelated numbers
    seed, n = 12345, 4000
    a, below = R.draw(n, 4, np.ones(4), np.ones(4), seed=seed)
    ppc = np.where(below, -a, a)
    z = E.normals(n, 4, seed=seed)
    assert not np.any(np.isclose(np.abs(z), np.abs(ppc), rtol=1e-12, atol=0))
    c = np.corrcoef(z.ravel(), ppc.ravel())[0, 1]
    assert abs(c) < 4 / math.sqrt(z.size)
    c = np.corrcoef(np.abs(z).ravel(), np.abs(ppc).ravel())[0, 1]
    assert abs(c) < 4 / math.sqrt(z.size)
    # and word 3 is what separates them
    u = E.normals(n, 4, seed=seed, stream=0)
    assert not np.any(u == z)


def test_logpdf_is_the_normal_density():
    rng = np.random.default_rng(6)
    for d in (1, 2, 5):
        A = rng.normal(size=(d, d))
        cov, mean = A @ A.T + np.eye(d), rng.normal(size=d)
        L = np.linalg.cholesky(cov)
        th = rng.normal(size=(50, d)) * 2
        c = th - mean
        want = (-0.5 * np.einsum("ni,ij,nj->n", c, np.linalg.inv(cov), c)
                - 0.5 * d * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(cov)[1])
        np.testing.assert_allclose(E.mvn_logpdf(th, mean, L), want, rtol=1e-11)
        th[7, d - 1] = np.inf
        assert np.isnan(E.mvn_logpdf(th, mean, L)[7])
        # at a draw, the density follows from |z|^2
        t2, z2 = E.mvn_draw(mean, L, 20, seed=d)
        np.testing.assert_allclose(E.bridge_l2(np.zeros(20), z2, L), -E.mvn_logpdf(t2, mean, L),
                                   rtol=1e-10)
    assert E.bridge_l2([-np.inf], [1.0], np.eye(2))[0] == -np.inf


# ---------------------------------------------------------------------------------------
# 4. the public surface
# ---------------------------------------------------------------------------------------
def test_bayes_factor_is_antisymmetric():
    from naima_amd.evidence import bayes_factor
    a, b = dict(logz=-12.5, logz_err=0.03), dict(logz=-15.25, logz_err=0.04)
    ab, ba = bayes_factor(a, b), bayes_factor(b, a)
    assert ab[0] == 2.75 and ba[0] == -2.75
    assert ab[1] == ba[1] == pytest.approx(0.05, rel=1e-14)
    assert bayes_factor(a, a) == (0.0, pytest.approx(0.03 * math.sqrt(2.0)))
    with pytest.raises(ValueError):
        bayes_factor(a, dict(logz=1.0))


def test_importing_needs_no_device_and_argument_errors_come_first():
    code = r'''
import sys
import numpy as np
import naima_amd.evidence as V
import naima_amd.posterior as P
from naima_amd import _lib
assert _lib._lib is None and not _lib._default
assert "matplotlib" not in sys.modules
chain, lp = np.zeros((10, 4, 2)), np.zeros((10, 4))
fn = lambda t: np.zeros(len(t))
bad = [
    dict(chain=np.zeros((10, 8))),                 # not a chain
    dict(chain=np.zeros((10, 4, 33)), log_prob=lp),  # more than NH_EVID_MAX_DIM parameters
    dict(log_prob=np.zeros((10, 5))),              # another shape
    dict(log_prob=np.zeros((9, 4))),
    dict(log_prob_fn=None),
    dict(discard=-1), dict(discard=9),             # one row left
    dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5),
    dict(n_draws=0), dict(n_draws=2.5), dict(n_draws=2 ** 31),
    dict(neff=0.0), dict(neff=float("nan")), dict(neff=float("inf")),
    dict(log_prior_norm=float("inf")),
    dict(tol=0.0), dict(tol=-1.0),
    dict(maxiter=0), dict(maxiter=1.5),
    dict(batch=0), dict(batch=True),
]
n = 0
for kw in bad:
    a = dict(chain=chain, log_prob=lp, log_prob_fn=fn)
    a.update(kw)
    try:
        V.bridge_sampling(**a)
    except ValueError:
        n += 1
    else:
        raise SystemExit("no ValueError for %r" % (kw,))
for x in (np.zeros((5, 33)), np.zeros((4, 3, 40))):
    try:
        P.covariance(x)
    except ValueError:
        n += 1
try:
    P.covariance(np.zeros((5, 2)), discard=5)
except ValueError:
    n += 1
assert _lib._lib is None and not _lib._default, "an argument error touched the device"
print(n, sorted(V.__all__), "covariance" in P.__all__)
'''
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode()
    assert out.startswith("26 ")
    for name in ("bridge_sampling", "bayes_factor", "EvidenceMixin"):
        assert name in out
    assert out.strip().endswith("True")


def test_public_names():
    import naima_amd
    from naima_amd import evidence, posterior
    from naima_amd.sampler import EnsembleSampler
    for name in ("bridge_sampling", "bayes_factor", "EvidenceMixin"):
        assert name in evidence.__all__ and hasattr(evidence, name)
    assert "covariance" in posterior.__all__ and callable(posterior.covariance)
    assert naima_amd.evidence is evidence
    assert issubclass(EnsembleSampler, evidence.EvidenceMixin)
    doc = evidence.__doc__ + evidence.bridge_sampling.__doc__ + EnsembleSampler.log_evidence.__doc__
    for word in ("log_prior_norm", "proper", "read_run"):
        assert word in doc


def test_log_evidence_is_one_rank_only():
    from naima_amd.sampler import EnsembleSampler

    class TwoRanks:
        size, rank = 2, 0

    s = EnsembleSampler(8, 2, lambda t: np.zeros(len(t)), comm=TwoRanks())
    with pytest.raises(NotImplementedError):
        s.log_evidence()


def test_entry_points_are_declared():
    from naima_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "naima_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert int(re.search(r"#define\s+NH_EVID_MAX_DIM\s+(\d+)", hdr).group(1)) \
        == _lib.NH_EVID_MAX_DIM == 32
    src = open(os.path.join(ROOT, "naima_amd", "csrc", "nh_evidence.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src).lower()  # (sums in a fixed order)
    assert "nh_evidence.hip" in open(os.path.join(ROOT, "naima_amd", "csrc", "build.sh")).read()
    assert "%#x" % E.MVN_STREAM == "0x4d564e31" and "0x4D564E31u" in open(
        os.path.join(ROOT, "naima_amd", "csrc", "nh_philox.h")).read()
