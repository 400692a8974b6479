"""The rank-normalised convergence statistics of Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021
("Rank-normalization, folding, and localization"), restated in NumPy / SciPy as naima_amd.posterior
defines them: what tests/test_rank_host.py checks the properties of and tests/test_gpu_rank.py
compares the device with.

  ranks         scipy.stats.rankdata(method="average") of a parameter over all rows and walkers
  scores        z = ndtri((r - 3/8) / (S + 1/4)), S values ranked together
  folding       |x - np.median(pooled x)|
  R-hat         the BDA3 formula of test_ensembles_host.rhat_numpy over the pooled (split) ensembles,
                on z and on the scores of the folded values, the larger of the two
  ESS           S / tau, tau being emcee's estimator as test_autocorr_host.ref_integrated restates it
                (the autocorrelation function averaged over the walkers), on z (bulk) or on the
                indicators x <= q05 and x <= q95 (tail: the smaller of the two)
"""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from test_autocorr_host import ref_integrated
from test_ensembles_host import rhat_numpy


def pooled_ranks(chain, discard=0):
    """(rows - discard, nwalkers, ndim): every parameter ranked over all rows and walkers; NaN
    throughout for a parameter with a non-finite value"""
    x = np.asarray(chain, dtype=float)[discard:]
    r = np.empty_like(x)
    for d in range(x.shape[2]):
        col = x[:, :, d].ravel()
        r[:, :, d] = rankdata(col, method="average").reshape(x.shape[:2]) \
            if np.all(np.isfinite(col)) else np.nan
    return r


def scores(r, S):
    return ndtri((np.asarray(r, dtype=float) - 0.375) / (S + 0.25))


def rank_normalize(chain, discard=0):
    r = pooled_ranks(chain, discard)
    return scores(r, r.shape[0] * r.shape[1])


def fold(chain, discard=0):
    x = np.asarray(chain, dtype=float)[discard:]
    return np.abs(x - np.median(x.reshape(-1, x.shape[2]), axis=0))


def rhat_rank(chain, k, discard=0, split=True, folded=True):
    r = rhat_numpy(rank_normalize(chain, discard), k, 0, split)
    if folded:
        r = np.maximum(r, rhat_numpy(rank_normalize(fold(chain, discard)), k, 0, split))
    return r


def tau(x3, c=5):
    with np.errstate(all="ignore"):
        return ref_integrated(np.asarray(x3, dtype=float), c)[0]


def ess(chain, kind="bulk", discard=0, c=5):
    x = np.asarray(chain, dtype=float)[discard:]
    S = x.shape[0] * x.shape[1]
    with np.errstate(all="ignore"):
        if kind == "bulk":
            return S / tau(rank_normalize(x), c)
        q = np.quantile(x.reshape(S, -1), [0.05, 0.95], axis=0)
        return np.minimum(S / tau((x <= q[0]).astype(float), c), S / tau((x <= q[1]).astype(float), c))


# ---- the two cases the moment-based R-hat gets wrong ------------------------------------------
# Both: 500 rows of two ensembles of four walkers, one parameter, independent draws.  The seeds
# are fixed so that the restatement alone, on the CPU, satisfies the inequalities
# tests/test_rank_host.py asserts; the GPU tests ask the same of the device.
def case_heavy_tails():
    """(a) both ensembles from Student's t with 1.5 degrees of freedom (no variance), one value
    replaced by 1e300"""
    x = np.random.default_rng(2021).standard_t(1.5, size=(500, 8, 1))
    x[123, 5, 0] = 1e300
    return x


def case_scales():
    """(b) equal means, scales 1 and 3"""
    x = np.random.default_rng(7).standard_normal((500, 8, 1))
    x[:, 4:] *= 3.0
    return x
