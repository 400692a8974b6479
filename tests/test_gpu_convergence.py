"""The running autocorrelation accumulator (nh_acf_accumulate / nh_acf_finalize behind
autocorr.RunningAutocorr) and EnsembleSampler.run_until_converged on the device loop.

Synthetic chains are AR(1) series per walker, made on the host from a fixed seed and uploaded; the
existing two-pass path (autocorr._integrated) and a float64 NumPy statement of emcee's
function_1d are computed once per chain and shared.

The tolerance.  The two-pass path centres every series on its mean, the running path on its first
value, so the running path's cancellation grows with (m / sigma)^2, m and sigma being the mean and
the spread of x - x[row_start].  Distances between autocorrelation functions are therefore taken in
units of  n_t * eps * (1 + max_w (m_w / sigma_w)^2)  per dimension.  C_EXISTING[chain] is the
largest distance of the EXISTING path from the NumPy statement in these units over that chain's
row_starts and dimensions, measured on an MI355X and rounded up to two digits
(profiles/NOTES_convergence.md; test_existing_path_distance prints and checks them); the running
path is allowed ten times that against the existing path.  The constants are kept per chain
because ONE constant over all chains would be the 35 units of the chain at offset 1e6, where the
NumPy statement's own mean rounds at 1e6 * eps: thirty thousand times what the other chains show.
tau = 2 sum_{k <= window} f_k - 1 is a sum of window + 1 such values: its tolerance is
2 (window + 1) times f's."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
# MEASURED (see the module docstring): 0.001066, 0.0004335, 0.0001655, 35.30; the device loop's
# cfg1 chains of the end-to-end test over their prefixes of 100, 200, ... rows: 0.0135, 0.0184
C_EXISTING = {"300x6": 0.0011, "1500x70": 0.00044, "5000x64": 0.00017, "offset-1e6": 36.0,
              "cfg1": 0.014, "cfg1-thin3": 0.019}
C = 5  # the window search's step, emcee's default

# name -> (n_t, n_w, rho of every dimension, offset, row_starts)
CHAINS = {
    "one-row": (1, 2, (0.5,), 3.0, (0,)),
    "300x6": (300, 6, (0.95,), 3.0, (0, 37)),
    "1500x70": (1500, 70, (0.5, 0.95, 0.5), -2.0, (0, 37)),
    "5000x64": (5000, 64, (0.5, 0.95), 10.0, (0, 37)),
    "offset-1e6": (1500, 8, (0.5, 0.95), 1e6, (0, 37)),
}
MAX_LAGS = (2, 256, 1024)
CASES = [(name, rs, L) for name, v in CHAINS.items() for rs in v[4] for L in MAX_LAGS]


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def ar1(n_t, n_w, rhos, offset, seed=20261018):
    """x[t][w][d]: unit-variance AR(1) noise of coefficient rhos[d] around offset + d"""
    rng = np.random.default_rng(seed)
    n_d = len(rhos)
    rho = np.asarray(rhos, dtype=float)
    e = rng.standard_normal((n_t, n_w, n_d))
    x = np.empty((n_t, n_w, n_d))
    x[0] = e[0]
    for t in range(1, n_t):
        x[t] = rho * x[t - 1] + np.sqrt(1.0 - rho ** 2) * e[t]
    return x + offset + np.arange(n_d)


def numpy_acf(x):
    """emcee's function_1d of every walker's series, averaged over the walkers: f[d][k]"""
    n_t = x.shape[0]
    n = 1
    while n < n_t:
        n <<= 1
    y = x - np.mean(x, axis=0)
    ft = np.fft.fft(y, n=2 * n, axis=0)
    acf = np.fft.ifft(ft * np.conjugate(ft), axis=0)[:n_t].real
    with np.errstate(invalid="ignore", divide="ignore"):
        acf = acf / acf[0]
    return np.mean(acf, axis=1).T


def unit(x):
    """n_t * eps * (1 + max_w (m_w / sigma_w)^2) per dimension, of x - x[0]"""
    y = x - x[0]
    m, sd = np.mean(y, axis=0), np.std(y, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(sd > 0, (m / sd) ** 2, 0.0)
    return x.shape[0] * EPS * (1.0 + np.max(r, axis=0))


@functools.lru_cache(maxsize=None)
def chain(name):
    n_t, n_w, rhos, offset, _ = CHAINS[name]
    x = ar1(n_t, n_w, rhos, offset)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def device_chain(name):
    from naima_amd import _lib
    x = chain(name)
    return _lib.get_context().array(np.ascontiguousarray(x).reshape(x.shape[0], -1))


@functools.lru_cache(maxsize=None)
def existing(name, row_start):
    """(tau, windows, [f of each dimension]) of the two-pass path on x[row_start:]"""
    from naima_amd import autocorr
    tau, windows, fs, _ = autocorr._integrated(chain(name)[row_start:], C)
    return tau, windows, fs


@functools.lru_cache(maxsize=None)
def reference(name, row_start):
    return numpy_acf(chain(name)[row_start:])


def running(buf, shape, row_start, max_lag, cuts=None):
    """RunningAutocorr over the block's rows, given in one call or at the row counts `cuts`"""
    from naima_amd.autocorr import RunningAutocorr
    n_t, n_w, n_d = shape
    ra = RunningAutocorr(n_w, n_d, max_lag=max_lag, c=C)
    for n in (cuts if cuts is not None else [n_t]):
        ra.update(buf, n, row_start)
    tau, windows = ra.tau()
    return ra, tau, windows


def f_distance(fa, fb, u):
    """max_k |fa[k] - fb[k]| over the lags both hold, in units of u"""
    m = min(len(fa), len(fb))
    return float(np.max(np.abs(np.asarray(fa[:m]) - np.asarray(fb[:m])))) / u


def existing_distances():
    """the existing path's distance from the NumPy statement, per (chain, row_start, dimension)"""
    out = {}
    for name, v in CHAINS.items():
        for rs in v[4]:
            x = chain(name)[rs:]
            if x.shape[0] < 2:
                continue  # (one row: a constant series, NaN on every path)
            u, ref = unit(x), reference(name, rs)
            for d, f in enumerate(existing(name, rs)[2]):
                out[(name, rs, d)] = f_distance(f, ref[d], u[d])
    return out


def check_against(tau, windows, fs, ref_tau, ref_windows, ref_fs, u, c_existing, what):
    """windows equal; f within 10 c_existing u, tau within 2 (window + 1) times that"""
    assert np.array_equal(windows, ref_windows), (what, windows, ref_windows)
    for d in range(len(u)):
        tol_f = 10.0 * c_existing * u[d]
        dt = abs(tau[d] - ref_tau[d])
        if fs is not None:
            dist = f_distance(fs[d], ref_fs[d], u[d])
            print("%s d=%d: f distance %.3g units (allowed %.3g)" % (what, d, dist, 10.0 * c_existing))
            assert dist <= 10.0 * c_existing, (what, d, dist)
        print("%s d=%d: |dtau| %.3g (allowed %.3g)" % (what, d, dt, 2 * (windows[d] + 1) * tol_f))
        assert dt <= 2 * (windows[d] + 1) * tol_f, (what, d, dt)


# ------------------------------------------------------------------------------- the accumulator
def test_existing_path_distance(na):
    """what the tolerance was taken from: the two-pass path against NumPy, in the units above"""
    dist = existing_distances()
    for key, v in sorted(dist.items()):
        print("existing path vs NumPy %s: %.4g units" % (key, v))
    for name in CHAINS:
        worst = [v for key, v in dist.items() if key[0] == name]
        if worst:
            print("%s: largest %.4g (C_EXISTING %r)" % (name, max(worst), C_EXISTING[name]))
            assert max(worst) <= C_EXISTING[name]


@pytest.mark.parametrize("name,row_start,max_lag", CASES)
def test_chunk_invariance(na, name, row_start, max_lag):
    """one call, calls of one row, calls of 7 then 300 rows: f and tau bit for bit"""
    x, buf = chain(name), device_chain(name)
    n_t = x.shape[0]
    ones = list(range(row_start + 1, n_t + 1))
    mixed, n = [], row_start
    while n < n_t:
        n = min(n_t, n + (7 if len(mixed) % 2 == 0 else 300))
        mixed.append(n)
    ra0, tau0, win0 = running(buf, x.shape, row_start, max_lag)
    for cuts in (ones, mixed):
        ra, tau, win = running(buf, x.shape, row_start, max_lag, cuts)
        assert ra.max_lag == ra0.max_lag and ra.rebuilds == ra0.rebuilds
        assert np.array_equal(ra.f, ra0.f, equal_nan=True)
        assert np.array_equal(tau, tau0, equal_nan=True) and np.array_equal(win, win0)
    if n_t - row_start > 1:
        assert np.all(ra0.f[:, 0] == 1.0) and np.all(np.isfinite(tau0))
    else:
        assert np.all(np.isnan(tau0))  # one row: a constant series


@pytest.mark.parametrize("name,row_start,max_lag", CASES)
def test_agreement_with_the_two_pass_path(na, name, row_start, max_lag):
    x, buf = chain(name), device_chain(name)
    ra, tau, win = running(buf, x.shape, row_start, max_lag)
    ref_tau, ref_win, ref_fs = existing(name, row_start)
    if x.shape[0] - row_start < 2:
        assert np.all(np.isnan(tau)) and np.all(np.isnan(ref_tau)) and np.array_equal(win, ref_win)
        return
    check_against(tau, win, list(ra.f), ref_tau, ref_win, ref_fs, unit(x[row_start:]),
                  C_EXISTING[name], "%s row_start=%d max_lag=%d" % (name, row_start, max_lag))


@pytest.mark.parametrize("row_start", [0, 37])
def test_constant_and_non_finite_series(na, row_start):
    """a constant walker, one inf, one NaN: their dimensions' tau is NaN, the fourth dimension is
    what it is without them, bit for bit"""
    from naima_amd import _lib, autocorr
    ctx = _lib.get_context()
    clean = ar1(400, 10, (0.5, 0.95, 0.5, 0.95), 3.0, seed=7)
    x = clean.copy()
    x[:, 3, 0] = 4.25
    x[200, 5, 1] = np.inf
    x[row_start + 2, 0, 2] = np.nan
    bufs = [ctx.array(a.reshape(400, -1)) for a in (clean, x)]
    for max_lag in (2, 256):
        (ra_c, tau_c, win_c), (ra, tau, win) = [running(b, x.shape, row_start, max_lag, [150, 400])
                                                for b in bufs]
        assert np.all(np.isnan(tau[:3])) and np.all(np.isnan(ra.f[:3]))
        assert np.all(win[:3] == 400 - row_start - 1)
        assert tau[3] == tau_c[3] and win[3] == win_c[3] and np.isfinite(tau[3])
        m = min(ra.f.shape[1], ra_c.f.shape[1])
        assert np.array_equal(ra.f[3, :m], ra_c.f[3, :m])
    ref_tau, ref_win, _, _ = autocorr._integrated(x[row_start:], C)
    assert np.array_equal(np.isnan(ref_tau), np.isnan(tau)) and np.array_equal(ref_win, win)


@pytest.mark.parametrize("name,row_start", [("300x6", 0), ("5000x64", 37)])
def test_forced_rebuild(na, name, row_start):
    """max_lag = 2 on a rho = 0.95 chain: the lags double until the window is certain, and the
    result is that of max_lag = 1024"""
    x, buf = chain(name), device_chain(name)
    small, tau_s, win_s = running(buf, x.shape, row_start, 2, [200, x.shape[0]])
    large, tau_l, win_l = running(buf, x.shape, row_start, 1024)
    assert small.rebuilds > 0 and large.rebuilds == 0 and 2 < small.max_lag <= 1024
    assert np.array_equal(tau_s, tau_l) and np.array_equal(win_s, win_l)
    m = small.f.shape[1]
    assert np.all(win_s < m) and np.array_equal(small.f, large.f[:, :m])


def test_update_starts_again_for_another_block_or_fewer_rows(na):
    x, buf = chain("300x6"), device_chain("300x6")
    ra, tau, _ = running(buf, x.shape, 0, 256, [100, 300])
    ra.update(buf, 120, 0)  # fewer rows than before: from the start
    assert ra.n == 120 and np.array_equal(ra.tau()[0], running(buf, x.shape, 0, 256, [120])[1])
    ra.update(buf, 300, 37)  # another row_start
    assert np.array_equal(ra.tau()[0], running(buf, x.shape, 37, 256)[1])
    with pytest.raises(ValueError):
        ra.update(buf, 301, 0)
    with pytest.raises(ValueError):
        ra.update(device_chain("1500x70"), 10, 0)  # not n_w * n_d columns


# --------------------------------------------------------------------------- on the device loop
def _problem(na, name):
    from bench import build_problem
    model, p0, raw, data, prior, labels = build_problem(name, na)
    return model, p0, data, prior


def _sampler(na, device, seed=31, nw=32):
    from naima_amd.sampler import EnsembleSampler
    model, p0, data, prior = _problem(na, "cfg1")
    nd = p0.size
    s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=seed, naima_style=True,
                        store_blobs=True, device=device, nan_policy="reject")
    pos = p0 * (1 + 0.003 * np.random.default_rng(seed).standard_normal((nw, nd)))
    return s, pos


def _resident_steps(monkeypatch):
    """steps made by launches of the resident loop, per DeviceLoop"""
    from naima_amd.device_sampler import DeviceLoop
    made, orig = {}, DeviceLoop._run_resident

    def counted(self, slice0, nslices, block):
        rec = orig(self, slice0, nslices, block)
        if rec is not None:
            made[id(self)] = made.get(id(self), 0) + nslices // 2
        return rec

    monkeypatch.setattr(DeviceLoop, "_run_resident", counted)
    return made


@pytest.mark.parametrize("device,thin_by,rtol", [(True, 1, 0.01), (True, 3, 0.01), (False, 1, 0.01),
                                                 (True, 1, 0.05)],
                         ids=["device", "device-thin3", "host", "device-rtol5"])
def test_run_until_converged_end_to_end(na, monkeypatch, device, thin_by, rtol):
    """the smallest workload, 32 walkers, at most 1500 rows checked every 100 with tol = 5 (with
    the default rtol the rule does not hold within 1500 rows on these chains; "device-rtol5"
    adds a run that stops early, in a block that is larger than the run)"""
    from numpy.testing import assert_allclose

    from naima_amd import autocorr
    max_steps, every, tol = 1500, 100, 5
    c_existing = C_EXISTING["cfg1" if thin_by == 1 else "cfg1-thin3"]
    made = _resident_steps(monkeypatch)
    s, pos = _sampler(na, device)
    with np.errstate(all="ignore"):
        st = s.run_until_converged(pos, max_steps=max_steps, check_every=every, tol=tol, rtol=rtol,
                                   thin_by=thin_by)
    conv = s.convergence
    stop = conv["rows"]
    assert conv["where"] == ("device" if device else "host")
    assert s.iteration == stop and s.steps_total == stop * thin_by
    x = s.get_chain()
    assert x.shape == (stop, 32, s.ndim)
    assert [r for r, _ in conv["history"]] == list(range(every, stop + 1, every))
    # the reference: the two-pass path on the final chain's prefixes, and the rule on it
    old, first, hit = np.inf, max_steps, False
    for n, tau in conv["history"]:
        ref_tau, ref_win, ref_fs, _ = autocorr._integrated(x[:n], C)
        assert np.all(np.isfinite(ref_tau))
        # the reference quantities keep clear of their thresholds, or the stop would hang on
        # the last bits of tau
        change = np.abs(old - ref_tau) / ref_tau
        print("rows %d: tau %s, tau * tol / n %s, change %s" % (n, ref_tau, ref_tau * tol / n, change))
        assert np.all(np.abs(ref_tau * tol - n) >= 1e-6 * n)
        assert np.all(np.abs(change - rtol) >= 1e-6 * rtol)
        if device:
            u, ref = unit(x[:n]), numpy_acf(x[:n])
            dist = [f_distance(ref_fs[d], ref[d], u[d]) for d in range(s.ndim)]
            print("rows %d: existing path vs NumPy %s units (C_EXISTING %r)" % (n, dist, c_existing))
            assert max(dist) <= c_existing
            check_against(tau, ref_win, None, ref_tau, ref_win, None, u, c_existing, "rows %d" % n)
        else:
            assert np.array_equal(tau, ref_tau)
        if not hit and autocorr.converged(ref_tau, old, n, tol, rtol):
            first, hit = n, True
        old = ref_tau
    assert stop == first and conv["converged"] == hit
    if device:
        # (measured: the device loop's chain stops early with rtol = 0.05 only; the host-driven
        # loop's chain differs from it to rounding and may pass the rule at any check, the last
        # one included)
        assert hit == (rtol > 0.01) and (not hit or stop < max_steps)
    print("stopped at %d rows, converged: %s, max_lag %d, rebuilds %d"
          % (stop, conv["converged"], conv["max_lag"], conv["rebuilds"]))

    def books(a, b):
        assert np.array_equal(np.asarray(st.coords), np.asarray(b[1].coords))
        assert np.array_equal(a.naccepted, b[0].naccepted)
        assert (a.nan_proposals, a.prior_forbidden_proposals) == \
            (b[0].nan_proposals, b[0].prior_forbidden_proposals)
        assert b[0].iteration == stop and b[0].steps_total == stop * thin_by

    # the same seed, run plainly for as many rows: the same chain bit for bit.  (A fresh sampler's
    # first call stays with the per-launch kernel on this workload, and the two kernels' log-
    # probabilities and blobs agree to rounding: test_resident_loop_equals_per_launch_loop)
    f, _ = _sampler(na, device)
    with np.errstate(all="ignore"):
        sf = f.run_mcmc(pos, stop, thin_by=thin_by)
    assert np.array_equal(f.get_chain(), x)
    assert_allclose(s.get_log_prob(), f.get_log_prob(), rtol=1e-9)
    for a, b in zip(s.get_blobs(), f.get_blobs()):
        assert_allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=1e-10,
                        atol=1e-300, equal_nan=True)
    books(s, (f, sf))
    # ... and as plain calls of check_every rows each, which issue the same launches: everything
    g, _ = _sampler(na, device)
    sg = pos
    with np.errstate(all="ignore"):
        for _ in range(0, stop, every):
            sg = g.run_mcmc(sg, every, thin_by=thin_by)
    assert np.array_equal(g.get_chain(), x)
    assert np.array_equal(g.get_log_prob(), s.get_log_prob())
    for a, b in zip(s.get_blobs(), g.get_blobs()):
        assert np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True)
    books(s, (g, sg))
    if device:
        # the resident loop wherever plain calls take it: as many steps by its launches as the
        # plain calls of check_every rows make, no fewer than the single plain call, and every
        # group behind the first (which makes the plan) whole
        d = s._dev
        assert d.resident_failed_launches == 0 and g._dev.resident_failed_launches == 0
        assert d.resident_info == g._dev.resident_info and d.resident_launches == g._dev.resident_launches
        assert made[id(d)] == made[id(g._dev)] >= made.get(id(f._dev), 0)
        assert made[id(d)] >= (stop - every) * thin_by, (made, stop)


def test_forced_sharding_is_refused_like_several_ranks(na, monkeypatch):
    monkeypatch.setenv("NAIMA_AMD_FORCE_SHARDED", "1")
    s, pos = _sampler(na, True)
    with pytest.raises(NotImplementedError):
        s.run_until_converged(pos, max_steps=1500, check_every=100, tol=5)
    assert s.steps_total == 0 and s.iteration == 0
