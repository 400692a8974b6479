"""Several independent ensembles in one sampler, without a GPU: the move stream of k ensembles
(nh_moves_create_ensembles) against k stand-alone streams, the arguments of
``EnsembleSampler(ensembles=)`` and ``get_sampler``, the books a run keeps, and
``posterior.rhat``'s validation.  ``rhat_numpy`` restates the Gelman-Rubin formula in NumPy; the GPU
tests (tests/test_gpu_ensembles.py) compare the device with it."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from naima_amd.sampler import EnsembleSampler


def gauss(x):
    return -0.5 * np.sum((x - 1.5) ** 2 / 0.25, axis=1), np.sum(x, axis=1)


# ------------------------------------------------------------------ the restatement
def sequences_numpy(chain, k, discard=0, split=True):
    """the m = k (2 if split else 1) pooled sequences of a chain (rows, k n, ndim):
    [m][L][ndim], sequence part * k + r being the rows of ``part`` (a remainder dropped from the
    front) and the walkers [r n, (r+1) n) of ensemble r, L = rows per part * n"""
    x = np.asarray(chain, dtype=float)[discard:]
    rows, nw, nd = x.shape
    nsplit, n = (2 if split else 1), nw // k
    per = rows // nsplit
    x = x[rows - per * nsplit:]
    return np.array([x[p * per:(p + 1) * per, r * n:(r + 1) * n].reshape(per * n, nd)
                     for p in range(nsplit) for r in range(k)])


def rhat_numpy(chain, k, discard=0, split=True):
    """BDA3 (Gelman et al., 3rd ed., 11.4): W = mean of the within-sequence variances, B/L =
    variance of the sequence means, R-hat = sqrt(((L-1)/L W + B/L) / W); NaN for a parameter of
    which a sequence is constant or holds a non-finite value"""
    seq = sequences_numpy(chain, k, discard, split)
    L = seq.shape[1]
    with np.errstate(all="ignore"):
        var, mean = seq.var(axis=1, ddof=1), seq.mean(axis=1)
        W, BL = var.mean(axis=0), mean.var(axis=0, ddof=1)
        r = np.sqrt(((L - 1.0) / L * W + BL) / W)
    constant = np.any(np.ptp(seq, axis=1) == 0, axis=0)
    r[constant | np.any(~np.isfinite(seq), axis=(0, 1))] = np.nan
    return r


def test_restatement_on_known_sequences():
    """two sequences 0, 1, 2, 3 and 10, 11, 12, 13 (one walker each would be too few for the
    sampler, not for the formula): W = 5/3, B/L = 50, R-hat = sqrt((3/4 * 5/3 + 50) / (5/3));
    identical ensembles give sqrt((L-1)/L)"""
    x = np.zeros((4, 2, 1))
    x[:, 0, 0], x[:, 1, 0] = [0, 1, 2, 3], [10, 11, 12, 13]
    assert_allclose(rhat_numpy(x, 2, split=False), np.sqrt((0.75 * 5 / 3 + 50) / (5 / 3)), rtol=1e-15)
    x[:, 1, 0] = x[:, 0, 0]
    assert_allclose(rhat_numpy(x, 2, split=False), np.sqrt(0.75), rtol=1e-15)
    # split: the halves (0, 1) and (2, 3) of each
    assert_allclose(rhat_numpy(x, 2), np.sqrt((0.5 * 0.5 + 4.0 / 3.0) / 0.5), rtol=1e-15)
    x[:, 1, 0] = 7.0
    assert np.isnan(rhat_numpy(x, 2, split=False)[0])


def test_rhat_from_moments_is_the_restatement():
    from naima_amd.posterior import rhat_from_moments
    rng = np.random.default_rng(3)
    x = rng.normal(size=(21, 12, 3)) + np.arange(3)[:, None, None].repeat(4, axis=1).reshape(1, 12, 1)
    x[:, 4:8, 2] = 0.25      # a constant sequence
    x[5, 1, 1] = np.nan      # a non-finite value
    for split in (False, True):
        seq = sequences_numpy(x, 3, discard=2, split=split)
        fin = np.isfinite(seq)
        cnt = fin.sum(axis=1)
        with np.errstate(all="ignore"):
            mean = np.where(fin, seq, 0).sum(axis=1) / cnt
            var = (np.where(fin, seq - mean[:, None], 0) ** 2).sum(axis=1) / (cnt - 1)
        got = rhat_from_moments(cnt, mean, var, seq.shape[1])
        want = rhat_numpy(x, 3, discard=2, split=split)
        assert np.array_equal(np.isnan(got), [False, True, True])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert_allclose(got[0], want[0], rtol=1e-13)
        assert 1.2 < got[0] < 2.5


def test_rhat_validation_comes_before_any_device_work():
    from naima_amd import posterior
    x = np.zeros((10, 12, 2))
    for k in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            posterior.rhat(x, k)
    with pytest.raises(ValueError):
        posterior.rhat(x, 2.0)
    with pytest.raises(ValueError, match="do not split"):
        posterior.rhat(x, 5)
    with pytest.raises(ValueError, match="rows, nwalkers, ndim"):
        posterior.rhat(x[0], 2)
    with pytest.raises(ValueError, match="two at least"):
        posterior.rhat(x, 2, discard=7)  # three rows behind it: split needs four
    with pytest.raises(ValueError, match="negative"):
        posterior.rhat(x, 2, discard=-1)
    s = EnsembleSampler(16, 2, gauss)
    with pytest.raises(ValueError, match="ensembles >= 2"):
        s.get_rhat()
    with pytest.raises(ValueError, match="ensembles >= 2"):
        s.run_until_converged(np.zeros((16, 2)), 10, rhat=1.01)
    with pytest.raises(ValueError, match="larger than 1"):
        EnsembleSampler(16, 2, gauss, ensembles=2).run_until_converged(np.zeros((16, 2)), 10, rhat=1.0)


# ------------------------------------------------------------------ the stream
def test_stream_of_three_ensembles_is_three_streams():
    """k = 3, n = 6, seeds (11, 7, 11), 70 steps (two block boundaries): ensemble r's entries are
    Moves(seeds[r], 6)'s, z and ln U bit for bit, S and partner after subtracting 6 r; partners
    stay in the inactive half of the walker's own ensemble; equal seeds, equal ensembles"""
    from naima_amd._lib import Moves
    k, n, a, seeds, steps = 3, 6, 2.0, (11, 7, 11), 70
    h = n // 2

    def take(m):
        out = [[], [], [], []]
        left = steps
        while left:
            addr, got = m.take(left)
            for dst, v in zip(out, m.view(addr, got)):
                dst.append(v.copy())
            left -= got
        return [np.concatenate(v) for v in out]

    m = Moves(seeds, n, a, ensembles=k)
    assert (m.N, m.ns) == (k * n, k * h)
    S, P, Z, L = take(m)
    assert S.shape == (steps, 2, k * h) and Z.shape == S.shape
    for r in range(k):
        s1, p1, z1, l1 = take(Moves(seeds[r], n, a))
        sl = slice(r * h, (r + 1) * h)
        assert np.array_equal(Z[:, :, sl].view(np.uint64), z1.view(np.uint64))
        assert np.array_equal(L[:, :, sl].view(np.uint64), l1.view(np.uint64))
        assert np.array_equal(S[:, :, sl] - n * r, s1)
        assert np.array_equal(P[:, :, sl] - n * r, p1)
        # a partner of an active walker: same ensemble, inactive half
        assert np.all(P[:, :, sl] // n == r)
        for half in range(2):
            other = S[:, 1 - half, sl]
            assert np.all((P[:, half, sl, None] == other[:, None, :]).any(axis=-1))
    # every step moves every walker exactly once
    assert np.array_equal(np.sort(S.reshape(steps, -1), axis=1),
                          np.tile(np.arange(k * n), (steps, 1)))
    assert np.array_equal(S[:, :, 2 * h:] - 2 * n, S[:, :, :h])
    assert np.array_equal(P[:, :, 2 * h:] - 2 * n, P[:, :, :h])
    assert np.array_equal(Z[:, :, 2 * h:], Z[:, :, :h]) and np.array_equal(L[:, :, 2 * h:], L[:, :, :h])
    assert not np.array_equal(Z[:, :, h:2 * h], Z[:, :, :h])


def test_stream_arguments():
    from naima_amd._lib import Moves, NaimaHipError
    for seeds, k, n in [((1, 2), 0, 6), ((1, 2), 2, 5), ((1, 2), 2, 0)]:
        with pytest.raises((NaimaHipError, ValueError)):
            Moves(seeds, n, 2.0, ensembles=k)
    with pytest.raises(ValueError):
        Moves((1, 2, 3), 6, 2.0, ensembles=2)
    import ctypes as C
    from naima_amd import _lib
    lib, h = _lib.load(), C.c_void_p()
    assert lib.nh_moves_create_ensembles(None, 2, 6, 2.0, 32, 4, 0, C.byref(h)) != 0
    # one ensemble through the new entry point: nh_moves_create's stream
    for n in (8, 30):
        one, ref = Moves((5,), n, 2.0, ensembles=1), Moves(5, n, 2.0)
        for want in (9, 32, 32, 5):  # (into a third block)
            for x, y in zip(one.view(*one.take(want)), ref.view(*ref.take(want))):
                assert np.array_equal(x, y)


# ------------------------------------------------------------------ the sampler
def test_sampler_arguments():
    with pytest.raises(ValueError):
        EnsembleSampler(30, 3, gauss, ensembles=2)      # n = 15 is odd
    with pytest.raises(ValueError):
        EnsembleSampler(16, 3, gauss, ensembles=4)      # n = 4 < 2 ndim
    with pytest.raises(ValueError):
        EnsembleSampler(32, 3, gauss, ensembles=3)      # 32 / 3
    with pytest.raises(ValueError):
        EnsembleSampler(32, 3, gauss, ensembles=0)
    with pytest.raises(ValueError, match="seeds"):
        EnsembleSampler(32, 3, gauss, ensembles=2, seed=(1, 2, 3))
    s = EnsembleSampler(36, 3, gauss, ensembles=3, seed=40)
    assert s.seeds == (40, 41, 42) and s.seed == 40 and s.ensembles == 3
    assert s.ensemble_slices == [slice(0, 12), slice(12, 24), slice(24, 36)]
    assert EnsembleSampler(36, 3, gauss, ensembles=3, seed=[9, 9, 2]).seeds == (9, 9, 2)
    one = EnsembleSampler(12, 3, gauss, seed=40)
    assert one.seeds == (40,) and one.seed == 40 and one.ensembles == 1
    assert EnsembleSampler(12, 3, gauss).seed == 12345
    x = np.arange(5 * 36 * 3).reshape(5, 36, 3)
    y = s.split_ensembles(x)
    assert y.shape == (5, 3, 12, 3) and np.array_equal(y[:, 1], x[:, 12:24])
    assert s.split_ensembles(np.arange(36)).shape == (3, 12)
    with pytest.raises(ValueError):
        s.split_ensembles(np.zeros((5, 7)))


def test_several_ranks_are_refused(monkeypatch):
    class TwoRanks:
        rank, size = 0, 2

    with pytest.raises(NotImplementedError):
        EnsembleSampler(32, 3, gauss, ensembles=2, comm=TwoRanks())
    EnsembleSampler(32, 3, gauss, ensembles=1, comm=TwoRanks())
    monkeypatch.setenv("NAIMA_AMD_FORCE_SHARDED", "1")
    with pytest.raises(NotImplementedError):
        EnsembleSampler(32, 3, gauss, ensembles=2)
    EnsembleSampler(32, 3, gauss)


def test_host_loop_ensemble_is_the_single_run():
    """the host-driven loop on an analytic log-probability: ensemble r of a combined run is, bit
    for bit, the single-ensemble run with seeds[r] from the same positions (the evaluation is
    per walker here, so the launch shape cannot show), and moving ensemble 1's start leaves
    ensembles 0 and 2 alone"""
    k, n, nd, seeds = 3, 8, 3, (5, 21, 5)
    pos = np.random.default_rng(1).normal(size=(k * n, nd))
    c = EnsembleSampler(k * n, nd, gauss, ensembles=k, seed=seeds)
    c.run_mcmc(pos, 40)
    for r, sl in enumerate(c.ensemble_slices):
        s = EnsembleSampler(n, nd, gauss, seed=seeds[r])
        s.run_mcmc(pos[sl], 40)
        assert np.array_equal(c.get_chain()[:, sl], s.get_chain())
        assert np.array_equal(c.get_log_prob()[:, sl], s.get_log_prob())
        assert np.array_equal(c.get_blobs()[0][:, sl], s.get_blobs()[0])
        assert np.array_equal(c.naccepted[sl], s.naccepted)
    moved = pos.copy()
    moved[n:2 * n] += 3.0
    d = EnsembleSampler(k * n, nd, gauss, ensembles=k, seed=seeds)
    d.run_mcmc(moved, 40)
    for r in (0, 2):
        sl = c.ensemble_slices[r]
        assert np.array_equal(c.get_chain()[:, sl], d.get_chain()[:, sl])
    assert not np.array_equal(c.get_chain()[:, n:2 * n], d.get_chain()[:, n:2 * n])


# ------------------------------------------------------------------ get_sampler and the books
def _table():
    from naima_amd import datatable as D
    from naima_amd import units as u
    t = D.DataTable()
    t["energy"] = np.geomspace(1, 30, 6) * u.TeV
    t["flux"] = 1e-11 * np.geomspace(1, 30, 6) ** -2.0 * u.Unit("1/(cm2 s TeV)")
    t["flux_error"] = 0.1 * t["flux"]
    return t


def _powerlaw(pars, data):
    from naima_amd import units as u
    e = data["energy"].to("TeV").value
    return pars[0] * e ** -pars[1] * u.Unit("1/(cm2 s TeV)")


def test_get_sampler_starts_and_run_info(tmp_path):
    import naima_amd as na
    kw = dict(data_table=_table(), model=_powerlaw, labels=["norm", "index"], nburn=0,
              device=False, verbose=False)
    starts = np.array([[2e-11, 1.5], [1e-11, 2.0], [5e-12, 2.6]])
    s, st = na.get_sampler(p0=starts, nwalkers=24, seed=7, guess=False, **kw)
    assert s.ensembles == 3 and s.seeds == (7, 8, 9) and s.nwalkers == 24
    assert s.run_info["ensembles"] == 3 and s.run_info["seeds"] == [7, 8, 9]
    assert_allclose(s.run_info["p0"], starts)
    for r, sl in enumerate(s.ensemble_slices):
        want = starts[r] + 0.1 * starts[r] * np.random.default_rng(7 + r).normal(size=(8, 2))
        assert np.array_equal(st.coords[sl], want)
    with pytest.raises(ValueError):
        na.get_sampler(p0=starts, nwalkers=24, ensembles=2, **kw)
    # guess, row by row: every start is scaled to the data's flux
    g, _ = na.get_sampler(p0=starts, nwalkers=24, seed=7, **kw)
    gp = np.array(g.run_info["p0"])
    assert_allclose(gp[:, 1], starts[:, 1])
    assert len(set(np.round(gp[:, 0] / starts[:, 0], 6))) == 3
    # a 1-D p0: k balls round one point, ensemble r's the ball of get_sampler(seed=seeds[r])
    b, sb = na.get_sampler(p0=starts[1], nwalkers=24, ensembles=3, seed=(4, 30, 4), **kw)
    assert b.seeds == (4, 30, 4)
    for r, sl in enumerate(b.ensemble_slices):
        one, so = na.get_sampler(p0=starts[1], nwalkers=8, seed=b.seeds[r], **kw)
        assert one.ensembles == 1 and one.run_info["ensembles"] == 1
        assert one.run_info["seeds"] == [b.seeds[r]]
        assert np.array_equal(sb.coords[sl], so.coords)
    assert np.array_equal(sb.coords[:8], sb.coords[16:])
    # ... and through save_run / read_run
    s.log_prob_fn, s.naima_style, s.args = gauss, False, ()
    s.run_mcmc(np.random.default_rng(0).normal(size=(24, 2)) + 1.5, 6)
    r = na.read_run(na.save_run(str(tmp_path / "run"), s))
    assert r.run_info["ensembles"] == 3 and list(r.run_info["seeds"]) == [7, 8, 9]
    assert_allclose(r.run_info["p0"], starts)
    assert r.get_chain().shape == (6, 24, 2)


def test_chain_text_has_one_rhat_line_only_when_given():
    from naima_amd.plot import _chain_text

    class Run:
        acceptance_fraction = np.array([0.4, 0.5])

    dist = np.linspace(1.0, 2.0, 50)
    with_it = _chain_text(Run(), "index", dist, (8, 50), False, tau=3.2, rhat=1.2345)
    lines = with_it.split("\n")
    assert lines.count("Gelman-Rubin R-hat: 1.234") + lines.count("Gelman-Rubin R-hat: 1.235") == 1
    assert lines.index("Autocorrelation time: 3.2") + 1 == [
        i for i, l in enumerate(lines) if l.startswith("Gelman-Rubin")][0]
    without = _chain_text(Run(), "index", dist, (8, 50), False, tau=3.2)
    assert "Gelman-Rubin" not in without
    assert [l for l in lines if not l.startswith("Gelman-Rubin")] == without.split("\n")
    assert "nan" in _chain_text(Run(), "index", dist, (8, 50), False, rhat=np.nan)


def test_a_single_row_p0_is_the_one_dimensional_call():
    import naima_amd as na
    kw = dict(data_table=_table(), model=_powerlaw, labels=["norm", "index"], nburn=0,
              device=False, verbose=False, nwalkers=8, seed=3)
    a, sa = na.get_sampler(p0=[[1e-11, 2.0]], **kw)
    b, sb = na.get_sampler(p0=[1e-11, 2.0], **kw)
    assert a.ensembles == 1 and a.run_info == b.run_info
    assert np.ndim(a.run_info["p0"]) == 1 and np.array_equal(sa.coords, sb.coords)
