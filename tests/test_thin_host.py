"""emcee's thin_by on the host-driven loop (no GPU): ``run_mcmc(pos, n, thin_by=t)`` makes n*t
steps and keeps the states after steps t, 2t, ...; the books (iteration = stored rows, steps_total
= steps made, acceptance per step made) and naima's run_sampler / save_run surface."""
import numpy as np
import pytest

from naima_amd.sampler import EnsembleSampler, run_sampler

NW, ND = 32, 3


def gauss(x):
    return -0.5 * np.sum((x - 1.5) ** 2 / 0.25, axis=1), np.sum(x, axis=1), x[:, :2] * 2.0


def start():
    return np.random.default_rng(2).normal(size=(NW, ND))


@pytest.mark.parametrize("t", [1, 2, 7])
def test_thinned_run_is_every_tth_row_of_the_unthinned_run(t):
    n = 9
    full = EnsembleSampler(NW, ND, gauss, seed=5)
    sf = full.run_mcmc(start(), n * t)
    thin = EnsembleSampler(NW, ND, gauss, seed=5)
    before = thin.steps_total
    st = thin.run_mcmc(start(), n, thin_by=t)
    assert np.array_equal(thin.get_chain(), full.get_chain()[t - 1::t])
    assert thin.get_chain().shape == (n, NW, ND)
    assert np.array_equal(thin.get_log_prob(), full.get_log_prob()[t - 1::t])
    bt, bf = thin.get_blobs(), full.get_blobs()
    assert len(bt) == len(bf) == 2
    for a, b in zip(bt, bf):
        assert np.array_equal(a, b[t - 1::t])
    assert np.array_equal(st.coords, sf.coords) and np.array_equal(st.log_prob, sf.log_prob)
    assert thin.iteration == n
    assert thin.steps_total - before == n * t and thin.steps_since_reset == n * t
    assert np.array_equal(thin.acceptance_fraction, full.acceptance_fraction)
    assert np.array_equal(thin.naccepted, full.naccepted)


@pytest.mark.parametrize("bad", [0, -1, "x"])
def test_invalid_thinning_raises(bad):
    s = EnsembleSampler(NW, ND, gauss, seed=5)
    with pytest.raises(ValueError):
        s.run_mcmc(start(), 3, thin_by=bad)
    with pytest.raises(ValueError):
        next(s.sample(start(), iterations=3, thin_by=bad))
    assert s.steps_total == 0
    s.run_info = {}
    with pytest.raises(ValueError):
        run_sampler(3, sampler=s, pos=start(), verbose=False, thin_by=bad)


def test_generator_yields_one_state_per_stored_row():
    n, t = 6, 4
    full = EnsembleSampler(NW, ND, gauss, seed=8)
    full.run_mcmc(start(), n * t)
    s = EnsembleSampler(NW, ND, gauss, seed=8)
    states = [np.array(st.coords) for st in s.sample(start(), iterations=n, thin_by=t)]
    assert len(states) == n
    assert np.array_equal(np.array(states), full.get_chain()[t - 1::t])
    # store=False: still one state every t steps, nothing kept
    s2 = EnsembleSampler(NW, ND, gauss, seed=8)
    states2 = [np.array(st.coords) for st in
               s2.sample(start(), iterations=n, store=False, thin_by=t)]
    assert len(states2) == n and np.array_equal(np.array(states2), np.array(states))
    assert s2.get_chain().shape[0] == 0 and s2.steps_total == n * t


def test_calls_with_different_thinning_follow_each_other():
    full = EnsembleSampler(NW, ND, gauss, seed=3)
    full.run_mcmc(start(), 3 + 4 * 5 + 2 * 2)
    s = EnsembleSampler(NW, ND, gauss, seed=3)
    st = s.run_mcmc(start(), 3)
    st = s.run_mcmc(st, 4, thin_by=5)
    st = s.run_mcmc(st, 2, thin_by=2)
    rows = [0, 1, 2] + [3 + 5 * k + 4 for k in range(4)] + [23 + 2 * k + 1 for k in range(2)]
    assert np.array_equal(s.get_chain(), full.get_chain()[rows])
    assert np.array_equal(s.get_blobs()[1], full.get_blobs()[1][rows])
    assert s.iteration == 9 and s.steps_total == 27
    assert np.array_equal(s.acceptance_fraction, full.acceptance_fraction)
    s.reset()
    assert s.iteration == 0 and s.steps_since_reset == 0 and s.steps_total == 27
    s.run_mcmc(st, 2, thin_by=3)
    assert s.steps_since_reset == 6 and s.iteration == 2
    assert np.array_equal(s.acceptance_fraction, s.naccepted / 6.0)


def test_run_sampler_records_thin_by_and_it_survives_save_and_read(tmp_path, capsys):
    import naima_amd as na
    from naima_amd.datatable import make_data
    n, t = 20, 3
    full = EnsembleSampler(NW, ND, gauss, seed=4)
    full.run_mcmc(start(), n * t)
    s = EnsembleSampler(NW, ND, gauss, seed=4)
    s.labels = ["norm", "index", "cutoff"]
    s.run_info = {"n_walkers": NW, "n_burn": 0}
    s, pos = run_sampler(n, sampler=s, pos=start(), verbose=True, thin_by=t)
    out = capsys.readouterr().out
    assert "(10 of 20 steps)" in out  # the printout goes by stored rows
    assert s.run_info["thin_by"] == t and s.run_info["n_run"] == n
    assert s.get_chain().shape == (n, NW, ND) and s.steps_since_reset == n * t
    assert np.array_equal(s.get_chain(), full.get_chain()[t - 1::t])
    k = 5
    s.data = make_data(dict(energy=np.geomspace(1, 10, k), energy_unit="TeV",
                            flux=np.ones(k), flux_error_lo=0.1 * np.ones(k),
                            flux_error_hi=0.1 * np.ones(k), ul=np.zeros(k, bool), cl=0.9,
                            flux_unit="1/(cm2 s TeV)"))
    fn = na.save_run(str(tmp_path / "run"), s)
    r = na.read_run(fn)
    assert int(r.run_info["thin_by"]) == t
    assert np.array_equal(r.get_chain(), s.get_chain())
    # an unthinned run records thin_by = 1
    s1 = EnsembleSampler(NW, ND, gauss, seed=4)
    s1.run_info = {}
    run_sampler(4, sampler=s1, pos=start(), verbose=False)
    assert s1.run_info["thin_by"] == 1 and s1.iteration == 4
