"""emcee's thin_by on the device loop: the steps' rows go to a staging block in HBM and every
thin_by-th one is copied to the compact block that is kept (nh_hist_thin) -- the kernel alone, the
loop against an unthinned run of the same launches, the staging budget, call sequences against the
host-driven loop, several ranks, and naima's run_sampler / plot_chain surface."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


def _problem(na, name):
    from bench import build_problem
    model, p0, raw, data, prior, labels = build_problem(name, na)
    return model, p0, data, prior, labels


# ------------------------------------------------------------------------------- the kernel
def _thin(ctx, mats, dsts, first, stride, nrows, dst_row0, offset=0):
    """upload, launch, download; offset: doubles by which every base is shifted (alignment)"""
    from naima_amd import _lib
    srcs_d = [ctx.array(np.concatenate([np.zeros(offset), m.ravel()])) for m in mats]
    dsts_d = [ctx.array(np.concatenate([np.zeros(offset), d.ravel()])) for d in dsts]
    segs = (_lib.nh_thin_seg * len(mats))(*[
        _lib.nh_thin_seg(a.ptr + 8 * offset, b.ptr + 8 * offset, m.shape[1])
        for a, b, m in zip(srcs_d, dsts_d, mats)])
    rc = _lib._lib.nh_hist_thin(ctx.h, segs, len(mats), first, stride, nrows, dst_row0)
    ctx.sync()
    return rc, [b.get()[offset:].reshape(d.shape) for b, d in zip(dsts_d, dsts)]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned-16", "aligned-8"])
def test_kernel_equals_numpy_slicing(na, offset):
    from naima_amd import _lib
    ctx = _lib.get_context()
    rng = np.random.default_rng(11)
    widths = [1, 2, 3, 64, 513, 2048, 2560, 4099]
    cases = 0
    for nsegs in range(1, 9):
        for rows, first, stride, nrows, dst_row0, drows in [
                (40, 1, 2, 19, 0, 19),     # ends one row short of the last
                (40, 4, 5, 7, 3, 12),      # rows 4, 9, ..., 34
                (40, 32, 33, 1, 2, 4),     # one row
                (70, 0, 1, 50, 5, 60),     # a plain copy
                (64, 6, 7, 8, 0, 9)]:      # rows 6, 13, ..., 55
            ws = [widths[(nsegs + k) % len(widths)] for k in range(nsegs)]
            mats = [rng.standard_normal((rows, w)) for w in ws]
            dsts = [np.full((drows, w), SENTINEL) for w in ws]
            rc, got = _thin(ctx, mats, dsts, first, stride, nrows, dst_row0, offset)
            assert rc == 0, _lib._lib.nh_last_error().decode()
            for m, g in zip(mats, got):
                assert first + (nrows - 1) * stride < rows - 1  # (short of the last row)
                want = m[first:first + (nrows - 1) * stride + 1:stride]
                assert want.shape[0] == nrows
                assert np.array_equal(g[dst_row0:dst_row0 + nrows], want)
                assert np.all(g[:dst_row0] == SENTINEL) and np.all(g[dst_row0 + nrows:] == SENTINEL)
            cases += 1
    assert cases == 40


def test_kernel_refuses_bad_arguments(na):
    from naima_amd import _lib
    ctx = _lib.get_context()
    lib = _lib._lib
    src = ctx.array(np.arange(60.0))
    dst = ctx.array(np.full(60, SENTINEL))
    w = 3

    def run(segs, nsegs, first, stride, nrows, dst_row0):
        rc = lib.nh_hist_thin(ctx.h, segs, nsegs, first, stride, nrows, dst_row0)
        ctx.sync()
        return rc

    one = (_lib.nh_thin_seg * 1)(_lib.nh_thin_seg(src.ptr, dst.ptr, w))
    assert run(one, 1, 0, 0, 2, 0) != 0 and "stride" in lib.nh_last_error().decode()
    assert run(one, 1, -1, 2, 2, 0) != 0 and "first" in lib.nh_last_error().decode()
    assert run(one, 0, 0, 2, 2, 0) != 0 and "nsegs" in lib.nh_last_error().decode()
    nine = (_lib.nh_thin_seg * 9)(*[_lib.nh_thin_seg(src.ptr, dst.ptr, w)] * 9)
    assert run(nine, 9, 0, 2, 2, 0) != 0 and "nsegs" in lib.nh_last_error().decode()
    assert run(one, 1, 0, 2, -1, 0) != 0
    # in place: rows 1, 3, 5 of a matrix to its own rows 0, 1, 2
    same = (_lib.nh_thin_seg * 1)(_lib.nh_thin_seg(src.ptr, src.ptr, w))
    assert run(same, 1, 1, 2, 3, 0) != 0 and "overlap" in lib.nh_last_error().decode()
    # ... and a destination that starts inside the rows read
    part = (_lib.nh_thin_seg * 1)(_lib.nh_thin_seg(src.ptr, src.ptr + 8 * w * 4, w))
    assert run(part, 1, 0, 2, 3, 0) != 0 and "overlap" in lib.nh_last_error().decode()
    # (the same rows, disjoint: behind the rows read)
    assert run(part, 1, 0, 1, 4, 0) == 0
    assert np.array_equal(src.get()[:24], np.r_[np.arange(12.0), np.arange(12.0)])
    # nothing of the refused calls was launched; nrows == 0 is a no-op that succeeds
    assert run(one, 1, 0, 2, 0, 0) == 0
    assert np.all(dst.get() == SENTINEL)


# ------------------------------------------------------------------------- the device loop
def _samplers(na, name, nw, seed=31):
    from naima_amd.sampler import EnsembleSampler
    model, p0, data, prior, _ = _problem(na, name)
    nd = p0.size
    kw = dict(args=[data, model, prior], seed=seed, naima_style=True, store_blobs=True,
              device=True, nan_policy="reject")
    rng = np.random.default_rng(seed)
    pos = p0 + 0.1 * p0 * rng.normal(size=(nw, nd))  # (the benchmark's ball: NaN and -inf occur)
    return EnsembleSampler(nw, nd, na.lnprob, **kw), EnsembleSampler(nw, nd, na.lnprob, **kw), pos


def _row_bytes(dev):
    return 8 * dev.N * (dev.ndim + 1 + sum(m for _, m, _, _ in dev.cur_blobs))


def _alloc_mb(dev, rows):
    """what the context sets aside for a staging block of `rows` rows, in MiB"""
    widths = [dev.N * dev.ndim, dev.N] + [dev.N * m for _, m, _, _ in dev.cur_blobs]
    return sum(dev.ctx._bucket(8 * rows * w) for w in widths) / float(1 << 20)


def _thinned_and_unthinned(na, monkeypatch, name, nw, t, n, budget_rows):
    """a thinned call of n rows behind a 4-step warm-up call, and a second sampler from the same
    seed that makes the same steps unthinned, call by call as thin_info lists them"""
    d, f, pos = _samplers(na, name, nw)
    with np.errstate(all="ignore"):
        sd, sf = d.run_mcmc(pos, 4), f.run_mcmc(pos, 4)
        dev = d._dev
        budget = _alloc_mb(dev, budget_rows) if budget_rows else 1e-6
        monkeypatch.setenv("NAIMA_AMD_THIN_STAGE_MB", repr(budget))
        it0, steps0 = d.iteration, d.steps_total
        sd = d.run_mcmc(sd, n, thin_by=t)
        info = dev.thin_info
        # the memory condition: the staging block within the budget (or one row), the block that
        # flush downloads compact
        assert info["thin_by"] == t and info["where"] == "device"
        assert info["stage_bytes"] <= max(budget * (1 << 20), _row_bytes(dev))
        assert info["stage_bytes"] == info["stage_rows"] * _row_bytes(dev)
        kept = dev.hist[-1]
        assert kept["n"] == n and kept["coords"].shape[0] == n and kept["logp"].shape[0] == n
        assert all(b.shape[0] == n for b in kept["blobs"]) and len(kept["blobs"]) == len(dev.cur_blobs) >= 1
        assert d.iteration == it0 + n and d.steps_total == steps0 + n * t
        assert sum(c[0] for c in info["calls"]) == n * t
        for steps, _ in info["calls"]:
            sf = f.run_mcmc(sf, steps)
    assert dev.resident_launches > 0 and f._dev.resident_launches == dev.resident_launches
    return d, f, sd, sf, info


def _pick(a, t):
    return np.asarray(a, dtype=float)[4:][t - 1::t]  # (behind the warm-up call's four rows)


@pytest.mark.parametrize("t", [2, 5, 32, 33])
@pytest.mark.parametrize("name,nw", [("cfg1", 32), ("cfg3", 512)], ids=["cfg1-32", "cfg3-512"])
def test_thinned_run_equals_rows_of_the_unthinned_run(na, monkeypatch, name, nw, t):
    """chunks of c*t steps into a staging block of at most 127 rows (a budget of what 64 rows
    take: the pool rounds allocations up to powers of two), over 400 steps: at least three chunks
    and a dozen 32-step blocks of moves.  Both runs issue the same launches: bit for bit"""
    n = 400 // t + 2
    d, f, sd, sf, info = _thinned_and_unthinned(na, monkeypatch, name, nw, t, n, 64)
    assert len(info["calls"]) >= 3, info
    assert all(steps % t == 0 and stored == steps for steps, stored in info["calls"])
    assert t <= info["stage_rows"] < 128 and info["stage_rows"] % t == 0
    assert d.get_chain().shape == (4 + n, nw, d.ndim)
    assert np.array_equal(d.get_chain()[4:], _pick(f.get_chain(), t))
    assert np.array_equal(d.get_log_prob()[4:], _pick(f.get_log_prob(), t))
    bd, bf = d.get_blobs(), f.get_blobs()
    assert len(bd) == len(bf) >= 2
    for x, y in zip(bd, bf):
        assert np.array_equal(np.asarray(x, dtype=float)[4:], _pick(y, t), equal_nan=True)
    assert np.array_equal(sd.coords, sf.coords) and np.array_equal(sd.log_prob, sf.log_prob)
    assert np.array_equal(d.naccepted, f.naccepted)
    assert np.array_equal(d.acceptance_fraction, f.acceptance_fraction)
    assert d.iteration == 4 + n and f.iteration == 4 + n * t


@pytest.mark.parametrize("name,nw", [("cfg1", 32), ("cfg3", 512)], ids=["cfg1-32", "cfg3-512"])
def test_budget_below_thin_by_rows_keeps_one_row_of_staging(na, monkeypatch, name, nw):
    """a budget that not even t rows fit: every stored row is t - 1 steps without a history and one
    step with it, the staging block is one row.  The unthinned run keeps a history for all steps
    (another route for the blobs through the same launches): the NaN / inf patterns are the same
    and the values agree as two routes through the loops do (test_resident_loop_equals_per_launch_
    loop's tolerances)"""
    t, n = 5, 24
    d, f, sd, sf, info = _thinned_and_unthinned(na, monkeypatch, name, nw, t, n, 0)
    assert info["stage_rows"] == 1 and info["calls"] == [(t - 1, 0), (1, 1)] * n
    a, b = d.get_chain()[4:], _pick(f.get_chain(), t)
    assert a.shape == b.shape == (n, nw, d.ndim)
    assert_allclose(a, b, rtol=1e-10)
    la, lb = d.get_log_prob()[4:], _pick(f.get_log_prob(), t)
    assert np.array_equal(np.isinf(la), np.isinf(lb)) and np.array_equal(np.isnan(la), np.isnan(lb))
    fin = np.isfinite(lb)
    assert_allclose(la[fin], lb[fin], rtol=1e-9)
    same = np.array_equal(a, b) and np.array_equal(la, lb, equal_nan=True)
    for x, y in zip(d.get_blobs(), f.get_blobs()):
        x, y = np.asarray(x, dtype=float)[4:], _pick(y, t)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.isinf(x), np.isinf(y))
        assert_allclose(x, y, rtol=1e-10, atol=1e-300, equal_nan=True)
        same = same and np.array_equal(x, y, equal_nan=True)
    assert_allclose(d.acceptance_fraction, f.acceptance_fraction)
    assert d.iteration == 4 + n
    print("%s: one-row staging == unthinned rows; bit-identical: %s" % (name, same))


def test_thin_by_one_takes_the_unthinned_path(na):
    d, f, pos = _samplers(na, "cfg1", 32)
    with np.errstate(all="ignore"):
        sd = d.run_mcmc(d.run_mcmc(pos, 4), 70, thin_by=1)
        sf = f.run_mcmc(f.run_mcmc(pos, 4), 70)
    assert d._dev.thin_info is None  # (no staging block, no extra launch)
    assert np.array_equal(d.get_chain(), f.get_chain()) and d.iteration == f.iteration == 74
    assert np.array_equal(sd.coords, sf.coords)


def test_call_sequences_with_thinning_equal_the_host_loop(na):
    """thinned and unthinned calls, a reset, reads between calls, calls without a history and an
    iterated generator, on the device loop and on the host-driven loop (the tolerances of
    test_seeded_call_sequences_equal_the_host_loop)"""
    from naima_amd.sampler import EnsembleSampler
    model, p0, data, prior, _ = _problem(na, "cfg1")
    nw, nd = 32, p0.size
    kw = dict(args=[data, model, prior], seed=31, naima_style=True, store_blobs=True)
    rng = np.random.default_rng(20261016)

    def compare(h, d, where):
        assert d.iteration == h.iteration and d.steps_total == h.steps_total, where
        ch, cd = h.get_chain(), d.get_chain()
        assert cd.shape == ch.shape, where
        assert_allclose(cd, ch, rtol=1e-8, err_msg=where)
        assert_allclose(d.get_log_prob(), h.get_log_prob(), rtol=1e-6, err_msg=where)
        bh, bd = h.get_blobs(), d.get_blobs()
        assert (bh is None) == (bd is None), where
        for x, y in zip(bd or [], bh or []):
            x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
            assert x.shape == y.shape, where
            assert_allclose(x, y, rtol=1e-8, atol=1e-300, equal_nan=True, err_msg=where)
        assert_allclose(d.acceptance_fraction, h.acceptance_fraction, err_msg=where)

    sequences = [
        [("run", 5, 1, True), ("run", 6, 5, True), ("read",), ("run", 3, 2, False),
         ("run", 10, 1, True), ("read",), ("reset",), ("run", 4, 7, True), ("iter", 5, 3, True),
         ("read",)],
        [("run", 2, 33, True), ("read",), ("iter", 4, 2, False), ("run", 2, 1, False),
         ("run", 7, 2, True), ("read",), ("reset",), ("read",), ("run", 1, 3, True), ("read",)],
    ]
    for k, ops in enumerate(sequences):
        h = EnsembleSampler(nw, nd, na.lnprob, **kw)
        d = EnsembleSampler(nw, nd, na.lnprob, device=True, **kw)
        sh = sd = p0 * (1 + 0.003 * rng.standard_normal((nw, nd)))
        for i, op in enumerate(ops):
            where = "sequence %d, call %d of %s" % (k, i, ops)
            if op[0] == "run":
                sh = h.run_mcmc(sh, op[1], store=op[3], thin_by=op[2])
                sd = d.run_mcmc(sd, op[1], store=op[3], thin_by=op[2])
            elif op[0] == "iter":
                nh = nd_ = 0
                for sh in h.sample(sh, op[1], store=op[3], thin_by=op[2]):
                    nh += 1
                for sd in d.sample(sd, op[1], store=op[3], thin_by=op[2]):
                    nd_ += 1
                assert nh == nd_ == op[1], where  # one state per stored row
            elif op[0] == "reset":
                h.reset()
                d.reset()
            else:
                compare(h, d, where)
                assert_allclose(sd.coords, sh.coords, rtol=1e-8, err_msg=where)
        assert d._dev.resident_launches > 0


# --------------------------------------------------------------------------- several ranks
def test_sharded_path_on_one_rank_thins_on_the_host(na, monkeypatch):
    """the sharded code path (NAIMA_AMD_FORCE_SHARDED=1, a one-rank communicator): the block stays
    full-rate in HBM, tagged, and flush slices it -- against the one-rank thinned run, with the
    tolerances of the sharded path's own test (test_sharded_path_with_rccl_on_one_rank)"""
    from naima_amd.sampler import EnsembleSampler
    model, p0, data, prior, _ = _problem(na, "cfg3")
    nw, nd = 64, p0.size
    kw = dict(args=[data, model, prior], seed=42, naima_style=True, store_blobs=True, device=True)
    pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((nw, nd)))

    def run():
        s = EnsembleSampler(nw, nd, na.lnprob, **kw)
        st = s.run_mcmc(pos, 4)
        st = s.run_mcmc(st, 8, thin_by=5)
        st = s.run_mcmc(st, 2, store=False, thin_by=3)
        st = s.run_mcmc(st, 3, thin_by=2)
        return s, st

    one, st1 = run()
    assert one._dev.thin_info["where"] == "device"
    monkeypatch.setenv("NAIMA_AMD_FORCE_SHARDED", "1")
    s, st = run()
    assert s._dev.sharded and s._dev.thin_info["where"] == "host"
    assert s._dev.hist[-1]["thin_by"] == 2 and s._dev.hist[-1]["coords"].shape[0] == 6
    assert s.iteration == one.iteration == 4 + 8 + 2 + 3
    assert s.steps_total == one.steps_total == 4 + 40 + 6 + 6
    assert s.get_chain().shape == one.get_chain().shape == (15, nw, nd)
    assert_allclose(s.get_chain(), one.get_chain(), rtol=1e-9)
    assert_allclose(s.get_log_prob(), one.get_log_prob(), rtol=1e-7)
    for x, y in zip(s.get_blobs(), one.get_blobs()):
        assert_allclose(np.asarray(x, dtype=float), np.asarray(y, dtype=float), rtol=1e-9,
                        atol=1e-300)
    assert_allclose(st.coords, st1.coords, rtol=1e-9)
    assert_allclose(s.acceptance_fraction, one.acceptance_fraction)


def test_thinned_run_of_two_ranks_sharing_one_gpu(na, tmp_path):
    """two processes on the one GPU share cfg3's ensemble (the resident loop over a shared
    ensemble): thinned calls, with and without a history, between unthinned ones -- every rank
    reads what one process's thinned run gives (test_shared_ensemble_two_ranks_one_gpu's
    tolerances)"""
    from naima_amd.sampler import EnsembleSampler
    name, nw, nranks = "cfg3", 32, 2
    port = 29700 + (os.getpid() % 1000)
    subprocess.check_call(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=%d" % nranks, "--master-addr", "127.0.0.1", "--master-port", str(port),
         os.path.join(ROOT, "tests", "gpu_thin_ranks_worker.py"), str(tmp_path), name, str(nw)],
        cwd=ROOT, timeout=600,
        env=dict(os.environ, MASTER_ADDR="127.0.0.1", NH_RUN_SPIN_LIMIT=str(1 << 24)))
    model, p0, data, prior, _ = _problem(na, name)
    nd = p0.size
    s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=42, naima_style=True,
                        store_blobs=True, device=True, nan_policy="reject")
    pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((nw, nd)))
    st = s.run_mcmc(pos, 5)
    st = s.run_mcmc(st, 14, thin_by=5)
    st = s.run_mcmc(st, 3, store=False, thin_by=3)
    st = s.run_mcmc(st, 4)
    st = s.run_mcmc(st, 2, thin_by=33)
    want = dict(coords=st.coords, logp=st.log_prob, chain=s.get_chain(), lnp=s.get_log_prob(),
                blob0=np.asarray(s.get_blobs()[0]), blob1=np.asarray(s.get_blobs()[1]),
                acc=s.acceptance_fraction)
    assert want["chain"].shape[0] == 25
    for r in range(nranks):
        for key, w in want.items():
            have = np.load(tmp_path / ("%s_%d.npy" % (key, r)))
            assert have.shape == w.shape, (key, r)
            assert_allclose(have, w, rtol=1e-10, atol=1e-300, err_msg="%s of rank %d" % (key, r))


# --------------------------------------------------------------------------------- surface
def test_run_sampler_thin_by_and_the_autocorrelation_time_in_steps(na, capsys):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from naima_amd import plot as P
    from naima_amd.autocorr import integrated_time
    model, p0, data, prior, labels = _problem(na, "cfg3")
    # (64 walkers from a 10 % ball decorrelate over a few hundred steps: a row every 40 steps, and
    # rows enough for integrated_time's tol = 50)
    nw, nrun, t = 64, 2000, 40
    s, pos = na.get_sampler(data_table=data, p0=p0, labels=labels, model=model, prior=prior,
                            nwalkers=nw, nburn=40, prefit=False, seed=4, verbose=False)
    assert s.iteration == 40  # (the burn-in is not thinned)
    s, pos = na.run_sampler(nrun, sampler=s, pos=pos, verbose=True, thin_by=t)
    out = capsys.readouterr().out
    assert "(1000 of 2000 steps)" in out
    assert s.device and s._dev is not None and s._dev.thin_info["where"] == "device"
    assert s.run_info["thin_by"] == t and s.run_info["n_run"] == nrun
    chain = s.get_chain()
    assert chain.shape == (nrun, nw, p0.size) and s.iteration == nrun
    assert s.steps_since_reset == nrun * t
    assert np.shape(s.get_blobs()[0])[:2] == (nrun, nw)
    assert 0.1 < np.mean(s.acceptance_fraction) < 0.9
    tau_rows = integrated_time(chain)
    tau = s.get_autocorr_time(thin=t, quiet=True)
    assert tau.shape == (p0.size,) and np.all(np.isfinite(tau)) and np.all(tau > 0)
    text = "\n".join(x.get_text() for x in P.plot_chain(s, 1).texts)
    print("autocorrelation time, stored rows:", tau_rows, "-> steps:", tau_rows * t)
    assert "Autocorrelation time: %.1f" % (tau_rows[1] * t) in text
    assert "Steps in chain: %d" % nrun in text
    plt.close("all")
