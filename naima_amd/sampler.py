"""The ensemble driver: an affine-invariant stretch-move sampler with the surface
naima reads from ``emcee.EnsembleSampler`` (core.py:127-160, 450-493, 529-530 of the
reference), but calling the log-probability ONCE per half-ensemble with all
proposed walkers, and sharding those walkers over the GPUs of a node.

emcee itself is third-party (``emcee>=3.0``, not in the reference tree, not
installed here): the move below restates its published algorithm
(``RedBlueMove.propose`` + ``StretchMove.get_proposal``) -- random split of the
ensemble into two halves; for the active half S with complement C:
z = ((a-1)U+1)^2/a, partner j ~ randint(|C|), q = C_j - (C_j - S) z,
accept if ln U' < (ndim-1) ln z + lnp(q) - lnp(S).  Parity with emcee is
statistical, not bitwise ("parity unpinned").
"""
import time

import os

import numpy as np

from . import units as u
from .dist import LocalComm, shard_bounds, shard_counts
from .evidence import EvidenceMixin
from .infocrit import InfoCritMixin
from .optimize import OptimizeMixin
from .predictive import PredictiveMixin
from .reweight import ReweightMixin

__all__ = ["EnsembleSampler", "State", "get_sampler", "run_sampler"]


class State:
    """what ``sampler.sample`` yields (emcee.State): coords, log_prob, blobs"""

    def __init__(self, coords, log_prob=None, blobs=None, random_state=None):
        if isinstance(coords, State):
            self.coords, self.log_prob = coords.coords.copy(), coords.log_prob
            self.blobs, self.random_state = coords.blobs, coords.random_state
            return
        self.coords = np.atleast_2d(np.array(coords, dtype=float))
        self.log_prob = log_prob
        self.blobs = blobs
        self.random_state = random_state

    def __iter__(self):  # emcee allows  pos, lnp, rstate = state
        return iter((self.coords, self.log_prob, self.random_state))


def _split_blob(b):
    """a blob returned by the model -> (ndarray with leading walker axis, unit or None)"""
    if isinstance(b, u.Quantity):
        return np.asarray(b.value, dtype=float), b.unit
    return np.asarray(b, dtype=float), None


class EnsembleSampler(InfoCritMixin, PredictiveMixin, EvidenceMixin, ReweightMixin,
                      OptimizeMixin):
    """Stretch-move ensemble sampler over a *batched* log-probability.

    log_prob_fn(coords[n, ndim], *args) -> lnp[n]  or  (lnp[n], blob0[n,...], ...)
    With ``naima_style=True`` (what ``get_sampler`` uses) the function is naima's
    ``lnprob(pars, data, model, prior)`` and is called with ``coords.T`` so that
    ``pars[i]`` is a vector over walkers.

    ``ensembles`` = k > 1: the ``nwalkers`` = k n walkers are k INDEPENDENT ensembles of n, walkers
    [r n, (r+1) n) being ensemble r, that share every launch: each walker's partner is drawn from
    its own ensemble (``_lib.Moves(..., ensembles=k)``), nothing else differs.  ``seed`` is then an
    int s, for the seeds (s, s+1, ..., s+k-1), or a sequence of k ints; ensemble r makes exactly
    the moves of a single-ensemble sampler of n walkers with seed ``seeds[r]``.  ``get_rhat``
    compares the ensembles (Gelman-Rubin).  One rank only.
    """

    def __init__(self, nwalkers, ndim, log_prob_fn, args=(), a=2.0, seed=None, comm=None,
                 naima_style=False, store_blobs=True, device=False, use_graph=True,
                 nan_policy="raise", ensembles=1):
        if isinstance(ensembles, bool) or not isinstance(ensembles, (int, np.integer)) \
                or ensembles < 1:
            raise ValueError("ensembles must be a positive integer")
        k = int(ensembles)
        if nwalkers % k or (nwalkers // k) % 2 or nwalkers // k < 2 * ndim:
            raise ValueError("need an even number of walkers%s, at least twice the dimension"
                             % (" in each of the %d ensembles" % k if k > 1 else ""))
        self.nwalkers, self.ndim, self.a = int(nwalkers), int(ndim), float(a)
        self.ensembles, self.nwalkers_each = k, int(nwalkers) // k
        self.log_prob_fn, self.args = log_prob_fn, tuple(args)
        self.comm = comm if comm is not None else LocalComm()
        # the streams are replicated on every rank: proposals/accepts are identical.
        # _rng: numpy, for the initial ball; _moves: the C++ stretch-move stream
        if seed is None or np.ndim(seed) == 0:
            s0 = int(seed if seed is not None else 12345)
            self.seeds = tuple(s0 + r for r in range(k))
        else:
            self.seeds = tuple(int(v) for v in seed)
            if len(self.seeds) != k:
                raise ValueError("%d seeds for %d ensembles" % (len(self.seeds), k))
        if k > 1 and (self.comm.size > 1 or
                      os.environ.get("NAIMA_AMD_FORCE_SHARDED", "0") == "1"):
            raise NotImplementedError("several ensembles with walkers sharded over several ranks")
        self.seed = self.seeds[0]
        self._rng = np.random.default_rng(self.seed)
        self._moves = None
        self.naima_style = naima_style
        self.store_blobs = store_blobs
        # a proposal whose log-probability is NaN: "raise" is emcee's behaviour (ValueError
        # "Probability function returned NaN", EnsembleSampler.compute_log_prob) -- the host loop
        # raises on the spot, the device loop (whose launches cannot) when the run's results
        # next reach the host; "reject" treats the proposal as one that is never accepted and
        # counts it in ``nan_proposals``
        if nan_policy not in ("raise", "reject"):
            raise ValueError("nan_policy must be 'raise' or 'reject'")
        self.nan_policy = nan_policy
        self.nan_proposals = 0
        # proposals the prior forbade (-inf): the device loop evaluates none of their integrals
        # (the reference evaluates the model and discards it, core.py:103-119); counted for the
        # bench line, which credits them as walker-steps like every other proposal
        self.prior_forbidden_proposals = 0
        self.steps_total = 0  # ensemble steps since the sampler was made (reset() keeps it)
        # device=True: ensemble, proposals, log-probabilities and blobs live in HBM; the
        # launch sequence of one half-step (propose -> model -> likelihood -> accept)
        # is captured into a hipGraph and replayed (needs naima_style log_prob_fn)
        self.device = bool(device)
        self.use_graph = bool(use_graph)
        self._device_ok = None
        # accept + next proposal + parameter packs as ONE launch (nh_move_cycle)
        self.fuse_moves = os.environ.get("NAIMA_AMD_FUSE_MOVES", "1") != "0"
        self._dev = None
        self.n_lnprob_calls = 0
        self.n_walker_evals = 0
        self.reset()

    def moves(self, pinned=False):
        """the stretch-move random stream (one per sampler, created on first use)"""
        if self._moves is None:
            from ._lib import Moves
            if self.ensembles == 1:
                self._moves = Moves(self.seed, self.nwalkers, self.a, ksteps=32, depth=4,
                                    pinned=pinned)
            else:
                self._moves = Moves(self.seeds, self.nwalkers_each, self.a, ksteps=32, depth=4,
                                    pinned=pinned, ensembles=self.ensembles)
        return self._moves

    @property
    def ensemble_slices(self):
        """the walkers of each ensemble: ``[slice(r n, (r+1) n) for r in range(ensembles)]``"""
        n = self.nwalkers_each
        return [slice(r * n, (r + 1) * n) for r in range(self.ensembles)]

    def split_ensembles(self, x, axis=None):
        """``x`` with its walker axis (the first of length ``nwalkers``, or ``axis``) reshaped
        into (ensembles, walkers of each)"""
        x = np.asarray(x)
        if axis is None:
            hits = [i for i, m in enumerate(x.shape) if m == self.nwalkers]
            if not hits:
                raise ValueError("no axis of length nwalkers = %d" % self.nwalkers)
            axis = hits[0]
        axis = axis % x.ndim
        if x.shape[axis] != self.nwalkers:
            raise ValueError("axis %d is not of length nwalkers = %d" % (axis, self.nwalkers))
        return x.reshape(x.shape[:axis] + (self.ensembles, self.nwalkers_each) + x.shape[axis + 1:])

    # ------------------------------------------------------------------ store
    def reset(self):
        if getattr(self, "_dev", None) is not None:
            self._dev.reset()
        self.iteration = 0
        self._steps_at_reset = self.steps_total
        self._chain, self._logp, self._blobs = [], [], None
        # (blob_units stays: the units are the model function's, not the chain's, and the run
        # that follows a burn-in starts from a state with log-probabilities and never
        # evaluates the initial ensemble again -- run_sampler's results keep their units)
        self.naccepted = np.zeros(self.nwalkers)
        if getattr(self, "_dev", None) is not None:
            # several ranks: the ensemble all of them were found well at is kept NOW, behind the
            # cleared books (a replay after the reference's burn-in -> reset -> run flow,
            # core.py:483-487, 529-530, must not bring the burn-in's iteration count and
            # acceptance counters back)
            self._dev.keep_verified()

    @property
    def steps_since_reset(self):
        """ensemble steps made since ``reset()`` (``iteration`` counts the rows STORED since then:
        with ``thin_by`` = t it grows by one every t steps)"""
        return self.steps_total - self._steps_at_reset

    @property
    def acceptance_fraction(self):
        """moves accepted per walker, divided by the steps MADE since ``reset()``.  (emcee divides
        by the backend's ``iteration``, the count of stored rows, and so over-reports a thinned
        run's acceptance fraction by a factor of ``thin_by``.)"""
        self._flush()
        return self.naccepted / max(1, self.steps_since_reset)

    def _flush(self):
        if self._dev is not None:
            self._dev.flush()

    def get_chain(self, flat=False, discard=0, thin=1):
        self._flush()
        c = np.array(self._chain).reshape(-1, self.nwalkers, self.ndim)[discard::thin]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_prob(self, flat=False, discard=0, thin=1):
        self._flush()
        c = np.array(self._logp).reshape(-1, self.nwalkers)[discard::thin]
        return c.reshape(-1) if flat else c

    def get_blobs(self, flat=False, discard=0, thin=1):
        """list (one entry per blob) of arrays [nsteps, nwalkers, ...]; dense, not
        emcee's object array"""
        self._flush()
        if self._blobs is None:
            return None
        out = []
        for per_step in self._blobs:
            a = np.array(per_step)[discard::thin]
            out.append(a.reshape((-1,) + a.shape[2:]) if flat else a)
        return out

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """emcee's estimate of the integrated autocorrelation time of each parameter:
        ``thin * integrated_time(self.get_chain(discard=discard, thin=thin), **kwargs)``, the
        autocorrelation function computed on the GPU (naima_amd.autocorr).  ``kwargs`` are
        integrated_time's (``c``, ``tol``, ``quiet``); a chain shorter than ``tol`` times the
        estimate raises ``autocorr.AutocorrError`` unless ``quiet=True``.  With several ranks this
        is a COLLECTIVE call, as ``get_chain`` is: every rank makes it, or none does."""
        from .autocorr import integrated_time
        x = self.get_chain(discard=discard, thin=thin)
        return thin * integrated_time(x, **kwargs)

    def get_rhat(self, discard=0, split=True, method="moments"):
        """Gelman-Rubin R-hat of each parameter across the independent ensembles
        (``posterior.rhat`` of ``get_chain(discard=discard)``, the moments computed on the GPU);
        needs ``ensembles`` >= 2.  ``method="rank"``: the rank-normalised, folded statistic of
        Vehtari et al. 2021, the chain ranked on the GPU."""
        from .posterior import _check_method, rhat
        _check_method(method)
        if self.ensembles < 2:
            raise ValueError("R-hat compares independent ensembles: make the sampler with "
                             "ensembles >= 2")
        if method == "moments":
            return rhat(self.get_chain(discard=discard), self.ensembles, split=split)
        block = self._chain_block(1)
        if block is not None:
            return rhat(block, self.ensembles, discard=discard, split=split, method=method)
        return rhat(self.get_chain(discard=discard), self.ensembles, split=split, method=method)

    def _chain_block(self, thin=1):
        """the stored chain as a ``dview.DeviceChain`` with its log-probabilities where the
        device loop still holds ALL of it in one pending history block in HBM (one rank, every
        stored row asked for), else None: the caller uploads ``get_chain()``.  Nothing is flushed;
        the launches that fill the block are settled first, as a flush settles them."""
        from .dview import DeviceChain, matrix_on
        dev = self._dev
        if dev is None or thin != 1 or self.comm.size > 1 or len(self._chain) or len(dev.hist) != 1:
            return None
        b = dev.hist[0]
        if not b.plain:
            return None
        dev._meet()
        return DeviceChain(matrix_on(b.coords, b.n, self.nwalkers * self.ndim),
                           self.nwalkers, self.ndim, matrix_on(b.logp, b.n, self.nwalkers))

    def get_ess(self, kind="bulk", discard=0, thin=1):
        """The bulk or tail effective sample size of each parameter
        (``posterior.ess(self.get_chain(discard=discard, thin=thin), kind)``, ranked and reduced
        on the GPU): the stored values over emcee's autocorrelation time of the rank-normalised
        chain, or of the indicators of its 5 % and 95 % quantiles.  Read from the history block in
        HBM where the device loop still holds the whole chain there (``thin=1``)."""
        from .posterior import _check_kind, ess
        _check_kind(kind)
        block = self._chain_block(thin)
        if block is not None:
            return ess(block, kind, discard=discard)
        return ess(self.get_chain(discard=discard, thin=thin), kind)

    def get_summary(self, discard=0):
        """``posterior.summary`` of ``get_chain(discard=discard)``: mean, sd, median, q16, q84,
        ess_bulk, ess_tail, tau and, with several ensembles, rhat and rhat_rank per parameter;
        read from the history block in HBM where the device loop still holds the whole chain"""
        from .posterior import summary
        block = self._chain_block(1)
        labels = getattr(self, "labels", None)
        if block is not None:
            return summary(block, self.ensembles, discard=discard, labels=labels)
        return summary(self.get_chain(discard=discard), self.ensembles, labels=labels)

    # legacy emcee-2 names that naima's analysis code touches
    @property
    def chain(self):
        return np.swapaxes(self.get_chain(), 0, 1)

    @property
    def flatchain(self):
        return self.get_chain(flat=True)

    @property
    def lnprobability(self):
        return self.get_log_prob().T

    # --------------------------------------------------------------- evaluate
    def compute_log_prob(self, coords):
        """lnprob of ``coords[n, ndim]``: this rank evaluates its block, the blocks
        meet in one all-gather.  Returns (lnp[n], [local blob arrays], (lo, hi))."""
        n = coords.shape[0]
        lo, hi = shard_bounds(n, self.comm.rank, self.comm.size)
        mine = coords[lo:hi]
        if self.naima_style:
            res = self.log_prob_fn(mine.T, *self.args)
        else:
            res = self.log_prob_fn(mine, *self.args)
        self.n_lnprob_calls += 1
        self.n_walker_evals += hi - lo
        if isinstance(res, tuple):
            lnp_local, blobs = np.asarray(res[0], dtype=float), list(res[1:])
        else:
            lnp_local, blobs = np.asarray(res, dtype=float), []
        lnp_local = np.broadcast_to(lnp_local, (hi - lo,)).astype(float)
        if np.any(np.isnan(lnp_local)):
            if self.nan_policy == "raise":
                raise ValueError("Probability function returned NaN")
            self.nan_proposals += int(np.isnan(lnp_local).sum())
            lnp_local = np.where(np.isnan(lnp_local), -np.inf, lnp_local)
        if self.comm.size > 1:
            m = max(shard_counts(n, self.comm.size))
            pad = np.full((m,), -np.inf)
            pad[:hi - lo] = lnp_local
            allp = self.comm.allgather(pad).reshape(self.comm.size, m)
            lnp = np.concatenate([allp[r, :c] for r, c in
                                  enumerate(shard_counts(n, self.comm.size))])
        else:
            lnp = lnp_local
        return lnp, blobs, (lo, hi)

    def _blob_arrays(self, blobs, nloc):
        arrs, units = [], []
        for b in blobs:
            v, un = _split_blob(b)
            if v.ndim == 0 or v.shape[0] != nloc:
                v = np.broadcast_to(v, (nloc,) + v.shape).copy()
            arrs.append(v)
            units.append(un)
        return arrs, units

    # ------------------------------------------------------------------ sample
    def sample(self, initial_state, iterations=1, store=True, log_prob0=None, yield_every=1,
               thin_by=1):
        """emcee's generator: one State per ensemble step.  ``yield_every`` > 1 (what
        ``run_mcmc`` asks for) lets the device loop replay several steps as one hipGraph
        and yield only after each such group.

        ``thin_by`` = t (emcee 3): the call makes ``iterations * t`` steps and stores -- and
        yields -- the state after every t-th of them; ``iteration`` counts the stored rows,
        ``steps_total`` the steps made, and ``yield_every`` counts stored rows.  The device loop
        thins on the GPU (DeviceLoop.sample): the full-rate history never leaves HBM."""
        thin_by = int(thin_by)
        if thin_by <= 0:
            raise ValueError("Invalid thinning argument")
        if self.device:
            if self._dev is None and self._device_ok is None:
                self._device_ok = self._probe_device(initial_state)
            if self._device_ok is not False:
                yield from self._sample_device(initial_state, iterations, store, yield_every,
                                               thin_by)
                return
            # the model shapes a grid / table per walker (Eemin, a seed temperature ... as
            # fit parameters): the general path needs the values on the host
        state = State(initial_state)
        coords = state.coords.copy()
        if coords.shape != (self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions")
        rng = self._rng
        N, ndim, a = self.nwalkers, self.ndim, self.a
        keep_blobs = self.store_blobs
        # every rank keeps the blobs of ALL walkers: the rank that evaluates a walker
        # changes from half-step to half-step (a random split, contiguous shards of it), so
        # the proposals' blobs follow their log-probabilities through one more all-gather
        # per blob (as the device loop does; this host-driven loop is the general /
        # fallback path and pays for it with the control plane's bandwidth)
        if state.log_prob is None:
            logp, blobs, (lo, hi) = self.compute_log_prob(coords)
            cur, units = self._blob_arrays(blobs, hi - lo) if keep_blobs else ([], [])
            self.blob_units = units
            self._cur_blobs = [np.array(self._gather_rows(b, N)) for b in cur]
        else:
            logp = np.array(state.log_prob, dtype=float)
            if not hasattr(self, "_cur_blobs"):
                self._cur_blobs = []
        logp = logp.copy()
        moves = self.moves()
        for step in range(1, int(iterations) * thin_by + 1):
            addr, got = moves.take(1)
            Sm, Pm, Zm, Lm = moves.view(addr, got)
            for split in range(2):
                S, zz = Sm[0, split], Zm[0, split]
                s, cp = coords[S], coords[Pm[0, split]]
                factors = (ndim - 1.0) * np.log(zz)
                q = cp - (cp - s) * zz[:, None]
                newlp, blobs, (lo, hi) = self.compute_log_prob(q)
                lnpdiff = factors + newlp - logp[S]
                accepted = Lm[0, split] < lnpdiff
                acc_idx = S[accepted]
                coords[acc_idx] = q[accepted]
                logp[acc_idx] = newlp[accepted]
                self.naccepted[acc_idx] += 1
                if keep_blobs and blobs:
                    new, _ = self._blob_arrays(blobs, hi - lo)
                    for cur, nb in zip(self._cur_blobs, new):
                        cur[acc_idx] = self._gather_rows(nb, len(S))[accepted]
            self.steps_total += 1
            if step % thin_by:
                continue
            self.iteration += 1
            if store:
                self._chain.append(coords.copy())
                self._logp.append(logp.copy())
                if keep_blobs and self._cur_blobs:
                    if self._blobs is None:
                        self._blobs = [[] for _ in self._cur_blobs]
                    for j, b in enumerate(self._cur_blobs):
                        self._blobs[j].append(b.copy())
            yield State(coords, logp, self._cur_blobs if keep_blobs else None, rng)

    # ------------------------------------------------------------ device mode
    def _probe_device(self, initial_state):
        """one evaluation of two walkers on lazy device parameters: does the model run
        with its parameters in HBM?  Models that shape a particle grid or an emission
        table per walker do not (NotImplementedError from the radiative classes); they
        are sampled by the host-driven loop, which evaluates such walkers one by one."""
        import warnings

        from . import _lib
        from .darray import DPars
        if not self.naima_style:
            return True
        ctx = _lib.get_context()
        c = np.ascontiguousarray(State(initial_state).coords[:2].T, dtype=float)
        why = None
        try:
            res = self.log_prob_fn(DPars(ctx, ctx.array(c), self.ndim, c.shape[1]), *self.args)
            if self.store_blobs:
                from . import units as u
                from .darray import DFactor, DMat, DVec, lift_factor
                for b in res[1:]:
                    v = lift_factor(b.value if isinstance(b, u.Quantity) else b, c.shape[1])
                    if not isinstance(v, (DMat, DVec, DFactor, float, int)):
                        why = "a blob of type %s cannot be kept in HBM" % type(v).__name__
        except NotImplementedError as e:  # grid-/table-shaping parameters per walker
            why = str(e)
        except (TypeError, ValueError) as e:
            # a model that is not built from naima_amd's radiative classes: plain numpy
            # arithmetic on the parameters (ValueError from DVec), a functional model that
            # returns a host array (TypeError from the device likelihood) ...
            why = "%s: %s" % (type(e).__name__, e)
        finally:
            ctx.flush()
        if why is not None:
            warnings.warn("device=True is not possible for this model (%s); using the "
                          "host-driven loop (pass device=False to silence this)" % (why,))
            self.device = False
            return False
        return True

    def _sample_device(self, initial_state, iterations, store, yield_every=1, thin_by=1):
        from .device_sampler import DeviceLoop
        if self._dev is None:
            self._dev = DeviceLoop(self)
        yield from self._dev.sample(initial_state, iterations, store, yield_every, thin_by)

    def _gather_rows(self, rows, n):
        """this rank's block of an n-row array -> all n rows, on every rank"""
        size = self.comm.size
        if size == 1:
            return rows
        counts = shard_counts(n, size)
        pad = np.zeros((max(counts),) + rows.shape[1:])
        pad[:len(rows)] = rows
        allp = self.comm.allgather(pad).reshape((size, max(counts)) + rows.shape[1:])
        return np.concatenate([allp[r, :c] for r, c in enumerate(counts)], axis=0)

    def run_mcmc(self, initial_state, nsteps, thin_by=1, **kw):
        """``nsteps`` stored rows, ``nsteps * thin_by`` ensemble steps (see ``sample``)"""
        state = None
        kw.setdefault("yield_every", 1 << 30)  # nobody looks at the intermediate states
        for state in self.sample(initial_state, iterations=nsteps, thin_by=thin_by, **kw):
            pass
        return state


    def run_until_converged(self, initial_state, max_steps, check_every=100, tol=50, rtol=0.01,
                            c=5, discard=0, thin_by=1, max_lag=1024, rhat=None,
                            rhat_method="moments"):
        """Run until the integrated autocorrelation time has converged (the loop of emcee's
        tutorial "Autocorrelation analysis & convergence"), ``max_steps`` stored rows at the most.

        Every ``check_every`` stored rows the autocorrelation time ``tau`` of the rows this call has
        stored behind its first ``discard`` is estimated (``integrated_time(..., c=c, tol=0)``, in
        stored rows); the run stops at the first check with ``all(tau * tol < n)`` and
        ``all(|tau_old - tau| / tau < rtol)``, n being the number of those rows
        (``autocorr.converged``).  A NaN ``tau`` never converges (one warning).  ``thin_by`` is
        ``run_mcmc``'s.  Returns the last state; ``self.convergence`` says how it went:
        ``converged``, ``rows`` (stored by this call), ``tau``, ``history`` (``(rows, tau)`` of every
        check), ``where``, ``max_lag`` and ``rebuilds``.

        ``rhat`` = a number such as 1.01 (a sampler of ``ensembles`` >= 2): a check also requires
        ``all(R-hat < rhat)``, the split Gelman-Rubin statistic across the ensembles over the same
        rows (``posterior.rhat``) -- what tau alone cannot see, an ensemble that has settled
        somewhere else.  ``convergence["rhat"]`` is then the last check's R-hat and the history
        entries are ``(rows, tau, rhat)``.  tau is estimated over all walkers as before.
        ``rhat_method="rank"`` checks the rank-normalised, folded statistic instead
        (``posterior.rhat(method="rank")``, the one a threshold of 1.01 is defined for): the rows
        stored so far are ranked where they lie; ``convergence["rhat_method"]`` records which.

        On the device loop (``where == "device"``) the chain stays in HBM: the call allocates ONE
        history block of ``max_steps`` rows -- the memory of ``run_mcmc(max_steps)`` -- that its
        groups of ``check_every`` rows fill, and the lag sums below ``max_lag`` grow with it
        (``autocorr.RunningAutocorr``).  The host-driven loop (``where == "host"``) calls
        ``integrated_time`` on its chain at every check.  Several ranks: not implemented."""
        import warnings

        from . import autocorr
        max_steps, check_every, discard = int(max_steps), int(check_every), int(discard)
        thin_by, max_lag = int(thin_by), int(max_lag)
        if max_steps <= 0 or check_every <= 0:
            raise ValueError("max_steps and check_every must be positive")
        if not 0 <= discard < max_steps:
            raise ValueError("discard must lie in [0, max_steps)")
        if max_lag < 2:
            raise ValueError("max_lag must be at least 2")
        if thin_by <= 0:
            raise ValueError("Invalid thinning argument")
        if self.comm.size > 1 or (self.device and
                                  os.environ.get("NAIMA_AMD_FORCE_SHARDED", "0") == "1"):
            raise NotImplementedError("run_until_converged with walkers sharded over several ranks")
        if rhat is not None:
            if self.ensembles < 2:
                raise ValueError("rhat needs a sampler of ensembles >= 2")
            rhat = float(rhat)
            if not rhat > 1.0:
                raise ValueError("rhat must be larger than 1")
        from .posterior import _check_method
        _check_method(rhat_method)
        info = dict(converged=False, rows=0, tau=np.full(self.ndim, np.nan), history=[],
                    where="host", max_lag=max_lag, rebuilds=0)
        if rhat is not None:
            info["rhat"] = np.full(self.ndim, np.nan)
            info["rhat_method"] = rhat_method
        self.convergence = info
        old, warned = [np.inf], []
        from .posterior import rhat as _rhat

        def gelman_rubin(x, rows):
            """R-hat of the rows behind discard; NaN while each half has fewer than two"""
            if rows - discard < 4:
                return np.full(self.ndim, np.nan)
            if rhat_method == "moments":
                return _rhat(x, self.ensembles, discard=discard)
            return _rhat(x, self.ensembles, discard=discard, method=rhat_method)

        def check(rows, tau, rh=None):
            """the books of one check -> stop?"""
            tau = np.asarray(tau, dtype=float)
            info["history"].append((rows, tau) if rhat is None else (rows, tau, rh))
            info["rows"], info["tau"] = rows, tau
            if rhat is not None:
                info["rhat"] = rh
            if np.any(np.isnan(tau)) and not warned:
                warned.append(True)
                warnings.warn("the autocorrelation time of a parameter is NaN (a constant walker "
                              "or a non-finite value): the run cannot converge")
            info["converged"] = autocorr.converged(tau, old[0], rows - discard, tol, rtol) and \
                (rhat is None or bool(np.all(rh < rhat)))  # (a NaN R-hat never passes)
            old[0] = tau
            return info["converged"]

        if self.device and self._dev is None and self._device_ok is None:
            self._device_ok = self._probe_device(initial_state)
        if self.device and self._device_ok is not False:
            from .device_sampler import DeviceLoop
            if self._dev is None:
                self._dev = DeviceLoop(self)
            info["where"] = "device"
            ra = autocorr.RunningAutocorr(self.nwalkers, self.ndim, max_lag, c)

            def on_check(buf, rows):
                if rows <= discard:
                    return False
                ra.update(buf, rows, discard)
                tau = ra.tau()[0]
                info["max_lag"], info["rebuilds"] = ra.max_lag, ra.rebuilds
                if rhat is None:
                    return check(rows, tau)
                # from the block where it lies: only the moments come to the host
                return check(rows, tau, gelman_rubin((buf, rows, self.nwalkers, self.ndim), rows))

            state = self._dev.sample_monitored(initial_state, max_steps, check_every, thin_by,
                                               on_check)
        else:
            state, rows, it0 = initial_state, 0, self.iteration
            while rows < max_steps:
                g = min(check_every, max_steps - rows)
                state = self.run_mcmc(state, g, thin_by=thin_by)
                rows += g
                if rows <= discard:
                    continue
                x = self.get_chain()[it0:]
                if check(rows, autocorr.integrated_time(x[discard:], c=c, tol=0),
                         None if rhat is None else gelman_rubin(x, rows)):
                    break
        return state

# --------------------------------------------------------------------------
# naima's entry points (core.py:220-538)
# --------------------------------------------------------------------------
def _run_mcmc(sampler, pos, nrun, verbose=True, thin_by=1):
    """core.py:127-160: the run with a progress printout every 5 %.  The steps between two
    printouts are one ``run_mcmc`` call, so the device loop replays whole groups of steps
    and the ensemble is only brought to the host for the printouts.  With ``thin_by`` the
    run -- and its printout -- go by stored rows, ``thin_by`` steps each."""
    state = pos
    nrun = int(nrun)
    edges = sorted(set(int(round(x)) for x in np.linspace(0, nrun, 21)))
    for a, b in zip(edges[:-1], edges[1:]):
        if verbose and sampler.comm.rank == 0 and a > 0:
            _print_progress(sampler, state, a, nrun)
        state = sampler.run_mcmc(state, b - a, store=True, thin_by=thin_by)
    return sampler, state


def _print_progress(sampler, state, i, nrun):
    print("\nProgress of the run: {0:.0f} percent ({1} of {2} steps)".format(
        int(100.0 * i / nrun), i, nrun))
    coords = np.asarray(state.coords)
    npars = coords.shape[-1]
    print("                           " + (" ".join(
        ["{%i:-^15}" % k for k in range(npars)])).format(*sampler.labels))
    print("  Last ensemble median : " + (" ".join(
        ["{%i:^15.3g}" % k for k in range(npars)])).format(*np.median(coords, axis=0)))
    print("  Last ensemble std    : " + (" ".join(
        ["{%i:^15.3g}" % k for k in range(npars)])).format(*np.std(coords, axis=0)))
    lp = np.asarray(state.log_prob)
    print("  Last ensemble lnprob :  avg: {0:.3f}, max: {1:.3f}".format(np.average(lp), np.max(lp)))


def _prefit(p0, data, model, prior):
    """Nelder-Mead maximum-likelihood prefit (core.py:163-217).  Same algorithm, options
    (maxfev 500, relative xtol 0.1, ftol 1e-3) and acceptance rules as the reference; the
    candidate points of each simplex iteration are evaluated as one walker batch
    (naima_amd.neldermead)."""
    from .core import lnprob
    from .neldermead import minimize_batched
    P0_IS_ML = False

    def flat_prior(*args):
        return 0.0

    if prior is None:
        prior = flat_prior

    def nll(X):  # (m, ndim) points -> m values of -lnprob under the flat prior
        X = np.atleast_2d(np.asarray(X, dtype=float))
        return -np.asarray(lnprob(np.ascontiguousarray(X.T), data, model, flat_prior)[0],
                           dtype=float).reshape(-1)

    res = minimize_batched(nll, p0, maxfev=500, xtol=1e-1, ftol=1e-3)
    ll_prior = float(np.asarray(lnprob(res["x"], data, model, prior)[0]))
    if (res["success"] or res["status"] == 1) and not np.isinf(ll_prior):
        # also kept when maxfev was reached: likely better than p0 (core.py:193-195)
        P0_IS_ML = res["status"] != 1
        p0 = res["x"]
    return p0, P0_IS_ML


def get_sampler(data_table=None, p0=None, model=None, prior=None, nwalkers=500, nburn=100,
                guess=True, interactive=False, prefit=False, labels=None, threads=None,
                data_sed=None, seed=None, comm=None, verbose=True, store_blobs=True,
                device=True, ensembles=1):
    """Generate a new MCMC sampler (signature of core.py:220-233; ``threads`` is
    accepted and ignored -- the walkers of a half-ensemble are one GPU batch;
    ``interactive`` is out of scope).  ``device=True`` (default): the ensemble and the step
    loop live on the GPU (models that cannot keep their parameters in HBM fall back to the
    host-driven loop with a warning).  Returns (sampler, state).

    ``ensembles`` = k > 1: the ``nwalkers`` walkers are k independent ensembles of nwalkers / k
    that share every launch (``EnsembleSampler``), for a Gelman-Rubin comparison
    (``sampler.get_rhat``, ``run_sampler(converge=dict(rhat=1.01))``).  ``p0`` of shape (k, ndim)
    starts each ensemble from its own row -- dispersed starts, what the comparison is for -- and
    implies ``ensembles=k``; ``guess`` and ``prefit`` are applied to each row.  A 1-D ``p0`` starts
    all of them round the same point.  Ensemble r's ball is drawn from
    ``np.random.default_rng(sampler.seeds[r])``: the ball of a single-ensemble
    ``get_sampler(seed=seeds[r])`` from the same point."""
    from .core import lnprob, sed_conversion
    from .datatable import validate_data_table
    if data_table is None:
        raise TypeError("Data table is missing!")
    data = validate_data_table(data_table, sed=data_sed)
    if model is None:
        raise TypeError("Model function is missing!")
    p0 = np.array(p0, dtype=float)
    if p0.ndim == 2 and len(p0) == 1:  # (one row: the 1-D call, books included)
        p0 = p0[0]
    if p0.ndim == 2:
        if ensembles not in (1, len(p0)):
            raise ValueError("p0 has %d rows for %d ensembles" % (len(p0), ensembles))
        ensembles = len(p0)
    elif p0.ndim != 1:
        raise ValueError("p0 must be (ndim,) or (ensembles, ndim)")
    ensembles = int(ensembles)
    starts = p0 if p0.ndim == 2 else p0[np.newaxis].repeat(max(1, ensembles), axis=0)
    ndim = starts.shape[1]
    if labels is None:
        labels = ["norm"] + ["par{0}".format(i) for i in range(1, ndim)]
    elif len(labels) < ndim:
        labels = list(labels) + ["par{0}".format(i) for i in range(len(labels), ndim)]

    def start(p0):
        """one starting point -> (the point after ``guess`` and ``prefit``, is it an ML point?)"""
        p0 = p0.copy()
        modelout = model(p0, data)
        spec = modelout[0] if isinstance(modelout, (tuple, list)) else modelout
        try:  # core.py:352-376: model and data must be convertible to differential flux
            sed_conversion(data["energy"], spec.unit, False)
            sed_conversion(data["energy"], data["flux"].unit, False)
        except u.UnitsError:
            raise u.UnitsError(
                "The physical type of the model and data units are not compatible, please modify "
                "your model or data so they match:\n Model units: {0} [{1}]\n Data units: {2} [{3}]\n"
                .format(spec.unit, spec.unit.physical_type, data["flux"].unit,
                        data["flux"].unit.physical_type))

        if guess:  # core.py:378-419
            normNames = ["norm", "ampl", "we", "wp"]
            normNames += ["log({0}".format(n) for n in normNames[:4]] + \
                         ["log10({0}".format(n) for n in normNames[:4]]
            idxs = []
            for nn in normNames:
                for l2 in labels:
                    if l2.lower().startswith(nn):
                        idxs.append(labels.index(l2))
            if len(idxs) == 1:
                e = data["energy"]
                nunit, sedf = sed_conversion(e, spec.unit, False)
                currFlux = np.trapezoid(e.value * (spec * sedf).to(nunit).value, e.value)
                nunit, sedf = sed_conversion(e, data["flux"].unit, False)
                dataFlux = np.trapezoid(e.value * (data["flux"] * sedf).to(nunit).value, e.value)
                ratio = dataFlux / currFlux
                if labels[idxs[0]].startswith("log("):
                    p0[idxs[0]] += np.log(ratio)
                elif labels[idxs[0]].startswith("log10("):
                    p0[idxs[0]] += np.log10(ratio)
                else:
                    p0[idxs[0]] *= ratio

        if prefit:
            return _prefit(p0, data, model, prior)
        return p0, False

    started = [start(row) for row in (starts if p0.ndim == 2 else starts[:1])]
    if p0.ndim == 1:
        started = started * len(starts)
    p0 = started[0][0] if p0.ndim == 1 else np.array([q for q, _ in started])

    sampler = EnsembleSampler(nwalkers, ndim, lnprob, args=[data, model, prior], seed=seed,
                              comm=comm, naima_style=True, store_blobs=store_blobs,
                              device=device, ensembles=ensembles)
    sampler.data_table = data_table
    sampler.data = data
    sampler.labels = labels
    sampler.modelfn = model
    sampler.run_info = {"n_walkers": nwalkers, "n_burn": nburn,
                        "p0": np.asarray(p0, dtype=float).tolist(), "guess": guess,
                        "ensembles": ensembles, "seeds": list(sampler.seeds)}
    # ball of 0.5 % (ML start) or 10 % around p0 (core.py:477-481), drawn from the
    # sampler's replicated stream so that every rank starts from the same ensemble; several
    # ensembles: each from the stream of its own seed
    n = nwalkers // ensembles
    pos = np.concatenate([
        q + (0.005 if is_ml else 0.1) * q *
        (sampler._rng if ensembles == 1 else np.random.default_rng(sd)).normal(size=(n, ndim))
        for (q, is_ml), sd in zip(started, sampler.seeds)])
    if nburn > 0:
        if verbose and sampler.comm.rank == 0:
            print("Burning in the {0} walkers with {1} steps...".format(nwalkers, nburn))
        sampler, state = _run_mcmc(sampler, pos, nburn, verbose)
    else:
        state = State(pos)
    sampler.run_info["p0_burn_median"] = [float(p) for p in np.median(state.coords, axis=0)]
    return sampler, state


def run_sampler(nrun=100, sampler=None, pos=None, verbose=True, thin_by=1, converge=None,
                **kwargs):
    """Run an MCMC sampler (core.py:496-538).  ``thin_by`` = t (emcee's): ``nrun`` is the number
    of STORED rows, each t ensemble steps after the one before; ``run_info["thin_by"]`` records
    it.  The burn-in of ``get_sampler`` is not thinned.

    ``converge`` = True, or a dict of ``EnsembleSampler.run_until_converged``'s keywords
    (``check_every``, ``tol``, ``rtol``, ``c``, ``discard``, ``max_lag``, ``rhat``, ``rhat_method``): ``nrun`` is then
    the MAXIMUM, the run stops once the autocorrelation time has converged, and ``run_info`` gains
    ``converged`` and ``autocorr_time`` (in stored rows).  With ``rhat`` (a sampler of several
    ensembles) the Gelman-Rubin statistic across them must also lie below it; ``run_info`` gains
    ``rhat``, the last check's value per parameter (and ``rhat_method`` when it is not the
    moments statistic)."""
    thin_by = int(thin_by)
    if thin_by <= 0:
        raise ValueError("Invalid thinning argument")
    if sampler is None or pos is None:
        sampler, pos = get_sampler(verbose=verbose, **kwargs)
    sampler.run_info["n_run"] = nrun
    sampler.run_info["thin_by"] = thin_by
    if verbose and sampler.comm.rank == 0:
        print("\nWalker burn in finished, running {0} steps...".format(nrun) if thin_by == 1 else
              "\nWalker burn in finished, running {0} steps, keeping every {1}th..."
              .format(nrun * thin_by, thin_by))
    sampler.reset()
    t0 = time.time()
    if isinstance(pos, State):
        pos = State(pos.coords)
    elif not hasattr(pos, "_loop"):  # (a DeviceState continues from the ensemble in HBM)
        pos = State(pos)
    if converge:
        opts = dict(converge) if isinstance(converge, dict) else {}
        pos = sampler.run_until_converged(pos, int(nrun), thin_by=thin_by, **opts)
        conv = sampler.convergence
        sampler.run_info["converged"] = bool(conv["converged"])
        sampler.run_info["autocorr_time"] = [float(t) for t in conv["tau"]]
        if "rhat" in conv:
            sampler.run_info["rhat"] = [float(t) for t in conv["rhat"]]
            if conv["rhat_method"] != "moments":
                sampler.run_info["rhat_method"] = conv["rhat_method"]
        if verbose and sampler.comm.rank == 0:
            print("{0} after {1} of at most {2} steps; autocorrelation time: {3}".format(
                "Converged" if conv["converged"] else "Not converged", conv["rows"], int(nrun),
                conv["tau"]) + ("; R-hat: {0}".format(conv["rhat"]) if "rhat" in conv else ""))
    else:
        sampler, pos = _run_mcmc(sampler, pos, nrun, verbose, thin_by)
    sampler.run_info["wall_s"] = time.time() - t0
    return sampler, pos
