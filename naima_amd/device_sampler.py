"""The device-resident step loop of ``EnsembleSampler(device=True)``.

State in HBM: coords[N][ndim], logp[N], the current blobs, per-walker acceptance
counters, and the chain history.  Per half-step the host only draws the random
numbers of the move (replicated numpy stream: identical on every rank and identical
to the host-path sampler), ships them as two small blocks, and launches ONE hipGraph:

    nh_move_propose -> [the launch sequence the naima model function produces:
    nh_pack_rows, nh_particle_weights, nh_integrate_tables, nh_synchrotron, ...]
    -> nh_priors -> nh_lnprob -> (RCCL all-gather when sharded) -> nh_move_accept
    -> nh_scatter_rows (blobs)

The graph is captured from the FIRST replay of the user's unchanged Python model
function on lazy device parameters (``naima_amd.darray``); walker-independent
pieces (grids, emission tables, data columns) are evaluated during a warm-up pass,
land in the context's caches, and are therefore not part of the graph.  After
capture no Python model code runs inside the loop.
"""
import collections
import ctypes as C
import functools
import os
import warnings
import weakref

import numpy as np

from . import _lib, loop_books, shared_merge
from .step_plan import AcceptHook, Front, StepPlan
from . import units as u
from .darray import DFactor, DMat, DPars, DVec, lift_factor
from .dist import shard_bounds, shard_counts
from .loop_books import Books, EnsembleCopy, JournalEntry, KeptBlob, LaunchQueue
from .move_ring import MoveRing

_GAVE_UP = ("a launch of the resident loop gave up waiting for a walker's record (status %d): its "
            "workgroups were not all resident")


class DeviceState:
    """what the loop yields: host views are fetched on first access"""

    def __init__(self, loop, rng):
        self._loop, self.random_state = loop, rng
        self._c = self._l = None

    @property
    def coords(self):
        if self._c is None:
            self._loop._before_read()
            self._c = self._loop.coords.get().reshape(self._loop.N, self._loop.ndim)
        return self._c

    @property
    def log_prob(self):
        if self._l is None:
            self._loop._before_read()
            self._l = self._loop.logp.get()
        return self._l

    @property
    def blobs(self):
        return self._loop.host_blobs()

    def __iter__(self):
        return iter((self.coords, self.log_prob, self.random_state))


def _release_loop(ctx, res):
    """finalizer of a DeviceLoop: its graph executables, then the half-step plan they launch
    (device packs, counters, partial-spectra buffers, the host descriptor)"""
    if ctx.h is None:
        return  # the context went first and took the device allocations with it
    if ctx.capturing:
        # (the collector may run this in the middle of ANOTHER loop's stream capture, which a
        # synchronisation would invalidate: the context releases it after the capture)
        ctx._release_later.append(functools.partial(_release_loop, ctx, res))
        return
    try:
        ctx.sync()
        for g in res["graphs"]:
            _lib._lib.nh_graph_destroy(ctx.h, g)
        for r in res.get("runs", []):
            _lib._lib.nh_half_step_run_destroy(ctx.h, r)
        res["runs"] = []
        for plan in res["plans"]:
            plan.destroy(ctx)
    except Exception:
        pass
    res["graphs"], res["plans"] = [], []


class DeviceLoop:
    def __init__(self, sampler):
        if not sampler.naima_style:
            raise ValueError("device=True needs naima_style=True (lnprob(pars, data, model, prior))")
        self.s = sampler
        self.ctx = _lib.get_context()
        self.N, self.ndim = sampler.nwalkers, sampler.ndim
        self.ns = self.N // 2
        comm = sampler.comm
        if self.ns < comm.size:
            raise ValueError("device=True needs at least one walker of every half-ensemble (%d) "
                             "per rank (%d)" % (self.ns, comm.size))
        # (a half-ensemble that does not divide evenly: the first ranks take one walker more,
        # as dist.shard_bounds says; all-gathers then travel padded to the largest block)
        self.lo, self.hi = shard_bounds(self.ns, comm.rank, comm.size)
        if comm.size > 1 and getattr(comm, "group", None) is not None:
            # ranks that sit on ONE device (a multi-GPU run rehearsed on a one-GPU box) each plan
            # for their share of its CUs -- or their resident launches cannot all be resident
            # together and the first shared launch gives up.  Who shares a device is read off the
            # ranks' PCI bus ids (collective: every rank, always); NAIMA_AMD_CU_SHARE overrides.
            ids = [p_.decode() for p_ in comm.group.allgather_bytes(self.ctx.pci_bus_id().encode())]
            share = max(collections.Counter(ids).values())
            if share > 1 and not os.environ.get("NAIMA_AMD_CU_SHARE"):
                os.environ["NAIMA_AMD_CU_SHARE"] = str(share)
        self._pads = {}
        # the sharded code path (split graphs around the all-gather) even for ONE rank:
        # lets a 1-GPU box run everything but the multi-process part (tests)
        self.sharded = comm.size > 1 or os.environ.get("NAIMA_AMD_FORCE_SHARDED", "0") == "1"
        # the all-gather captured INTO the step graphs (the sharded loop then replays whole
        # steps like the single-GPU loop) when the communicator's ranks have been seen to
        # survive that in a throw-away probe process (RcclComm.graph_capture_ok); else the
        # collective sits between two graphs.  NAIMA_AMD_RCCL_IN_GRAPH = auto | 0 | 1
        mode = os.environ.get("NAIMA_AMD_RCCL_IN_GRAPH", "auto")
        # (several ranks normally take the resident loop over the shared ensemble after a few
        # steps, and these launches around an all-gather are only its run-in and its fallback:
        # "auto" then does not spend a probe process per rank on them)
        shared_expected = (comm.size > 1 and getattr(comm, "group", None) is not None and
                           os.environ.get("NAIMA_AMD_SHARED", "1") != "0" and
                           os.environ.get("NAIMA_AMD_RESIDENT", "1") != "0" and sampler.use_graph)
        self.coll_in_graph = self.sharded and getattr(comm, "in_stream", False) and (
            mode == "1" or (mode == "auto" and not shared_expected and
                            hasattr(comm, "graph_capture_ok") and comm.graph_capture_ok()))
        self.split = self.sharded and not self.coll_in_graph  # collective between two graphs
        self.nloc = self.hi - self.lo
        ctx = self.ctx
        self.coords = ctx.empty((self.N * self.ndim,))
        self.logp = ctx.empty((self.N,))
        # ensemble steps per hipGraph launch when the host has nothing to do
        self.GSTEPS = max(1, int(os.environ.get("NAIMA_AMD_GSTEPS", "8")))
        self.multi_graph = None
        # the move stream on the device; a device cursor selects the current half-step's slice
        # of `blk` (advanced by the accept kernel)
        self.ring = MoveRing(ctx, self.ns)
        self.blk = self.ring.blk
        # nh_step_front mode: set after a recording evaluation when the model's parameter
        # packs read the proposal buffer and it asks for ONE particle-weights launch
        self.fused = False
        # ... and, when every launch of the model evaluation is one nh_half_step can absorb
        # (table reductions, a synchrotron component, the likelihood), the whole half-step is
        # ONE launch: proposal -> ... -> accept (NAIMA_AMD_MEGA=0 keeps the three launches)
        self.mega = False
        # next slice of the current block of moves / history rows before that block: what a
        # half-step plan created in the middle of a block has to be told
        self._pos = dict(slice=0, steps=0, bake=False)
        self.multi_graphs = {}
        self._plan = None
        self.done = ctx.empty((1,), dtype=np.int32)
        ctx.call("nh_memset", self.done, 0, 4)
        self._hook = None
        # nh_hist descriptor in HBM: the fused kernel appends the chain history itself
        # ... followed, in the one-launch mode, by the blobs' histories (device words holding
        # the base of each blob's history of the current call; 0: not kept).  Eight words in
        # one buffer: a call of sample() re-points all of them with ONE small launch
        # (nh_set_words) instead of two staged uploads
        self.histd = ctx.empty((8,), dtype=np.int64)
        ctx.call("nh_memset", self.histd, 0, self.histd.nbytes)
        self.blobhist_ptr = self.histd.ptr + 32
        self.blobs_in_kernel = False
        self.send_width = 0
        self.cursor = ctx.empty((1,), dtype=np.int32)
        self.sel = ctx.empty((self.ns,), dtype=np.int32)
        self.qT = ctx.empty((self.ndim * self.nloc,))
        self.factors = ctx.empty((self.nloc,))
        self.newlp = ctx.empty((self.ns,))
        self.mylp = ctx.empty((max(self.nloc, 1),))
        self.new_blobs = None
        self.all_blobs = None
        self.ident = ctx.array(np.arange(max(self.nloc, 1), dtype=np.int32), dtype=np.int32)
        self.graph2 = None
        self.graph21 = None
        self._pending = False
        self.step_graph = None
        self.accepted = ctx.empty((self.ns,), dtype=np.int32)
        self.nacc = ctx.empty((self.N,), dtype=np.int32)
        ctx.call("nh_memset", self.nacc, 0, self.nacc.nbytes)
        self.graph = None
        self.cur_blobs = None      # list of loop_books.KeptBlob
        self.const_blobs = []      # (position, value) of blobs that are plain numbers
        self.hist = []             # pending device history blocks
        self.warm = 0
        self._have_state = False
        # what this loop owns on the device besides pooled buffers: released when it goes
        self._res = dict(graphs=[], plans=[], runs=[])
        # the resident loop (nh_half_step_run: a whole block of moves per launch, walkers handed
        # from half-step to half-step by per-walker records): None = not tried yet, False = this
        # plan / configuration cannot (or NAIMA_AMD_RESIDENT=0), else the handle
        self._run = None if os.environ.get("NAIMA_AMD_RESIDENT", "1") != "0" else False
        self._resident_trust = 0          # launches of the resident loop that were checked as they were made
        self.resident_failed_launches = 0
        # launches of a one-GPU resident loop that are not yet known to have ended well: the
        # sampler queues launch n + 1 only once launch n - 1 is (nh_half_step_run_report: page-
        # locked memory the launch's epilogue writes, no stream operation), and settles all of
        # them before a call returns -- a launch that gave up later in a run costs the replay of
        # two blocks of moves at most, by the per-launch kernel (sample)
        self._rl = LaunchQueue()
        # copies of the current blobs as a launch WITHOUT a history found them (such a launch
        # writes the blobs of accepted moves straight into the current-blob arrays): what a
        # launch that gave up -- or ran void behind one that did -- is rolled back to
        self._cur_snaps = [None] * 4
        self._nan_pending = self._forbidden_pending = 0
        self._read_counts(reset=True)  # (the context's words may hold what an earlier sampler left)
        self.resident_launches = 0
        # ... and over an ensemble shared by several GPUs (nh_half_step_run_create_shared: movers
        # store their walkers' records into every rank's ring; no collective per half-step).
        # What a rank's launches leave on ITS device only -- the history rows and blobs of the
        # moves it made, their acceptance counts, the blobs' current values (stamped) -- is
        # merged over the control plane when somebody reads it
        self.shared = False
        self.shared_info = None
        self._cur_dirty = False   # current blobs differ between ranks (merge by stamp pending)
        self._cur_host = None     # host copies of the current blobs while nothing has changed them
        self._acc_dirty = False   # shared launches have accepted moves since the counts were summed
        self._acc_shared = 0.0
        self._acc_base = 0.0      # moves accepted by the launches of a shared loop that was given up
        # A shared ensemble's launches are not checked one by one (that would be a collective per
        # launch): every rank keeps the ensemble as it stood at the last point where ALL ranks were
        # known to be well (flush, reset: `verified`), and a journal of the sample() calls made
        # since.  A launch that gave up on any rank is found at the next such point -- the status
        # reduction every rank takes part in -- and the ranks TOGETHER go back to the kept ensemble
        # and make the journal's steps again with one launch and one all-gather per half-step
        # (the reference's Pool carries on when a worker is slow, core.py:523-536; this used to be
        # an exception on every rank)
        # what has changed the device state (initial states uploaded, steps queued), and its value
        # at the last full flush (None: none since the last reset) -- see flush
        self._changes, self._flushed_at = 0, None
        self._sh_snap = None
        self._sh_want = False
        self._sh_journal = []
        self._replaying = False
        # what the last call with thin_by > 1 did (_sample_thinned): thin_by, where the rows were
        # thinned, the staging block's rows and bytes, the internal calls as (steps, rows written)
        self.thin_info = None
        self._finalizer = weakref.finalize(self, _release_loop, self.ctx, self._res)

    @property
    def _hs(self):
        """the created one-launch plan (step_plan.OneLaunch), None while there is none"""
        return self._plan.hs if self._plan else None

    # ------------------------------------------------------------------ pieces
    def reset(self):
        """forget the chain and the acceptance counts (the sampler clears its host copies): the
        history still on the device is dropped, not downloaded"""
        self._meet()
        self.hist = []
        self.ctx.call("nh_memset", self.nacc, 0, self.nacc.nbytes)
        if self.shared:
            _lib._chk(_lib._lib.nh_half_step_run_counters(self.ctx.h, self._run, None, None, 1))
            self._acc_dirty, self._acc_shared = False, 0.0
        self._acc_base = 0.0
        self._flushed_at = None

    def _meet(self):
        """where every rank is (flush, reset): what only all of them together can find or mend"""
        self._flush_pending()
        self.check_resident(collective=True)
        self.check_nan(collective=True)
        self.ctx.check_general()  # (a per-walker grid longer than the general kernel's LDS)
        self._sync_cur_blobs()

    def _eval(self, qT_buf, n):
        """run the user's model on device parameters: (total DVec, blob list)"""
        pars = DPars(self.ctx, qT_buf, self.ndim, n)
        self.ctx._in_eval = True
        try:
            res = self.s.log_prob_fn(pars, *self.s.args)
        finally:
            self.ctx._in_eval = False
        self.s.n_lnprob_calls += 1
        self.s.n_walker_evals += n
        rows = bool(self._hook and self._hook.rows_active) and self.ctx._accept_hook is self._hook
        total = res[0] if rows else res[0].dense()  # (rows: exchanged as they are)
        blobs = [lift_factor(b, n) for b in res[1:]]
        # plain numbers among the blobs (lnprob's (model, nan) for a model that returns no
        # blob of its own, core.py:108-110) are the same for every walker and every step:
        # they are not kept in HBM but put back where they belong when the blobs are read
        self.const_blobs = [(j, float(b)) for j, b in enumerate(blobs)
                            if isinstance(b, (float, int))]
        return total, [b for b in blobs if not isinstance(b, (float, int))]

    def _blob_dense(self, b):
        """blob -> (owner, ptr, m, unit, trailing shape) with rows over walkers"""
        unit = None
        if isinstance(b, u.Quantity):
            b, unit = b.value, b.unit
        if isinstance(b, DFactor):  # (a transmission blob: its rows gathered, one launch)
            b = b.apply()
        if isinstance(b, DMat):
            own, ptr = b.buffer()
            return own, ptr, b.shape[1], unit, (b.shape[1],)
        if isinstance(b, DVec):
            d = b.dense()
            return d, d.ptr, 1, unit, ()
        raise TypeError("blob of type %s cannot be kept on the device" % type(b).__name__)

    def _part_evaluate(self):
        """propose this rank's block and evaluate it: everything up to the new
        log-probabilities (the part that precedes the exchange)"""
        ctx = self.ctx
        if self.fused:
            # proposal, parameter rows, weights, We: written by the preceding nh_step_front
            self._plan.rewind()
            ctx._plan = self._plan
            self._hook.used = False
            ctx._accept_hook = self._hook
        else:
            ctx.call("nh_move_propose", self.coords, self.blk, self.cursor, self.ns, self.ndim,
                     self.lo, self.nloc, self.qT, self.factors)
        try:
            total, blobs = self._eval(self.qT, self.nloc)
        finally:
            ctx._plan = None
            ctx._accept_hook = None
            ctx.flush()  # a held-back launch nobody consumed
        if self.sharded:
            # fixed hand-over buffer so that the two graphs and the collective between
            # them always see the same addresses
            if self._hook and self._hook.rows_active:
                pass  # rows { lnprob | blobs } are exchanged as the launch wrote them
            elif total.ptr != self.mylp.ptr:  # (the fused likelihood wrote it there itself)
                ctx.call("nh_copy", self.mylp, total.ptr, 8 * self.nloc)
            self._newlp_ptr = self.newlp.ptr
        else:
            self._total = total  # single rank: the accept kernel reads it in place
            self._newlp_ptr = total.ptr
        self._stage_blobs(blobs)

    def _stage_blobs(self, blobs):
        """copy the proposal's blobs into fixed staging buffers (only when kept)"""
        if not (self.s.store_blobs and self.cur_blobs):
            return
        if self.mega and self._hook.blobs_in_kernel:
            self.blobs_in_kernel = True  # the half-step launch keeps the blobs itself
            return
        if self.new_blobs is None:
            self.new_blobs = [self.ctx.empty((self.nloc, b.m)) for b in self.cur_blobs]
            if self.sharded:  # every rank keeps every walker's blobs
                self.all_blobs = [self.ctx.empty((self.ns, b.m)) for b in self.cur_blobs]
        for nb, kept, b in zip(self.new_blobs, self.cur_blobs, blobs):
            own, ptr, mb, _, _ = self._blob_dense(b)
            self.ctx.call("nh_scatter_rows", nb, kept.m, ptr, mb, self.ident, None, 0, self.nloc,
                          kept.m)
            del own

    def _part_accept(self):
        ctx = self.ctx
        if self.fused and self.sharded and self.blobs_in_kernel and self.send_width:
            nb = len(self.cur_blobs)
            cur = (C.c_void_p * nb)(*[b.cur.ptr for b in self.cur_blobs])
            mm = (C.c_int * nb)(*[b.m for b in self.cur_blobs])
            ctx.call("nh_move_accept_rows", self.coords, self.logp, self.blk, self.cursor,
                     self.recv_rows, self.send_width, self.ns, self.ndim, self.accepted, self.nacc,
                     self.sel, 0, nb, cur, mm)
        elif not (self.fused and self._hook and self._hook.used and self._hook.mv is not None):
            # not accepted by the likelihood's own launch: the separate kernels (which also advance
            # the cursor: 1), sharded (the accept waits for the all-gather), a foreign likelihood
            ctx.call("nh_move_accept", self.coords, self.logp, self.blk, self.cursor,
                     self._newlp_ptr, self.ns, self.ndim, self.accepted, self.nacc, self.sel,
                     0 if self.fused else 1)
        if self.s.store_blobs and self.cur_blobs and not self.blobs_in_kernel:
            src, lo, n = (self.all_blobs, 0, self.ns) if self.sharded else \
                (self.new_blobs, self.lo, self.nloc)
            for b, kept in zip(src, self.cur_blobs):
                ctx.call("nh_scatter_rows", kept.cur, kept.m, b, kept.m, self.sel, self.accepted,
                         lo, n, kept.m)
        if self.fused and not self.mega:
            self._front()

    def _front(self):
        """proposal of the next half-step + parameter packs + particle weights + We/Wp
        reductions (+ chain history, cursor advance): one launch"""
        self.ctx.call("nh_step_front", self.coords, self.logp, self.blk, self.cursor, self.done,
                      self.ns, self.ndim, self.lo, self.nloc, self.qT, self.factors,
                      *self._plan.front.step_front_args(), self.histd)

    def _record_half_step(self):
        """a half-step launched piece by piece while the model's parameter packs, weights
        launch and single-row reductions are recorded; if nh_step_front can produce them
        the loop switches to it"""
        from .darray import nh_accept, nh_grid, nh_lazy, nh_moment, nh_pack
        ctx = self.ctx
        plan = ctx._plan = StepPlan()
        try:
            self._half_step_body()
        finally:
            ctx._plan = None
        if not self.s.fuse_moves:
            return
        packs, weights, moments = plan.packs, plan.weights, plan.moments
        if not (1 <= len(packs) <= 4 and len(weights) == 1 and len(moments) <= 4):
            return
        lo_a = self.qT.ptr
        hi_a = lo_a + 8 * self.ndim * self.nloc
        pk = (nh_pack * 4)()
        for q, ((raw, ncols, N), out) in enumerate(packs):
            cols = (nh_lazy * 8).from_buffer_copy(raw.ljust(C.sizeof(nh_lazy) * 8, b"\0"))
            if N != self.nloc or ncols > 8:
                return
            for j in range(ncols):
                base = cols[j].base or 0
                if base and not (lo_a <= base < hi_a and (base - lo_a) % (8 * self.nloc) == 0
                                 and cols[j].stride == 1):
                    return
            pk[q].cols = cols
            pk[q].ncols, pk[q].ld, pk[q].out = ncols, ncols, out.ptr
        (kind, rows_ptr, N, grids), bufs = weights[0]
        if N != self.nloc or rows_ptr not in [out.ptr for _, out in packs] or len(grids) > 4:
            return
        gd = (nh_grid * 4)()
        wptr = {}
        for g, ((e, x, lne, lx, scale, nG), (wk, lwk)) in enumerate(zip(grids, bufs)):
            gd[g] = nh_grid(e, x, wk.ptr, lwk.ptr, scale, nG, 0, lne, lx)
            wptr[wk.ptr] = g
        mm = (nh_moment * 4)()
        lds_nodes = set()
        for k, ((w, lw, N, nG, lx, Kt, dlnKt), out) in enumerate(moments):
            if w not in wptr or N != self.nloc:
                return
            mm[k] = nh_moment(wptr[w], 0, Kt, dlnKt, out.ptr)
            lds_nodes.add(wptr[w])
        if 40 * sum(grids[g][5] for g in lds_nodes) * max(len(moments), 1) > 48 * 1024:
            return
        plan.replaying = True
        ctx.pin_caches()
        self._plan = plan
        self._res["plans"].append(plan)
        # (pos: the loop's own dict, changed as the loop goes and read when a launch is made)
        plan.front = Front(self.coords.ptr, self.logp.ptr, self.blk.ptr, self.cursor.ptr, self._pos,
                           self.qT.ptr, self.factors.ptr, self.histd.ptr, self.accepted.ptr,
                           self.nacc.ptr, self.sel.ptr, self.ns, self.ndim, self.lo, self.nloc,
                           pk, len(packs), kind, rows_ptr, gd, len(grids), mm, len(moments))
        if not self.sharded:
            self._hook = AcceptHook(self.nloc, mv=nh_accept(
                self.coords.ptr, self.logp.ptr, self.blk.ptr, self.cursor.ptr, self.ns, self.ndim,
                self.lo, 0, self.accepted.ptr, self.nacc.ptr, self.sel.ptr))
        else:  # sharded: likelihood into the all-gather send buffer, accept afterwards
            self._hook = AcceptHook(self.nloc, total=self.mylp)
        self.fused = True
        self.mega = plan.mega = plan.can_be_one_launch(self.nloc)
        if self.mega:
            if self._hook.total is None:
                self._hook.total = ctx.empty((self.nloc,))  # persistent: the plan points at it
            if self.s.store_blobs and self.cur_blobs:
                self._hook.blobs = [(b.cur.ptr, b.m, self.blobhist_ptr + 8 * i)
                                    for i, b in enumerate(self.cur_blobs)]
                if self.sharded:
                    # the blobs travel with the log-probabilities: ONE all-gather of rows
                    # { lnprob | blob 0 | blob 1 ... } per half-step
                    self.send_width = 1 + sum(b.m for b in self.cur_blobs)
                    self._hook.send_width = self.send_width
                    self.send_rows = ctx.empty((max(self.nloc, 1), self.send_width))
                    self.recv_rows = ctx.empty((self.ns, self.send_width))
                    self._hook.total_rows = self.send_rows
        # new slice protocol: cursor = the slice accepted last.  The two piecewise
        # half-steps (slices 0 and 1 of the first block) left it at 2.
        self.cursor.set(np.array([1], dtype=np.int32))
        if not self.mega:
            self._front()

    def _gather_rows(self, send_ptr, recv, n, width):
        """all-gather of rows of `width` doubles, rank r contributing its block of the n rows
        (dist.shard_counts); blocks of unequal length travel padded to the longest and are put
        side by side on arrival (one small copy per rank, in stream order)"""
        ctx, comm = self.ctx, self.s.comm
        counts = shard_counts(n, comm.size)
        if len(set(counts)) == 1:
            comm.allgather_device(ctx, send_ptr, recv, counts[0] * width)
            return
        m = max(counts)
        key = (m * width, comm.size)
        if key not in self._pads:
            self._pads[key] = (ctx.empty((m * width,)), ctx.empty((comm.size * m * width,)))
        ps, pr = self._pads[key]
        ctx.call("nh_copy", ps, send_ptr, 8 * counts[comm.rank] * width)
        comm.allgather_device(ctx, ps.ptr, pr, m * width)
        off = 0
        for r, cnt in enumerate(counts):
            ctx.call("nh_copy", recv.ptr + 8 * off * width, pr.ptr + 8 * r * m * width,
                     8 * cnt * width)
            off += cnt

    def _exchange(self):
        """the one collective of the path: every rank's new log-probabilities"""
        if self.sharded and self.blobs_in_kernel and self.send_width:
            self._gather_rows(self.send_rows.ptr, self.recv_rows, self.ns, self.send_width)
        elif self.sharded:
            self._gather_rows(self.mylp.ptr, self.newlp, self.ns, 1)
            if self.s.store_blobs and self.cur_blobs:
                # blobs of the proposals follow their log-probabilities: the walker a rank
                # evaluates changes every step, so every rank keeps all of them
                for nb, ab, kept in zip(self.new_blobs, self.all_blobs, self.cur_blobs):
                    self._gather_rows(nb.ptr, ab, self.ns, kept.m)

    def _half_step_body(self):
        self._part_evaluate()
        self._exchange()
        self._part_accept()
        self._pos["slice"] += 1

    def _init_state(self, coords_host, logp_host):
        ctx, s = self.ctx, self.s
        self.coords.set(np.ascontiguousarray(coords_host, dtype=float).ravel())
        if logp_host is not None and self._have_state:
            self.logp.set(np.asarray(logp_host, dtype=float))
            return
        # initial log-probability (and blobs) of the whole ensemble: this rank's block
        lo, hi = shard_bounds(self.N, s.comm.rank, s.comm.size)
        qT = ctx.array(np.ascontiguousarray(coords_host[lo:hi].T))
        total, blobs = self._eval(qT, hi - lo)
        if self.sharded:
            self._gather_rows(total.ptr, self.logp, self.N, 1)
        else:
            ctx.call("nh_copy", self.logp, total.ptr, 8 * self.N)
        if s.store_blobs and blobs:
            # (a later initial state keeps the current-blob arrays: captured graphs and the
            # one-launch plan point at them)
            old, self.cur_blobs, units = self.cur_blobs or [], [], []
            ident = ctx.array(np.arange(lo, hi, dtype=np.int32), dtype=np.int32)
            for i, b in enumerate(blobs):
                own, ptr, m, unit, trail = self._blob_dense(b)
                cur = old[i].cur if i < len(old) and old[i].m == m else ctx.empty((self.N, m))
                if self.sharded:
                    self._gather_rows(ptr, cur, self.N, m)
                else:
                    ctx.call("nh_scatter_rows", cur, m, ptr, m, ident, None, 0, hi - lo, m)
                self.cur_blobs.append(KeptBlob(cur, m, unit, trail))
                units.append(unit)
            s.blob_units = loop_books.with_const_blobs(units, self.const_blobs, lambda v: None)
        lp = self.logp.get()
        if np.any(np.isnan(lp)):
            raise ValueError("Probability function returned NaN")
        self._have_state = True
        self._cur_host = None
        self._changes += 1

    def host_blobs(self):
        if not self.cur_blobs:
            return None
        self._sync_cur_blobs()  # (a shared ensemble: collective -- every rank asks, or none)
        out = [b.cur.get().reshape((self.N,) + b.trail) for b in self.cur_blobs]
        return loop_books.with_const_blobs(out, self.const_blobs, lambda v: np.full((self.N,), v))

    # ------------------------------------------------------------------- loop
    def sample(self, initial_state, iterations, store, yield_every=1, thin_by=1):
        """``iterations`` stored rows of ``thin_by`` ensemble steps each (emcee's thin_by).  The
        launches write every step's row, as the blob bookkeeping of the step kernels needs; with
        thin_by > 1 they write them into a staging block that is reused, and every thin_by-th row
        is copied to the compact block that is kept (_sample_thinned)."""
        s = self.s
        cont = self._adopt(initial_state)
        iterations, thin_by = int(iterations), int(thin_by)
        # several ranks: merging the ranks' rows (shared_merge.merge_history_rows) needs every step's
        # row and flags on the host, so the block stays full-rate and flush slices it after the merge
        host_thin = thin_by > 1 and self.sharded
        jentry = None
        if self.sharded and s.comm.size > 1 and not self._replaying and self._run is not False:
            if self._sh_snap is None or not cont:  # (normally kept at the verified point itself)
                self._shared_snapshot()
            # (the steps the call has MADE, kept up to date as it goes: a caller that breaks out of
            # the generator early must not have the full count replayed -- ADVICE r5)
            jentry = JournalEntry(0, bool(store), yield_every, thin_by)
            self._sh_journal.append(jentry)
        block = None
        if store and iterations > 0 and (thin_by == 1 or host_thin):
            block = self._new_block(iterations * thin_by, shared=self.sharded and s.comm.size > 1,
                                    thin_by=thin_by if host_thin else 1)
            self.hist.append(block)
        if thin_by == 1:
            yield from self._steps(iterations, yield_every, block, jentry)
        else:
            yield from self._sample_thinned(iterations, thin_by, store, yield_every, block, jentry)

    def _adopt(self, initial_state):
        """the ensemble a call starts from -> whether it is the one already in HBM (a DeviceState
        of this loop); any other state is checked, uploaded and evaluated"""
        from .sampler import State
        cont = isinstance(initial_state, DeviceState) and initial_state._loop is self
        if not cont:
            st = State(initial_state)
            if st.coords.shape != (self.N, self.ndim):
                raise ValueError("incompatible input dimensions")
            self._init_state(st.coords, st.log_prob)
            self._sync_cur_blobs()
        return cont

    @property
    def _kept(self):
        """the blobs a call keeps the history of"""
        return (self.cur_blobs or []) if self.s.store_blobs else []

    def _new_block(self, rows, shared=False, thin_by=1):
        """a history block of `rows` rows in HBM: coords, log-prob and every kept blob; `shared`:
        with what the merge of several ranks' rows needs"""
        if shared:
            # a shared ensemble's launches: who moved (and accepted) what, per row; the
            # blobs as they stood before the first row (rows of rejected moves are filled
            # from the row before when the ranks' histories are merged: host copies where the
            # last merge left them, no launch)
            self._sync_cur_blobs()
        return loop_books.new_block(self.ctx, self.N, self.ndim, self._kept, rows, thin_by, shared,
                                    self._cur_host)

    def sample_monitored(self, initial_state, max_rows, check_every, thin_by, on_check):
        """up to ``max_rows`` stored rows into ONE history block of that many rows (the memory of a
        ``run_mcmc(max_rows)`` call), made as internal calls of ``check_every`` rows, each of which
        may take the resident loop and ends with its launches settled (what _steps ends with).
        After each, ``on_check(the block's coordinate buffer, its rows so far)`` looks at the
        chain where it is, in HBM; a true answer ends the call.  With thin_by > 1 the block is the
        compact one, in stored rows (_sample_thinned's staging, one staging block per internal
        call).  The books are those of plain calls: the block is a pending history block like any
        other and holds ``block.n`` rows.  One GPU only -> the last state"""
        s = self.s
        if self.sharded:
            raise NotImplementedError("a monitored run with walkers sharded over several ranks")
        self._adopt(initial_state)
        max_rows, check_every, thin_by = int(max_rows), int(check_every), int(thin_by)
        block = self._new_block(max_rows)
        self.hist.append(block)
        while block.n < max_rows:
            g = min(check_every, max_rows - block.n)
            if thin_by == 1:
                for _ in self._steps(g, 1 << 30, block, None):
                    pass
            else:
                for _ in self._sample_thinned(g, thin_by, True, 1 << 30, None, None, compact=block):
                    pass
            if on_check(block.coords, block.n):
                break
        return DeviceState(self, s._rng)

    def _sample_thinned(self, rows, t, store, yield_every, block, jentry, compact=None):
        """`rows` stored rows of `t` steps each.  One GPU, history kept: the steps run as internal
        calls of c*t steps that write a staging block of c*t rows through the usual paths; once
        a call's launches are known to have ended well (what _steps ends with), ONE launch copies
        staging rows t-1, 2t-1, ... to the next c rows of the compact block that flush downloads
        (nh_hist_thin, stream-ordered, no synchronisation of its own).  c: as many rows as keep
        the staging block's allocation within NAIMA_AMD_THIN_STAGE_MB (default 512).  If not even
        t rows fit, a stored row is t-1 steps without a history and one step with it, and the
        staging block holds one row.  `block` (several ranks): the full-rate block, thinned on
        the host by flush.  `compact` (a monitored run): the pending block that takes the rows,
        from its row compact.n on, instead of a new one.  thin_info says what was done."""
        s, ctx, N = self.s, self.ctx, self.N
        group = rows if yield_every >= rows else max(1, int(yield_every))
        info = dict(thin_by=t, where="host" if block is not None else "none", stage_rows=0,
                    stage_bytes=0, stage_alloc_bytes=0, calls=[])
        self.thin_info = info
        stage = None
        split = False
        if store and rows > 0 and block is None:
            widths = [N * self.ndim, N] + [N * b.m for b in self._kept]
            budget = int(float(os.environ.get("NAIMA_AMD_THIN_STAGE_MB", "512")) * (1 << 20))

            def alloc(r):  # (what the context's pool sets aside for r rows)
                return sum(ctx._bucket(8 * r * w) for w in widths)

            lo, hi = 0, group  # the largest c in [1, group] whose c*t rows stay in the budget
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if alloc(mid * t) <= budget else (lo, mid - 1)
            split = lo == 0
            group = max(1, lo)
            srows = 1 if split else group * t
            if compact is None:
                compact = self._new_block(rows)
                self.hist.append(compact)
            stage = self._new_block(srows)
            info.update(where="device", stage_rows=srows, stage_bytes=8 * srows * sum(widths),
                        stage_alloc_bytes=alloc(srows))

        def call(steps, blk):
            if blk is stage and stage is not None:
                stage.n = 0
            for _ in self._steps(steps, 1 << 30, blk, jentry):
                pass
            info["calls"].append((steps, steps if blk is not None else 0))

        done = 0
        while done < rows:
            c = min(group, rows - done)
            if stage is None:
                call(c * t, block)
            elif split:
                call(t - 1, None)
                call(1, stage)
                self._compact(stage, compact, 0, 1, 1)
            else:
                call(c * t, stage)
                self._compact(stage, compact, t - 1, t, c)
            s.iteration -= c * t - c  # (stored rows; _advance has counted the steps)
            done += c
            yield DeviceState(self, s._rng)

    def _compact(self, stage, compact, first, stride, nrows):
        """rows first, first + stride, ... of the staging block -> the compact block's next nrows
        rows: one launch for the chain, the log-probability and (up to six) blob histories"""
        for segs in stage.thin_segs(compact):
            self.ctx.call("nh_hist_thin", segs, len(segs), first, stride, nrows, compact.n)
        compact.n += nrows
        self._changes += 1

    def _steps(self, iterations, yield_every, block, jentry):
        """`iterations` ensemble steps from the ensemble in HBM, their rows appended to `block`
        (None: no history) from its row block.n on"""
        # the launches append the chain history themselves (the nh_hist descriptor) when the
        # call keeps one and the launch's plan exists; else one pair of copies per step ...
        dev_hist = self.fused and block is not None and not (self.mega and self._hs is None)
        # ... and the blobs' histories too, in the one-launch mode
        blob_dev_hist = dev_hist and self.blobs_in_kernel
        # several steps per launch need whatever the call keeps to be kept by the launches
        whole = (block is None or dev_hist) and not (block is not None and block.blobs and
                                                     not blob_dev_hist)
        # the whole call as launches of the resident loop, one per block of moves: nothing of the
        # per-launch kernel's bookkeeping (history descriptor words, slice counter) is needed
        fast = self._resident_ok() and yield_every >= iterations and whole
        it = 0
        if fast:
            it = yield from self._sample_resident(iterations, block, jentry)
        if not fast or it < iterations:
            yield from self._sample_per_launch(it, iterations, yield_every, block, jentry,
                                               dev_hist, blob_dev_hist, whole)
        self._flush_pending()

    def _advance(self, g, block, jentry):
        """the books after `g` more steps of the call"""
        s = self.s
        s.iteration += g
        s.steps_total += g
        if jentry is not None:
            jentry.made += g
        if block is not None:
            block.n += g
        self._changes += 1

    def _sample_resident(self, iterations, block, jentry):
        """the call as launches of the resident loop, up to KSTEPS steps each, a launch checked
        when the one behind it is queued (LaunchQueue.settle) -> the steps made: fewer than
        `iterations` when a launch gave up, and the per-launch loop makes the rest"""
        ring = self.ring
        moves = self.s.moves(pinned=True)
        it = 0
        while it < iterations:
            # the moves are a function of the seed only, so the stream's next steps are already on
            # the device (uploaded ahead by `launched`) unless this is the first call
            want = min(ring.KSTEPS, iterations - it)
            slice0 = ring.reserve(moves, want)
            if self._rl.queued >= 2:
                # launch n + 1 is queued only once launch n - 1 is known to have ended well (launch
                # n is running meanwhile: the device does not wait for this)
                gave_up = self._rl.settle(1, self._launch_report)
                if gave_up is not None:
                    return self._rollback(gave_up)
            rec = self._run_resident(slice0, 2 * want, block)
            if rec is None:
                return it  # (gave up: the per-launch loop replays these steps)
            if not self.shared:  # (a shared loop's launches are checked where all ranks are)
                rec.it = it
                self._rl.push(rec)
            ring.launched(moves, want)
            it += want
            self._advance(want, block, jentry)
            if it >= iterations and self._rl.queued:
                # the call's last launches: known to have ended well before the state is handed out
                gave_up = self._rl.settle(0, self._launch_report)
                if gave_up is not None:
                    return self._rollback(gave_up)
            yield DeviceState(self, self.s._rng)
        return it

    def _sample_per_launch(self, it, iterations, yield_every, block, jentry, dev_hist,
                           blob_dev_hist, whole):
        """steps it .. iterations of the call, a block of KSTEPS moves uploaded at a time, with one
        launch per half-step, a graph of several steps, or the resident loop for a block's rest"""
        s, ctx, ring, N = self.s, self.ctx, self.ring, self.N
        if self.fused:
            # (the per-launch kernel's history descriptor: where its launches append the chain)
            words = block.words(dev_hist, blob_dev_hist) if block is not None else [0] * 8
            ctx.call("nh_set_words", self.histd, (C.c_longlong * 8)(*words), 8)
        moves = s.moves(pinned=True)
        if it < iterations:
            ring.forget_launches()
        while it < iterations:
            self._flush_pending()  # (merged sharded mode) the block's last accept
            self._sync_cur_blobs()  # (launches per half-step keep every rank's blobs whole)
            self._cur_host = None
            # ---- ship the moves of the next K steps: ONE asynchronous upload from the
            # generator's page-locked ring (filled ahead by its worker thread) ----------
            K = ring.next_block(moves, iterations - it)
            if self.fused:
                if self.mega and self._hs is not None:
                    # (the one-launch kernel writes the cursor itself, every launch)
                    ctx.call("nh_half_step_begin_block", self._hs.handle, 0,
                             block.n if dev_hist else 0)
                    if self._plan.stage is not None:  # (its other launch: StepPlan.stage_a)
                        ctx.call("nh_half_step_begin_block", self._plan.stage.handle, 0, 0)
                else:
                    ctx.call("nh_memset", self.cursor, 0xFF, 4)  # -1: nothing accepted yet
                    if not self.mega:
                        self._front()  # slice 0 of the new block
            else:
                ctx.call("nh_memset", self.cursor, 0, 4)
            # (recorded behind the block's first launch: the host gets that one out first)
            mark, mark_pending = ring.block_mark(), True
            k = 0
            while k < K:
                self._pos["slice"], self._pos["steps"] = 2 * k, (block.n - k) if dev_hist else 0
                # several steps per graph launch when nothing has to happen on the host
                # between them (history is kept by the kernel, nobody reads the states)
                g = 1
                gmax = min(self.GSTEPS, K - k) if self.mega else self.GSTEPS
                resident = False
                if self._resident_ok() and yield_every >= K - k and whole:
                    # the rest of this block of moves in ONE launch of resident workgroups
                    g = K - k
                    if k > 0 and dev_hist:
                        # the per-launch kernel leaves the history row of a closed step to the
                        # NEXT launch of the block: there is none, the resident loop takes over
                        self._append_closed_row(block, blob_dev_hist)
                    self._flush_pending()
                    if self._run_resident(2 * k, 2 * g, block if dev_hist else None) is None:
                        continue  # (gave up: _resident_ok() is false from now on)
                    resident = True
                elif (self.step_graph is not None and self.fused and K - k >= gmax >= 2 and
                        yield_every >= gmax and whole):
                    g = gmax
                    # one launch per half-step: the slices are baked into the graph (the
                    # proposal's chain of dependent reads is one trip shorter), so there is
                    # one graph per (starting step of the block of moves, number of steps):
                    # the tail of a block shorter than GSTEPS is a graph of its own
                    key = (k, g) if self.mega else 0
                    if key not in self.multi_graphs:
                        self.multi_graphs[key] = self.multi_graph = self._capture_steps(k, g)
                    ctx.graph_launch(self.multi_graphs[key])
                elif (self.split and self.graph2 is not None and self.fused and
                        yield_every >= 2 and whole and not (block is not None and block.blobs)):
                    # sharded, nobody looks at the intermediate states: the accept of a
                    # half-step and the evaluation of the next are ONE graph, with the
                    # all-gather between two such graphs (two host calls per half-step
                    # instead of three)
                    self._run_half_step_merged()
                    self._run_half_step_merged()
                else:
                    self._flush_pending()
                    self._run_step()
                if mark_pending:
                    ctx.call("nh_marker_record", mark)
                    mark_pending = False
                k += g
                it += g
                if block is not None and not (dev_hist and blob_dev_hist):
                    block.copy_row(ctx, N, self.ndim, self.coords, self.logp, self.cur_blobs or [],
                                   state=not dev_hist, blobs=not blob_dev_hist)
                self._advance(g, block, jentry)
                if yield_every < 2:
                    self._flush_pending()
                if self.mega and dev_hist and not resident and (k >= K or yield_every <= iterations):
                    # one launch per half-step: the row of a closed step is written by the
                    # NEXT launch of the same block of moves; nothing follows the last one of
                    # a block, and whoever is handed this state may read the chain (nobody
                    # does between the graphs of one run_mcmc call: yield_every > iterations)
                    self._flush_pending()
                    self._append_closed_row(block, blob_dev_hist)
                yield DeviceState(self, s._rng)

    def _append_closed_row(self, block, blobs_too):
        """the history row of the step the per-launch kernel closed last, which it leaves to the
        next launch of the block of moves: there is none"""
        self.ctx.call("nh_hist_append", self.coords, self.logp, self.N, self.ndim, self.histd,
                      block.n - 1)
        if blobs_too:
            self.ctx.call("nh_half_step_append_blobs", self._hs.handle, block.n - 1)

    # ------------------------------------------------------------- resident loop
    def _resident_ok(self):
        """can the rest of a block of moves run as ONE launch (nh_half_step_run)?  Needs the
        one-launch plan, a single rank, blobs (if kept) kept by the launch; the library has
        the last word (LDS, occupancy, the plan's shape)"""
        if self._run is False or not self.mega or not self.s.use_graph or self._plan.staged:
            return False
        if self.sharded and (self.s.comm.size < 2 or getattr(self.s.comm, "group", None) is None
                             or os.environ.get("NAIMA_AMD_SHARED", "1") == "0"):
            return False
        hs = self._hs
        if hs is None:
            return False
        if self.s.store_blobs and self.cur_blobs and not self.blobs_in_kernel:
            return False
        if self._run is None and self.sharded:
            self._run = self._create_shared_run(hs) or False
            self.shared = bool(self._run)
            return self.shared
        if self._run is None:
            h = _lib._dp()
            if _lib._lib.nh_half_step_run_create(self.ctx.h, hs.handle, C.byref(h)) != 0:
                self._run = False
                self.resident_reason = _lib._lib.nh_last_error().decode()
                return False
            self._run = h
            self._rl.reset()  # (the library numbers a loop's launches from 1)
            self._adopt_run(hs, h)
        return True

    def _adopt_run(self, hs, h):
        """a resident loop that was created well: owned by this loop, its tables sorted, its
        shape on record (resident_info)"""
        self._res["runs"].append(h)
        self.ctx.sorted_tables(hs, h)
        g, t, l = _lib._i(), _lib._i(), _lib._ll()
        _lib._chk(_lib._lib.nh_half_step_run_info(h, C.byref(g), C.byref(t), C.byref(l)))
        mode, m, pcs = _lib._i(), _lib._i(), _lib._i()
        _lib._chk(_lib._lib.nh_half_step_run_syn_info(h, C.byref(mode), C.byref(m), C.byref(pcs)))
        inreg, nmax = _lib._i(), _lib._i()
        _lib._chk(_lib._lib.nh_half_step_run_table_info(h, C.byref(inreg), C.byref(nmax)))
        spl, rows = _lib._i(), _lib._i()
        _lib._chk(_lib._lib.nh_half_step_run_split_info(h, C.byref(spl), C.byref(rows)))
        deep = _lib._i()
        _lib._chk(_lib._lib.nh_half_step_run_pipeline_info(h, C.byref(deep)))
        self.resident_info = dict(
            grid=g.value, threads=t.value, lds_bytes=l.value,
            syn_log_domain=bool(mode.value), syn_nodes_per_piece=m.value, syn_pieces=pcs.value,
            tables_in_registers=bool(inreg.value), workgroups_per_walker=spl.value,
            rows_split=bool(rows.value), two_walkers_in_flight=bool(deep.value))

    def _create_shared_run(self, hs):
        """the resident loop over an ensemble shared with the other ranks' GPUs: rings in
        fine-grained memory, mapped by every other rank (hipIpc handles carried by the control
        plane), and a probe launch that exchanges tagged granules with every peer -- every step
        agreed by all ranks, so that all take the shared loop or none does"""
        lib, ctx, comm = _lib._lib, self.ctx, self.s.comm
        g = comm.group
        h = _lib._dp()
        why = ""

        def agreed(ok):
            return g.reduce_scalar(1.0 if ok else 0.0, "min") == 1.0

        def give_up(msg):
            if h.value:
                lib.nh_half_step_run_destroy(ctx.h, h)
            self.resident_reason = msg
            if comm.rank == 0:
                warnings.warn("the resident loop over a shared ensemble is not available (%s): "
                              "one launch and one all-gather per half-step instead" % msg)
            return None

        ok = lib.nh_half_step_run_create_shared(ctx.h, hs.handle, comm.rank, comm.size,
                                                C.byref(h)) == 0
        if not ok:
            why = lib.nh_last_error().decode()
        if not agreed(ok):
            return give_up("create: " + why)
        handle = C.create_string_buffer(64)
        ok = lib.nh_half_step_run_export(ctx.h, h, handle) == 0
        parts = g.allgather_bytes(handle.raw if ok else b"")
        ok = all(len(p_) == 64 for p_ in parts)
        for r, p_ in enumerate(parts):
            if ok and r != comm.rank:
                ok = lib.nh_half_step_run_attach(ctx.h, h, r, p_) == 0
        if not ok:
            why = lib.nh_last_error().decode()
        if not agreed(ok):
            return give_up("hipIpc: " + why)
        ctx.sync()
        g.barrier()
        st, us = _lib._i(), C.c_double()
        ok = lib.nh_half_step_run_probe(ctx.h, h, 64, C.byref(st), C.byref(us)) == 0 and \
            st.value == 0
        why = "" if ok else lib.nh_last_error().decode()
        if "ring" in os.environ.get("NAIMA_AMD_LADDER_REFUSE", "").split(","):
            # (tests: this rung of the exchange ladder refused although the probe went well -- the
            # ranks then take the next one, as on a node whose GPUs cannot store into each other)
            ok, why = False, "refused on request (NAIMA_AMD_LADDER_REFUSE=ring: fault injection of the tests)"
        if not agreed(ok):
            return give_up("a record stored by another GPU did not reach a running kernel; %s" % why)
        self._adopt_run(hs, h)
        self.shared_info = dict(ranks=comm.size, probe_us_per_exchange=us.value)
        return h

    def device_barrier(self):
        """ranks that share an ensemble meet on the device: one exchange of tagged granules
        with every peer (the probe launch), a few microseconds apart instead of the control
        plane's ~0.1 ms.  Synchronises the stream; a no-op for any other loop."""
        if self.shared:
            st = _lib._i()
            _lib._chk(_lib._lib.nh_half_step_run_probe(self.ctx.h, self._run, 1, C.byref(st), None))
            if st.value != 0:
                raise _lib.NaimaHipError("device barrier of the shared ensemble timed out")

    def _sync_cur_blobs(self):
        """a shared ensemble: every rank's current-blob arrays := the blobs of where each walker
        IS -- held by the rank that accepted its last move (largest stamp).  Collective."""
        if not self._cur_dirty:
            return
        self._cur_dirty = False
        stamps = np.empty(self.N, dtype=np.int32)
        _lib._chk(_lib._lib.nh_half_step_run_counters(self.ctx.h, self._run, None,
                                                      stamps.ctypes.data, 2))
        hosts = [b.cur.get().reshape(self.N, b.m) for b in self.cur_blobs or []]
        shared_merge.merge_current_blobs(self.s.comm.group, self.s.comm.rank, stamps, hosts)
        for b, host in zip(self.cur_blobs or [], hosts):
            b.cur.set(host.ravel())
        self._cur_host = hosts  # (valid until a launch changes the blobs again)

    def _run_resident(self, slice0, nslices, block):
        """queue a launch of the resident loop -> the books as it found them (_checkpoint, with the
        launch's number and its copy of the current blobs), or None if it was checked and gave up"""
        ctx, hs = self.ctx, self._hs
        if self.shared:
            self._acc_dirty = True
            own = block.own if block is not None else None
            _lib._chk(_lib._lib.nh_half_step_run_hist_flags(self._run, own.ptr if own is not None
                                                            else None))
            if self.s.store_blobs and self.cur_blobs:
                self._cur_dirty = True
                self._cur_host = None
            if own is not None:
                block.shared_rows.append((block.n, block.n + nslices // 2))
        hist_args = block.run_args() if block is not None else loop_books.NO_HISTORY
        books = self._checkpoint(block)
        probation = not self.shared and self._resident_trust < 2
        if probation:
            # The first launches of a loop are checked before anything builds on them: a launch
            # whose workgroups cannot all be resident (another process on the GPU, a profiler that
            # serialises workgroups) gives up on its first wait -- it leaves the ensemble, the
            # counters and the move stream as they were (k_run_epilogue does nothing then), so the
            # same block of moves is replayed by the per-launch kernel and the run carries on
            # with one launch per half-step.  (A shared ensemble: the ranks agree in
            # _create_shared_run / bench.py's rehearsal and raise together on a later time-out; a
            # one-GPU loop's later launches are checked a launch behind: _sample_resident.)
            books.counts = self._read_counts(reset=False)
        if block is None and not self.shared and self.s.store_blobs and self.cur_blobs:
            books.snap = self._snapshot_cur_blobs()
        ctx.call("nh_half_step_run", hs.handle, self._run, slice0, nslices, *hist_args)
        books.launch = self._rl.launched()  # (the library numbers a loop's launches the same way)
        if probation:
            st = self.resident_status()
            if st != 0:
                # (nothing consumed the launch's moves: the per-launch loop takes them from `blk`)
                self._leave_resident(_GAVE_UP % st, "the block of moves is replayed "
                                     "and the run continues with one launch per half-step", 1, books)
                return None
            self._resident_trust += 1
        self.resident_launches += 1
        self.s.n_lnprob_calls += nslices
        self.s.n_walker_evals += nslices * self.nloc
        return books

    def _rollback(self, rec):
        """a launch of the resident loop gave up waiting for a walker's record (its workgroups were
        not all resident: another process on the GPU, a profiler) -- `rec` is the first such
        launch, everything queued behind it found the same status and changed nothing either
        (k_run_epilogue leaves the ensemble, the counters and the blobs as a launch that gave up
        found them).  Back to the books `rec` holds, the move stream made again up to its step;
        the per-launch loop takes over for good -> the step of the call to carry on from"""
        void = self._rl.void_from(rec)
        self._rl.drop()
        self.ctx.sync()  # (the void launches behind it: nothing of theirs may still be running)
        self._leave_resident(_GAVE_UP % rec.status, "%d block(s) of moves are replayed "
                             "and the run continues with one launch per half-step" % void, void, rec,
                             rewind=True)
        return rec.it

    def _leave_resident(self, reason, then, failed, books, rewind=False):
        """the resident loop given up for good: `failed` launches of it void, the books back to
        `books` (with `rewind` the move stream too), the per-launch loop carries the run on"""
        self.resident_reason = reason
        if self.s.comm.rank == 0:
            warnings.warn(reason + "; " + then)
        self._run, self.shared = False, False
        self.resident_failed_launches += failed
        self._restore(books)
        if rewind:
            self._rewind_moves(books.steps_total)

    def _checkpoint(self, block=None, counts=None):
        """the host's books as one record for _restore (`counts`: the device's NaN / forbidden
        counters to put back, when known here)"""
        return Books.take(self.s, self, block, counts)

    def _restore(self, books):
        self._read_counts(reset=False, set_to=books.counts)  # (the replay counts them again)
        self._restore_cur_blobs(books.snap)  # (what launches that gave up may have written)
        books.put_back(self.s, self)

    def _rewind_moves(self, steps):
        """the move stream made again from the seed (a fresh generator, every upload of the old one
        done) and its first `steps` steps skipped: the steps every loop of this sampler has made"""
        s = self.s
        self.ring.reset()
        old, s._moves = s._moves, None
        moves = s.moves(pinned=True)
        if old is not None:
            old.close()
        while steps > 0:
            steps -= moves.take(min(self.ring.KSTEPS, steps))[1]

    def _snapshot_cur_blobs(self):
        """device copies of the current blobs, in stream order ahead of the launch about to be
        queued (one of four sets: at most three launches are ever unsettled) -> the set's index"""
        k = self._rl.count % len(self._cur_snaps)
        self._cur_snaps[k] = loop_books.copy_blobs(self.ctx, self.N, self.cur_blobs,
                                                   self._cur_snaps[k])
        return k

    def _restore_cur_blobs(self, k):
        if k is None or self._cur_snaps[k] is None:
            return
        loop_books.copy_blobs(self.ctx, self.N, self.cur_blobs, self._cur_snaps[k], back=True)
        self._cur_host = None

    def _before_read(self):
        """what comes before a download of the ensemble's state"""
        self._flush_pending()
        self._settle_before_read()  # (one GPU: the friendlier message, ahead of the status)
        self.check_resident()
        self.check_nan()

    def _settle_before_read(self):
        """somebody reads the state (or drains the counters) while launches of the resident loop
        are still unsettled -- a caller iterating sample() launch by launch: wait for them; one that
        gave up is replayed when the iteration goes on, and until then the state on the device is
        the one BEFORE it"""
        if self._rl.queued and self._run:
            rec = self._rl.settle(0, self._launch_report)
            if rec is not None:
                raise _lib.NaimaHipError(
                    "a launch of the resident loop gave up waiting for a walker's record (status %d); "
                    "its block of moves is replayed when the iteration continues -- read the state "
                    "after that" % rec.status)

    # ------------------------------------------------ a shared ensemble: kept state and replay
    def _shared_snapshot(self):
        """device copies of the ensemble (positions, log-probabilities, acceptance counts, current
        blobs) and the host's books, at a point where every rank is known to be well"""
        ctx = self.ctx
        self._flush_pending()
        # (the device's counters: drained at the kept state, the replay counts again)
        snap = self._checkpoint(counts=(0, 0))
        self._sync_cur_blobs()  # (every rank's current blobs whole before they are kept)
        snap.ensemble = EnsembleCopy.take(ctx, self.N, self.ndim, self.coords, self.logp, self.nacc,
                                          self._kept)
        self._sh_snap = snap
        self._sh_journal = []

    def _shared_verified(self):
        """every rank's launches since the kept state ended well: the ensemble as it stands is the
        one to go back to from now on.  It is KEPT at the end of the flush / reset this was found in
        (keep_verified) -- after the NaN / forbidden counts have been drained, the acceptance
        counters zeroed and the sampler's iteration reset -- so that a replay starts from the
        books as they stand behind that point, not before it (kept here, a reset()'s
        snapshot held the burn-in's acceptance counts and iteration)."""
        self._sh_snap = None
        self._sh_journal = []
        self._sh_want = bool(self.shared and self._have_state)

    def keep_verified(self):
        """the last thing a flush does, and a reset (the sampler's, once ITS books are cleared):
        keep the ensemble every rank was found well at (here, where every rank is anyway, and
        not inside the next call: a 20-step call is a millisecond)"""
        if self._sh_want:
            self._sh_want = False
            if self.shared and self._have_state:
                self._shared_snapshot()

    def _replay_shared(self, bad, mine):
        """a launch of the shared loop gave up on some rank (status `bad`; this rank's own: `mine`).
        Every rank is here (the status was reduced over all of them): back to the kept ensemble,
        the move stream made again up to its step, and the journal's calls once more -- one launch
        and one all-gather per half-step from here on."""
        ctx, s, snap, journal = self.ctx, self.s, self._sh_snap, self._sh_journal
        ctx.sync()
        # what the shared launches accepted up to the kept state stays counted (flush folded it)
        self._acc_base = self._acc_base + self._acc_shared
        self._acc_shared, self._acc_dirty = 0.0, False
        self._cur_dirty, self._cur_host = False, None
        self._sh_snap, self._sh_journal = None, []
        snap.ensemble.put_back(ctx, self.coords, self.logp, self.nacc, self.cur_blobs or [])
        self._leave_resident(
            "a launch of the resident loop over the shared ensemble gave up waiting for a record "
            "(status %d%s)" % (bad, "" if bad == mine else ", on another rank"),
            "every rank goes back %d step(s) to the last ensemble all of them held and carries on "
            "with one launch and one all-gather per half-step" % (s.steps_total - snap.steps_total),
            max(1, self.resident_launches - snap.rl), snap, rewind=True)
        self._replaying = True
        try:
            for jentry in journal:
                for n, keep, by in jentry.replay_calls():
                    if n > 0:
                        for _ in self.sample(DeviceState(self, s._rng), n, keep,
                                             yield_every=1 << 30, thin_by=by):
                            pass
            self._flush_pending()
            ctx.sync()
        finally:
            self._replaying = False

    def _launch_report(self, launch):
        """wait until launch number `launch` of the resident loop has ended -> (its status, the
        (NaN, forbidden) counts as it found them): what LaunchQueue.settle asks"""
        done, st, before = _lib._i(0), _lib._i(0), (C.c_int * 2)()
        _lib._chk(_lib._lib.nh_half_step_run_report(self.ctx.h, self._run, launch, 1,
                                                    C.byref(done), C.byref(st), None, None, before))
        return st.value, (before[0], before[1])

    def _read_counts(self, reset, set_to=None):
        """(NaN log-probabilities, proposals forbidden by the prior) the kernels have counted on
        the device since the last reset"""
        hs = self._hs
        extra = extra_f = 0
        if set_to is None:
            # launches of the separate kernels (cfg4; the first half-steps of any run): their
            # accepts count into the context's words
            n = _lib._i(0)
            _lib._chk(_lib._lib.nh_nan_count(self.ctx.h, 1 if reset else 0, C.byref(n)))
            extra = n.value
            _lib._chk(_lib._lib.nh_forbidden_count(self.ctx.h, 1 if reset else 0, C.byref(n)))
            extra_f = n.value
        if hs is None or hs.handle is None:
            return extra, extra_f
        n, f = _lib._i(0), _lib._i(0)
        if set_to is not None:
            n, f = _lib._i(-set_to[0] - 1), _lib._i(-set_to[1] - 1)
        _lib._chk(_lib._lib.nh_half_step_counts(self.ctx.h, hs.handle, 1 if reset else 0,
                                                C.byref(n), C.byref(f)))
        return n.value + (extra if reset else 0), f.value + (extra_f if reset else 0)

    def check_nan(self, collective=False):
        """NaN log-probabilities the launches met since the last look (one-launch plans count
        them on the device): counted, or raised as emcee does, by the sampler's nan_policy.
        With several ranks the counts are per rank (a proposal is counted by the rank that moved
        the walker): where every rank is known to be here (``collective``: flush, reset, the merge
        of the current blobs) they are summed over the ranks first, so that every rank counts --
        and raises -- the same; elsewhere a rank only accumulates what it has seen, because a
        ValueError on one rank would leave the others waiting in their next collective."""
        self._settle_before_read()  # (the counters are not drained under an unsettled launch)
        n, f = self._read_counts(reset=True)
        self._nan_pending += n
        self._forbidden_pending += f
        multi = self.s.comm is not None and self.s.comm.size > 1
        if multi and not collective:
            return
        n, f = self._nan_pending, self._forbidden_pending
        self._nan_pending = self._forbidden_pending = 0
        if multi:
            n, f = (int(x) for x in shared_merge.sum_over_ranks(self.s.comm.group, (n, f)))
        self.s.prior_forbidden_proposals += f
        if n:
            self.s.nan_proposals += n
            if self.s.nan_policy == "raise":
                raise ValueError("Probability function returned NaN (%d proposals of the device "
                                 "loop; emcee stops at the first one -- pass nan_policy='reject' "
                                 "to treat them as rejected proposals)" % n)

    def resident_status(self):
        """this rank's status word of the resident loop (0: every launch found its records);
        synchronises the stream, raises nothing -- for callers that reduce it over the ranks
        themselves (bench.py's rehearsal)"""
        st = _lib._i(0)
        if self._run:
            _lib._chk(_lib._lib.nh_half_step_run_status(self.ctx.h, self._run, C.byref(st)))
        return st.value

    def check_resident(self, collective=False):
        """raise if a launch of the resident loop gave up waiting for a walker's record (its
        workgroups were not all resident: another process on the GPU, a profiler that
        serialises workgroups); the ensemble is undefined from that launch on.  (A one-GPU
        loop's launches are checked as they are made, or a launch behind, and replayed by the
        per-launch kernel instead: _run_resident, sample -- what is left to find here is a
        shared ensemble's.)  ``collective``: every rank is here -- the worst status of all ranks
        decides, and all of them raise."""
        if self.shared and not collective and self.s.comm is not None and self.s.comm.size > 1:
            # a shared loop's status is acted on where EVERY rank is (flush, reset): an exception on
            # the one rank that reads its state here would leave the others waiting in their next
            # collective -- the launch that gave up is found there and replayed by all
            return
        mine = bad = self.resident_status()
        if collective and self.s.comm is not None and self.s.comm.size > 1:
            bad = int(self.s.comm.group.reduce_scalar(float(bad), "max"))
            if bad == 0:
                self._shared_verified()
            elif self.shared and self._sh_snap is not None and not self._replaying:
                self._replay_shared(bad, mine)
                return
        if bad != 0:
            raise _lib.NaimaHipError(
                "the resident half-step loop timed out waiting for a walker's record (status "
                "%d%s): its workgroups were not all resident%s.  Run with NAIMA_AMD_%s=0"
                % (bad, "" if bad == mine else ", on another rank",
                   ", or a rank of the shared ensemble fell behind or failed"
                   if self.shared else "", "SHARED" if self.shared else "RESIDENT"))

    def _run_half_step_merged(self):
        ctx = self.ctx
        if self._pending:
            if self.graph21 is None:
                self.graph21 = self._capture(lambda: (self._part_accept(), self._part_evaluate()))
            ctx.graph_launch(self.graph21)  # accept + next proposal + evaluation
        else:
            ctx.graph_launch(self.graph)    # evaluation (the proposal is already there)
        self._exchange()
        self._pending = True

    def _flush_pending(self):
        if self._pending:
            self.ctx.graph_launch(self.graph2)
            self._pending = False

    def _capture_steps(self, k0, nsteps):
        """hipGraph of ``nsteps`` ensemble steps starting at step k0 of a block of moves"""
        def run():
            for i in range(2 * nsteps):
                self._pos["slice"] = 2 * k0 + i
                self._half_step_body()

        self._pos["bake"] = bool(self.mega)
        try:
            return self._capture(run)
        finally:
            self._pos["bake"] = False

    def _capture(self, fn):
        ctx = self.ctx
        ctx.pin_caches()
        ctx.sync()
        ctx.graph_begin()
        try:
            fn()
        except Exception:
            ctx.graph_abort()
            raise
        g = ctx.graph_end()
        self._res["graphs"].append(g)
        return g

    def _run_step(self):
        """one ensemble step = two half-steps.  Single GPU: after the eager warm-up and
        the per-half-step capture check, BOTH half-steps are one graph (the cursor
        advances inside it), i.e. one host call per step."""
        s, ctx = self.s, self.ctx
        if self.split or not s.use_graph:
            self._run_half_step()
            self._run_half_step()
            return
        if self.step_graph is not None:
            ctx.graph_launch(self.step_graph)
            return
        if self.warm < 1:
            # the first evaluation settles which grids share a weights launch, the
            # second one is recorded
            self._half_step_body()
            self._record_half_step()
            self.warm += 2
            return
        if self.mega and self._hs is None:
            # the first one-launch half-step creates the kernel's descriptor (device
            # allocation + upload): not inside a stream capture
            self._first_one_launch_half_step()
            self._half_step_body()
            return

        def two():
            self._half_step_body()
            self._half_step_body()

        self.step_graph = self.graph = self._capture(two)
        ctx.graph_launch(self.step_graph)

    def _first_one_launch_half_step(self):
        """the half-step that creates the one-launch plan.  StepPlan.can_be_one_launch is an estimate
        made from the recorded launches; nh_half_step_create has the last word (exact LDS
        layout, its admission rules).  If it turns the plan down, nothing has been launched
        yet for this half-step: the loop drops to the three-launch fused sequence for good."""
        try:
            self._half_step_body()
        except _lib.NaimaHipError:
            if self._hs is not None:
                raise  # the plan exists: this was a real failure of a launch
            warnings.warn("nh_half_step_create turned the one-launch plan down (%s); the device "
                          "loop keeps the three-launch half-step"
                          % _lib._lib.nh_last_error().decode())
            self.mega = self._plan.mega = self._plan.staged = False
            self.blobs_in_kernel = False
            self._hook.reset(total=self.mylp if self.sharded else None)
            self._front()  # proposal + packs + weights of this slice, as a launch of its own
            self._half_step_body()

    def _run_half_step(self):
        """eager warm-up (fills the static caches), then capture, then replay.  One
        graph on a single GPU; with walkers sharded over ranks the collective sits
        between two graphs (evaluate | all-gather | accept)."""
        s, ctx = self.s, self.ctx
        multi = self.split
        if self.graph is not None:
            ctx.graph_launch(self.graph)
            if multi:
                self._exchange()
                ctx.graph_launch(self.graph2)
            return
        if self.warm < 2:
            if self.warm == 0:
                self._half_step_body()
            else:
                self._record_half_step()
            self.warm += 1
            return
        if self.mega and self._hs is None:
            self._first_one_launch_half_step()  # (never inside a capture)
            return
        if not s.use_graph:
            self._half_step_body()
            return
        if not multi:
            self.graph = self._capture(self._half_step_body)
            ctx.graph_launch(self.graph)
            return
        self.graph = self._capture(self._part_evaluate)
        ctx.graph_launch(self.graph)
        self._exchange()
        self.graph2 = self._capture(self._part_accept)
        ctx.graph_launch(self.graph2)

    def flush(self):
        """bring the pending chain history and acceptance counters to the host"""
        if self._flushed_at == self._changes and not self.hist and not self._pending:
            # nothing has run since the last flush: the books are on the host already.  (With
            # several ranks a flush is collective; the count follows the calls, which the ranks
            # make alike, so this early return is taken by all of them or none -- and a rank that
            # reads its results AGAIN, alone, after the others have left -- rank 0 writing the run
            # to disk, as the reference's save_run does in its one process, analysis.py:366-471 --
            # is not left waiting for peers that are gone.)
            return
        self._meet()
        s = self.s
        # (the ranks' rows of a shared loop's block are merged at full rate, before a thinned call's
        # rows are thinned)
        merge = functools.partial(shared_merge.merge_history_rows, s.comm.group, s.comm.rank) \
            if self.shared else None
        for block in self.hist:
            rows = block.host_rows(self.N, self.ndim, self.cur_blobs or [], merge)
            if rows is None:
                continue
            c, l, per = rows
            n = c.shape[0]
            s._chain.extend(list(c))
            s._logp.extend(list(l))
            if block.blobs:
                per = [a.reshape((n, self.N) + b.trail) for a, b in zip(per, self.cur_blobs)]
                per = loop_books.with_const_blobs(per, self.const_blobs,
                                                  lambda v: np.full((n, self.N), v))
                if s._blobs is None:
                    s._blobs = [[] for _ in per]
                for j, a in enumerate(per):
                    s._blobs[j].extend(list(a))
        self.hist = []
        s.naccepted = self.nacc.get().astype(float) + self._acc_base
        if self.shared:  # + the moves each rank's shared launches accepted
            if self._acc_dirty:  # (collective only when launches have run since the last look)
                self._acc_dirty = False
                own = np.empty(self.N, dtype=np.int32)
                _lib._chk(_lib._lib.nh_half_step_run_counters(self.ctx.h, self._run,
                                                              own.ctypes.data, None, 0))
                self._acc_shared = shared_merge.sum_over_ranks(s.comm.group, own).astype(float)
            s.naccepted += self._acc_shared
        self.keep_verified()
        self._flushed_at = self._changes
