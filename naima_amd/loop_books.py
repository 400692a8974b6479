"""The book-keeping records of the device step loop (device_sampler.DeviceLoop): the blobs it keeps,
a history block in HBM, the checkpoint of the host's books, a device copy of the ensemble, the
journal of a shared ensemble's calls and the queue of launches not yet known to have ended well.

Records only: each layout (the eight history words, the history arguments of a resident launch, a
block's rows on the host) is written down once, here.  No library call is made at import.
"""
import ctypes as C
import dataclasses
import typing

import numpy as np

from . import _lib
from .step_plan import _ByName


class KeptBlob(typing.NamedTuple):
    """a blob kept in HBM: its current values ``cur`` [N][m], the unit and the trailing shape the
    host sees it with"""
    cur: object
    m: int
    unit: object
    trail: tuple


def with_const_blobs(items, const_blobs, make):
    """``items`` (one per kept blob) with ``make(value)`` put back at the position of every blob
    that is a plain number (DeviceLoop.const_blobs: [(position, value)], ascending) -> items"""
    for j, v in const_blobs:
        items.insert(j, make(v))
    return items


def copy_blobs(ctx, N, kept, copies=None, back=False):
    """stream-ordered copies of the kept blobs' current values into ``copies`` (made here when
    None), or ``back`` from them -> copies"""
    if copies is None:
        copies = [ctx.empty((N, k.m)) for k in kept]
    for c, k in zip(copies, kept):
        dst, src = (k.cur, c) if back else (c, k.cur)
        ctx.call("nh_copy", dst, src, 8 * N * k.m)
    return copies


@dataclasses.dataclass
class EnsembleCopy:
    """device copies of the ensemble: positions, log-probabilities, acceptance counts and the
    current blobs"""
    N: int
    ndim: int
    coords: object
    logp: object
    nacc: object
    blobs: list

    @classmethod
    def take(cls, ctx, N, ndim, coords, logp, nacc, kept):
        e = cls(N, ndim, ctx.empty((N * ndim,)), ctx.empty((N,)), ctx.empty((N,), dtype=np.int32), [])
        ctx.call("nh_copy", e.coords, coords, 8 * N * ndim)
        ctx.call("nh_copy", e.logp, logp, 8 * N)
        ctx.call("nh_copy", e.nacc, nacc, 4 * N)
        e.blobs = copy_blobs(ctx, N, kept)
        return e

    def put_back(self, ctx, coords, logp, nacc, kept):
        ctx.call("nh_copy", coords, self.coords, 8 * self.N * self.ndim)
        ctx.call("nh_copy", logp, self.logp, 8 * self.N)
        ctx.call("nh_copy", nacc, self.nacc, 4 * self.N)
        copy_blobs(ctx, self.N, kept, self.blobs, back=True)


@dataclasses.dataclass
class HistoryBlock(_ByName):
    """``rows`` rows of chain history in HBM, the first ``n`` written: coords [rows][N ndim], logp
    [rows][N] and one matrix [rows][N m] per kept blob.  ``thin_by`` > 1: full-rate rows of a
    thinned call, thinned by host_rows.  A shared ensemble's block also has what the merge of the
    ranks' rows needs, all three or none: ``own`` [rows][N] int32 (who moved and accepted what),
    ``shared_rows`` ([row0, row1) of every shared launch) and ``cur0`` (the blobs as they stood
    before the first row: host arrays or device copies)."""
    rows: int
    n: int
    coords: object
    logp: object
    blobs: list
    thin_by: int = 1
    own: object = None
    shared_rows: list = None
    cur0: list = None

    def __post_init__(self):
        assert (self.own is None) == (self.shared_rows is None) == (self.cur0 is None)

    @property
    def shared(self):
        return self.own is not None

    @property
    def plain(self):
        """every stored row of a call is a row of the block, whole on this rank"""
        return self.n >= 1 and not self.shared and self.thin_by == 1

    def words(self, dev_hist, blob_dev_hist):
        """the eight words of the per-launch kernels' history descriptor (nh_set_words): where
        their launches append the chain (``dev_hist``) and the blobs (``blob_dev_hist``)"""
        if not dev_hist:
            return [0] * 8
        words = [self.coords.ptr, self.logp.ptr, 0, self.rows]
        if blob_dev_hist:
            words += [hb.ptr for hb in self.blobs]
        return (words + [0, 0, 0, 0])[:8]

    def run_args(self):
        """(hc, hl, hb[4], row0, cap) of nh_half_step_run"""
        hb = None
        if self.blobs:
            hb = (C.c_void_p * 4)(*([b.ptr for b in self.blobs] + [None] * 4)[:4])
        return self.coords.ptr, self.logp.ptr, hb, self.n, self.rows

    def copy_row(self, ctx, N, ndim, coords, logp, kept, state=True, blobs=True):
        """the current ensemble (``state``) and blobs (``blobs``) into row ``n``, stream-ordered"""
        kk = self.n
        if state:
            ctx.call("nh_copy", self.coords.ptr + 8 * kk * N * ndim, coords, 8 * N * ndim)
            ctx.call("nh_copy", self.logp.ptr + 8 * kk * N, logp, 8 * N)
        if blobs:
            for hb, k in zip(self.blobs, kept):
                ctx.call("nh_copy", hb.ptr + 8 * kk * N * k.m, k.cur, 8 * N * k.m)

    def thin_segs(self, compact):
        """the matrix pairs of nh_hist_thin from this (staging) block to ``compact``, at most
        eight per launch -> [nh_thin_seg array]"""
        pairs = [(self.coords, compact.coords), (self.logp, compact.logp)] + \
            list(zip(self.blobs, compact.blobs))
        return [(_lib.nh_thin_seg * len(part))(*[_lib.nh_thin_seg(a.ptr, b.ptr, a.shape[1])
                                                 for a, b in part])
                for part in (pairs[i:i + 8] for i in range(0, len(pairs), 8))]

    def host_rows(self, N, ndim, kept, merge=None):
        """the block's rows on the host -> (coords [r][N][ndim], logp [r][N], [blob [r][N][m]]) or
        None when there is none: downloaded, trimmed to ``n``, a shared block's completed by
        ``merge(own, shared_rows, cur0, coords, logp, blobs)`` at full rate, then every
        ``thin_by``-th row from ``thin_by - 1`` on"""
        n, tb = self.n, self.thin_by
        if n == 0:
            return None
        c = self.coords.get()[:n].reshape(n, N, ndim)
        l = self.logp.get()[:n].reshape(n, N)
        per = [hb.get()[:n].reshape(n, N, k.m) for hb, k in zip(self.blobs, kept)]
        if merge is not None and self.shared:
            cur0 = [b_ if isinstance(b_, np.ndarray) else b_.get() for b_ in self.cur0]
            merge(self.own.get()[:n].reshape(n, N), self.shared_rows, cur0, c, l, per)
        if tb > 1:
            c, l, per = c[tb - 1::tb], l[tb - 1::tb], [a[tb - 1::tb] for a in per]
        return (c, l, per) if c.shape[0] else None


NO_HISTORY = (None, None, None, 0, 0)  # HistoryBlock.run_args of a launch that keeps no history


def new_block(ctx, N, ndim, kept, rows, thin_by=1, shared=False, cur0_host=None):
    """a history block of ``rows`` rows in HBM for the ``kept`` blobs; ``shared``: with what the
    merge of several ranks' rows needs (``cur0_host``: host copies of the current blobs where
    the last merge left them, else they are copied on the device)"""
    own = shared_rows = cur0 = None
    if shared:
        own, shared_rows = ctx.empty((rows, N), dtype=np.int32), []
        cur0 = cur0_host if kept and cur0_host is not None else copy_blobs(ctx, N, kept)
    return HistoryBlock(rows, 0, ctx.empty((rows, N * ndim)), ctx.empty((rows, N)),
                        [ctx.empty((rows, N * k.m)) for k in kept], thin_by, own, shared_rows, cur0)


@dataclasses.dataclass
class Books:
    """the host's books at a checkpoint.  From ``take``: the sampler's and the loop's counters,
    the length of the pending history and the block being written with its rows.  Filled in by
    whoever knows: ``counts`` (the device's NaN / forbidden counters to put back), ``snap`` (the
    index of the launch's copy of the current blobs), ``launch`` (the launch's number), ``it``
    (the step of the call it started at), ``status`` (what it gave up with), ``ensemble`` (the
    kept ensemble of a shared loop)."""
    iteration: int
    steps_total: int
    nlc: int
    nwe: int
    rl: int
    nan_pending: int
    forbidden_pending: int
    hist_len: int
    block: HistoryBlock = None
    block_n: int = None
    counts: tuple = None
    snap: int = None
    launch: int = None
    it: int = None
    status: int = None
    ensemble: EnsembleCopy = None

    @classmethod
    def take(cls, s, loop, block=None, counts=None):
        return cls(s.iteration, s.steps_total, s.n_lnprob_calls, s.n_walker_evals,
                   loop.resident_launches, loop._nan_pending, loop._forbidden_pending,
                   len(loop.hist), block, block.n if block is not None else None, counts)

    def put_back(self, s, loop):
        s.iteration, s.steps_total = self.iteration, self.steps_total
        s.n_lnprob_calls, s.n_walker_evals = self.nlc, self.nwe
        loop.resident_launches = self.rl
        loop._nan_pending, loop._forbidden_pending = self.nan_pending, self.forbidden_pending
        loop.hist = loop.hist[:self.hist_len]  # (what predates the checkpoint stays)
        if self.block is not None:
            self.block.n = self.block_n


@dataclasses.dataclass
class JournalEntry:
    """a sample() call of a shared ensemble since the kept state: the steps it has MADE so far"""
    made: int
    store: bool
    yield_every: int
    thin_by: int

    def replay_calls(self):
        """(rows, store, thin_by) of the calls that make the steps again: the same rows stored,
        every thin_by-th; steps past the last stored row of a call that was left early are made
        without a history"""
        tb = self.thin_by
        return (self.made // tb, self.store, tb), (self.made % tb, False, 1)


class LaunchQueue:
    """launches of a one-GPU resident loop that are not yet known to have ended well, oldest
    first, and the number of launches queued so far (the library counts them the same way)"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.count, self._pending = 0, []

    @property
    def queued(self):
        return len(self._pending)

    def launched(self):
        """a launch was queued -> its number"""
        self.count += 1
        return self.count

    def push(self, rec):
        """``rec`` (a Books with its ``launch`` number) is to be settled, behind those queued"""
        self._pending.append(rec)

    def drop(self):
        """nothing queued is waited for any more (the numbering goes on)"""
        self._pending = []

    def settle(self, keep, report):
        """wait until all but the last ``keep`` queued launches are known to have ended
        (``report(launch number)`` -> (status, (NaN, forbidden) counts before it)); None, or the
        record of the first one that gave up (it and everything queued behind it are void)"""
        while len(self._pending) > keep:
            rec = self._pending[0]
            status, before = report(rec.launch)
            if status != 0:
                rec.status, rec.counts = status, before
                return rec
            self._pending.pop(0)
        return None

    def void_from(self, rec):
        """how many queued launches are void when ``rec`` gave up: it and those behind it"""
        return sum(1 for r in self._pending if r.launch >= rec.launch)
