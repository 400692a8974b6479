"""The device loop's book-keeping records (naima_amd/loop_books.py), without a GPU.

The records live on a stub context in the style of test_lazy_host.py's: "device memory" is a set of
NumPy arrays behind made-up addresses, and ``call`` restates the one entry point the records use
(nh_copy: bytes from one address to another, in order) and keeps a list of the calls.  Each layout
is compared against the expression the loop spelled out by hand before the records existed.
"""
import ctypes as C
import types

import numpy as np
import pytest

from naima_amd import loop_books as LB
from naima_amd.loop_books import Books, EnsembleCopy, HistoryBlock, JournalEntry, KeptBlob, LaunchQueue


class Buf:
    def __init__(self, ptr, host):
        self.ptr, self.host, self.shape, self.dtype = ptr, host, host.shape, host.dtype

    def get(self):
        return self.host.copy()


class StubCtx:
    """device memory as NumPy arrays behind made-up addresses; call() restates nh_copy"""

    def __init__(self):
        self.bufs, self.next, self.copies = [], 0x10000, []

    def array(self, a, dtype=np.float64):
        host = np.ascontiguousarray(a, dtype=dtype).copy()
        b = Buf(self.next, host)
        self.next += host.nbytes + 4096
        self.bufs.append(b)
        return b

    def empty(self, shape, dtype=np.float64):
        return self.array(np.full(shape, -7), dtype)  # (never a value the tests write)

    def raw(self, x, nbytes):
        """the nbytes bytes at an address (or at the start of a buffer), as a writable view"""
        ptr = x.ptr if isinstance(x, Buf) else x
        for b in self.bufs:
            if b.ptr <= ptr and ptr + nbytes <= b.ptr + b.host.nbytes:
                return b.host.reshape(-1).view(np.uint8)[ptr - b.ptr:ptr - b.ptr + nbytes]
        raise AssertionError("%d bytes at %#x are not device memory" % (nbytes, ptr))

    def call(self, name, dst, src, nbytes):
        assert name == "nh_copy", "unexpected library call %s" % name
        self.copies.append(nbytes)
        self.raw(dst, nbytes)[:] = self.raw(src, nbytes)


N, NDIM = 6, 3
RNG = np.random.default_rng(7)


def kept_blobs(ctx, widths):
    return [KeptBlob(ctx.array(RNG.normal(size=(N, m))), m, None, (m,) if m > 1 else ())
            for m in widths]


def filled_block(ctx, kept, rows, n, **kw):
    block = LB.new_block(ctx, N, NDIM, kept, rows, **kw)
    for b in [block.coords, block.logp] + block.blobs:
        b.host[:] = RNG.normal(size=b.shape)
    block.n = n
    return block


# ------------------------------------------------------------------ the history block
@pytest.mark.parametrize("nblobs", [0, 1, 4])
@pytest.mark.parametrize("dev_hist", [False, True])
@pytest.mark.parametrize("blob_dev_hist", [False, True])
def test_history_words(nblobs, dev_hist, blob_dev_hist):
    ctx = StubCtx()
    block = LB.new_block(ctx, N, NDIM, kept_blobs(ctx, [2] * nblobs), 11)
    words = block.words(dev_hist, blob_dev_hist)
    if not dev_hist:
        want = [0] * 8
    else:
        want = [block.coords.ptr, block.logp.ptr, 0, 11]
        want += [b.ptr for b in block.blobs] if blob_dev_hist else []
        want += [0] * (8 - len(want))
    assert words == want and len(words) == 8
    assert list((C.c_longlong * 8)(*words)) == want  # (what nh_set_words takes them as)


@pytest.mark.parametrize("nblobs", [0, 1, 4])
def test_run_arguments(nblobs):
    ctx = StubCtx()
    block = LB.new_block(ctx, N, NDIM, kept_blobs(ctx, [1, 3, 2, 5][:nblobs]), 9)
    block.n = 4
    hc, hl, hb, row0, cap = block.run_args()
    assert (hc, hl, row0, cap) == (block.coords.ptr, block.logp.ptr, 4, 9)
    if nblobs == 0:
        assert hb is None
    else:
        assert len(hb) == 4
        assert list(hb) == [b.ptr for b in block.blobs] + [None] * (4 - nblobs)
    # a launch that keeps no history: the same five arguments, nothing to write to
    assert len(LB.NO_HISTORY) == 5 and not any(LB.NO_HISTORY)


def test_shared_fields_come_together():
    ctx = StubCtx()
    kept = kept_blobs(ctx, [2])
    plain = LB.new_block(ctx, N, NDIM, kept, 5)
    assert not plain.shared and (plain.own, plain.shared_rows, plain.cur0) == (None, None, None)
    assert plain.rows == 5 and plain.coords.shape == (5, N * NDIM) and plain.blobs[0].shape == (5, N * 2)
    ctx.copies.clear()
    sh = LB.new_block(ctx, N, NDIM, kept, 5, shared=True)
    assert sh.shared and sh.own.shape == (5, N) and sh.own.dtype == np.int32 and sh.shared_rows == []
    assert ctx.copies == [8 * N * 2] and np.array_equal(sh.cur0[0].host, kept[0].cur.host)
    host = [np.zeros((N, 2))]
    ctx.copies.clear()
    assert LB.new_block(ctx, N, NDIM, kept, 5, shared=True, cur0_host=host).cur0 is host
    assert ctx.copies == []  # (host copies the last merge left: no launch)
    assert LB.new_block(ctx, N, NDIM, [], 5, shared=True, cur0_host=host).cur0 == []
    with pytest.raises(AssertionError):
        HistoryBlock(5, 0, plain.coords, plain.logp, [], own=sh.own)


def test_plain_block():
    ctx = StubCtx()
    block = LB.new_block(ctx, N, NDIM, [], 5)
    assert not block.plain  # (no row yet)
    block.n = 1
    assert block.plain
    assert not LB.new_block(ctx, N, NDIM, [], 5, thin_by=2).plain
    sh = LB.new_block(ctx, N, NDIM, [], 5, shared=True)
    sh.n = 3
    assert not sh.plain
    # (read by name too, as while it was a dict)
    assert block["n"] == 1 and block.get("thin_by", 1) == 1 and block.get("own") is None


@pytest.mark.parametrize("state,blobs", [(True, True), (True, False), (False, True), (False, False)])
def test_copy_row(state, blobs):
    ctx = StubCtx()
    kept = kept_blobs(ctx, [1, 3])
    block = filled_block(ctx, kept, 4, 2)
    before = [b.host.copy() for b in [block.coords, block.logp] + block.blobs]
    coords, logp = ctx.array(RNG.normal(size=N * NDIM)), ctx.array(RNG.normal(size=N))
    block.copy_row(ctx, N, NDIM, coords, logp, kept, state=state, blobs=blobs)
    want = ([8 * N * NDIM, 8 * N] if state else []) + ([8 * N * 1, 8 * N * 3] if blobs else [])
    assert ctx.copies == want
    new = [coords.host, logp.host] + [k.cur.host.ravel() for k in kept]
    for i, (b, old) in enumerate(zip([block.coords, block.logp] + block.blobs, before)):
        written = state if i < 2 else blobs
        old[2] = new[i] if written else old[2]
        assert np.array_equal(b.host, old)  # (row n, and no other)


def test_thin_segments():
    ctx = StubCtx()
    kept = kept_blobs(ctx, [1, 2, 1, 1, 1, 1, 1])  # 2 + 7 matrices: two launches
    stage, compact = LB.new_block(ctx, N, NDIM, kept, 10), LB.new_block(ctx, N, NDIM, kept, 3)
    parts = stage.thin_segs(compact)
    assert [len(p) for p in parts] == [8, 1]
    got = [(s.src, s.dst, s.width) for p in parts for s in p]
    assert got == [(a.ptr, b.ptr, a.shape[1]) for a, b in
                   zip([stage.coords, stage.logp] + stage.blobs, [compact.coords, compact.logp] + compact.blobs)]


@pytest.mark.parametrize("tb", [1, 5, 33])
@pytest.mark.parametrize("n", [70, 7, 3])
def test_host_rows(tb, n):
    ctx = StubCtx()
    kept = kept_blobs(ctx, [1, 3])
    block = filled_block(ctx, kept, 70, n, thin_by=tb)
    rows = block.host_rows(N, NDIM, kept)
    if n < tb:
        assert rows is None
        return
    c, l, per = rows
    assert np.array_equal(c, block.coords.host[:n][tb - 1::tb].reshape(-1, N, NDIM))
    assert np.array_equal(l, block.logp.host[:n][tb - 1::tb])
    assert [a.shape for a in per] == [(len(c), N, 1), (len(c), N, 3)]
    for a, hb in zip(per, block.blobs):
        assert np.array_equal(a.reshape(len(c), -1), hb.host[:n][tb - 1::tb])
    assert len(c) == n // tb


def test_host_rows_of_an_empty_block():
    ctx = StubCtx()
    assert LB.new_block(ctx, N, NDIM, [], 4).host_rows(N, NDIM, []) is None


def test_merge_sees_full_rate_rows_before_thinning():
    ctx = StubCtx()
    kept = kept_blobs(ctx, [2])
    block = filled_block(ctx, kept, 20, 17, thin_by=5, shared=True)
    block.shared_rows.append((0, 17))
    block.own.host[:] = np.arange(20 * N).reshape(20, N)
    seen = []

    def merge(own, shared_rows, cur0, c, l, per):
        seen.append((own.shape, shared_rows, [type(b) for b in cur0], c.shape, l.shape, per[0].shape))
        assert np.array_equal(own, block.own.host[:17])
        assert np.array_equal(cur0[0], kept[0].cur.host)
        c[16] = 1.5  # (completed in place: what the thinned rows are taken from)

    c, l, per = block.host_rows(N, NDIM, kept, merge)
    assert seen == [((17, N), [(0, 17)], [np.ndarray], (17, N, NDIM), (17, N), (17, N, 2))]
    assert c.shape == (3, N, NDIM)  # rows 4, 9, 14 of 17: what the merge wrote into row 16 is gone,
    assert not np.any(c == 1.5)     # ... and what it writes into a kept row is kept
    c, l, per = block.host_rows(N, NDIM, kept, lambda own, sr, cur0, c, l, per: c.__setitem__(14, 2.5))
    assert np.all(c[2] == 2.5) and not np.any(c[:2] == 2.5)
    # a block that is not shared is not merged, whatever the loop passes
    plain = filled_block(ctx, kept, 20, 17)
    plain.host_rows(N, NDIM, kept, merge)
    assert len(seen) == 1


# ------------------------------------------------------------------ the checkpoint
def test_books_are_put_back():
    ctx = StubCtx()
    old = LB.new_block(ctx, N, NDIM, [], 4)
    old.n = 4
    block = LB.new_block(ctx, N, NDIM, [], 8)
    block.n = 3
    s = types.SimpleNamespace(iteration=10, steps_total=30, n_lnprob_calls=60, n_walker_evals=360)
    loop = types.SimpleNamespace(resident_launches=2, _nan_pending=1, _forbidden_pending=5,
                                 hist=[old, block])
    books = Books.take(s, loop, block)
    assert (books.counts, books.snap, books.launch, books.it, books.status, books.ensemble) == (None,) * 6
    assert Books.take(s, loop, None, counts=(0, 0)).counts == (0, 0)
    assert Books.take(s, loop).block_n is None
    s.iteration, s.steps_total, s.n_lnprob_calls, s.n_walker_evals = 42, 62, 124, 744
    loop.resident_launches, loop._nan_pending, loop._forbidden_pending = 4, 0, 0
    block.n = 8
    loop.hist.append(LB.new_block(ctx, N, NDIM, [], 2))
    books.put_back(s, loop)
    assert vars(s) == dict(iteration=10, steps_total=30, n_lnprob_calls=60, n_walker_evals=360)
    assert (loop.resident_launches, loop._nan_pending, loop._forbidden_pending) == (2, 1, 5)
    assert len(loop.hist) == 2 and loop.hist[0] is old and loop.hist[1] is block
    assert block.n == 3 and old.n == 4  # (what predates the checkpoint is untouched)


# ------------------------------------------------------------------ the ensemble's copy
def test_ensemble_copy_round_trip():
    ctx = StubCtx()
    kept = kept_blobs(ctx, [1, 4])
    coords, logp = ctx.array(RNG.normal(size=N * NDIM)), ctx.array(RNG.normal(size=N))
    nacc = ctx.array(np.arange(N), dtype=np.int32)
    live = [coords, logp, nacc] + [k.cur for k in kept]
    first = [b.host.copy() for b in live]
    sizes = [8 * N * NDIM, 8 * N, 4 * N, 8 * N * 1, 8 * N * 4]
    e = EnsembleCopy.take(ctx, N, NDIM, coords, logp, nacc, kept)
    assert ctx.copies == sizes
    assert e.nacc.dtype == np.int32 and [b.shape for b in e.blobs] == [(N, 1), (N, 4)]
    for b in live:
        b.host[:] = 3
    ctx.copies.clear()
    e.put_back(ctx, coords, logp, nacc, kept)
    assert ctx.copies == sizes
    for b, want in zip(live, first):
        assert b.host.tobytes() == want.tobytes()


def test_blob_copies_reuse_their_buffers():
    ctx = StubCtx()
    kept = kept_blobs(ctx, [2, 3])
    first = [k.cur.host.copy() for k in kept]
    copies = LB.copy_blobs(ctx, N, kept)
    again = LB.copy_blobs(ctx, N, kept, copies)  # (a set of the ring, used a second time)
    assert again is copies and ctx.copies == [8 * N * 2, 8 * N * 3] * 2
    for k in kept:
        k.cur.host[:] = 0
    LB.copy_blobs(ctx, N, kept, copies, back=True)
    assert all(k.cur.host.tobytes() == f.tobytes() for k, f in zip(kept, first))
    assert LB.copy_blobs(ctx, N, []) == []


# ------------------------------------------------------------------ journal, constants, queue
@pytest.mark.parametrize("made", [0, 4, 14, 17])
@pytest.mark.parametrize("tb", [1, 5])
def test_journal_replay_split(made, tb):
    j = JournalEntry(0, True, 3, tb)
    j.made += made
    assert j.replay_calls() == ((made // tb, True, tb), (made % tb, False, 1))
    stored, rest = j.replay_calls()
    assert stored[0] * tb + rest[0] == made and rest[0] < tb


K0, K1 = "kept0", "kept1"
CONST_CASES = [  # (positions of the constant blobs, kept blobs, the model's blobs in order)
    ([0], 0, ["c0"]), ([0], 1, ["c0", K0]), ([0], 2, ["c0", K0, K1]),
    # (a position past the end, which no model has, appends)
    ([1], 0, ["c1"]), ([1], 1, [K0, "c1"]), ([1], 2, [K0, "c1", K1]),
    ([0, 2], 0, ["c0", "c2"]), ([0, 2], 1, ["c0", K0, "c2"]), ([0, 2], 2, ["c0", K0, "c2", K1]),
]


@pytest.mark.parametrize("positions,nkept,want", CONST_CASES)
def test_constant_blobs_go_back_to_their_positions(positions, nkept, want):
    given = [K0, K1][:nkept]
    out = LB.with_const_blobs(given, [(j, float(j)) for j in positions], lambda v: "c%d" % v)
    assert out is given and out == want


def queue_of(n):
    q, recs = LaunchQueue(), []
    for it in range(n):
        rec = Books(0, 0, 0, 0, 0, 0, 0, 0)
        rec.launch, rec.it = q.launched(), 10 * it
        q.push(rec)
        recs.append(rec)
    return q, recs


def test_launch_queue_settles_all_but_the_last():
    q, recs = queue_of(3)
    asked = []

    def report(launch):
        asked.append(launch)
        return 0, (0, 0)

    assert q.queued == 3 and q.count == 3
    assert q.settle(1, report) is None
    assert asked == [1, 2] and q.queued == 1 and q.void_from(recs[0]) == 1  # (launch 3 is left)
    assert q.settle(0, report) is None and asked == [1, 2, 3] and q.queued == 0
    assert q.count == 3 and q.launched() == 4  # (numbered on from where the loop stands)
    q.push(recs[0])
    q.drop()
    assert (q.count, q.queued) == (4, 0)  # (dropped: nothing is waited for, the numbering goes on)
    q.reset()
    assert (q.count, q.queued) == (0, 0)


@pytest.mark.parametrize("keep", [0, 1])
def test_launch_queue_returns_the_first_launch_that_gave_up(keep):
    q, recs = queue_of(3)
    script = {1: (0, (0, 0)), 2: (3, (4, 9)), 3: (3, (4, 9))}
    asked = []

    def report(launch):
        asked.append(launch)
        return script[launch]

    rec = q.settle(keep, report)
    assert asked == [1, 2]  # (nothing behind the first that gave up is asked about)
    assert rec is recs[1] and q.queued == 2 and (rec.launch, rec.it, rec.status, rec.counts) == (2, 10, 3, (4, 9))
    assert q.void_from(rec) == 2  # it and the one queued behind it
    assert q.void_from(recs[2]) == 1
