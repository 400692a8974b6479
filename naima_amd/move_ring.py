"""The move stream on the device: a ring of stretch-move random numbers in HBM and the markers
that say which of its bytes a launch or an upload may still be using."""
import itertools


class MoveRing:
    # the random numbers of up to KSTEPS ensemble steps travel as ONE block; room for MOVES_CAP
    # steps: the resident loop keeps the stream's next steps on the device ahead of time
    KSTEPS = 32
    MOVES_CAP = 4 * KSTEPS

    def __init__(self, ctx, ns):
        self.ctx = ctx
        self.step_bytes = 8 * 2 * 3 * ns
        # one spare slice: the fused move kernel proposes the half-step AFTER the one it
        # accepts, so the last one of a block reads (and discards) slice 2*KSTEPS
        self.blk = ctx.empty((2 * self.MOVES_CAP + 1, 3 * ns))
        ctx.call("nh_memset", self.blk, 0, self.blk.nbytes)
        self._blk_tmp = None
        self._launch_marks = itertools.cycle([ctx.marker() for _ in range(3)])
        # markers behind the uploads, in rotation; the ones not yet waited for, oldest first
        self._markers = itertools.cycle([ctx.marker() for _ in range(4)])
        self._inflight = []
        self.reset()

    # ---------------------------------------------------------------- the resident loop
    def reserve(self, moves, want):
        """`want` steps on the device behind `used`, their upload ahead in the stream -> their slice"""
        need = want - (self.have - self.used)
        if need > 0:
            # (the generator hands its stream out in pieces that end at its own block
            # boundaries: they land side by side in `blk` and run as ONE launch)
            if self.have + need > self.MOVES_CAP:
                self._to_front()
            self._append(moves, need, ahead=False)
        self._wait_ahead()
        return 2 * self.used

    def launched(self, moves, want):
        """a launch that consumes `want` steps has been queued"""
        self.used += want
        # a marker behind this launch: `blk` is a ring, and the host runs launches ahead of
        # the device -- an upload on the copy stream may overlap THIS launch (whose steps lie
        # below `have`), but must wait for every earlier one, which may still be reading the
        # very bytes it is about to overwrite once the ring has wrapped
        self.prev = self.last
        self.last = next(self._launch_marks)
        self.ctx.call("nh_marker_record", self.last)
        if self.have - self.used < self.KSTEPS and self.have + self.KSTEPS <= self.MOVES_CAP:
            self._append(moves, self.KSTEPS, ahead=True)

    # --------------------------------------------------------------- the per-launch loop
    def forget_launches(self):
        """whatever ran before the next ahead-upload is ordered ahead of the launch it follows"""
        self.prev = self.last = None

    def next_block(self, moves, limit):
        """the next K <= min(KSTEPS, limit) steps at the front of `blk` -> K"""
        self._drain(1)
        left = self.have - self.used
        if left > 0:
            # steps the resident loop uploaded ahead and did not use: they come first
            K = min(left, self.KSTEPS, limit)
            self._to_front(K)
        else:
            self.have = self.used = 0
            addr, K = moves.take(min(self.KSTEPS, limit))
            self.ctx.call("nh_upload", self.blk, addr, self.step_bytes * K)
        return K

    def block_mark(self):
        """the marker to record behind the upload just queued (any later point is as good)"""
        self._inflight.append(next(self._markers))
        return self._inflight[-1]

    def reset(self):
        """every upload done, nothing on the device"""
        self._drain(0)
        # steps on the device / consumed / last ahead marker / markers behind the last two launches
        self.have = self.used = 0
        self.ahead = self.prev = self.last = None

    # ------------------------------------------------------------------------------ pieces
    # nh_moves_take's contract: only the copy of the MOST RECENT take may still be queued when the
    # next one is taken (the generator hands a used-up block back one block late, so that copy's
    # source is still intact); every earlier upload has to be complete -- _drain(1) before a take
    def _drain(self, keep):
        while len(self._inflight) > keep:
            self.ctx.call("nh_marker_wait", self._inflight.pop(0))

    def _wait_ahead(self):
        if self.ahead is not None:  # the main stream waits for the copy stream's last upload
            self.ctx.call("nh_stream_wait_marker", self.ahead)
            self.ahead = None

    def _append(self, moves, n, ahead):
        """the stream's next n steps behind the ones `blk` holds; ahead: on the copy stream,
        beside the running launch (nh_upload_ahead), else on the main stream"""
        ctx, done = self.ctx, 0
        while done < n:
            self._drain(1)
            addr, got = moves.take(n - done)
            mark = self.block_mark()
            dst = self.blk.ptr + self.step_bytes * self.have
            if ahead:
                # (the first ahead-upload of a loop waits for the launch just queued: whatever
                # ran before it -- the per-launch loop's graphs read `blk` too -- is then done)
                ctx.call("nh_upload_ahead", dst, addr, self.step_bytes * got, mark,
                         self.prev if self.prev is not None else self.last)
                self.ahead = mark
            else:
                ctx.call("nh_upload", dst, addr, self.step_bytes * got)
                ctx.call("nh_marker_record", mark)
            self.have += got
            done += got

    def _to_front(self, k=None):
        """the unused steps `blk` holds (the first k of them) move to its front, in stream order
        behind whatever still reads the block; with k the loop that follows consumes them"""
        ctx, sb = self.ctx, self.step_bytes
        avail = self.have - self.used
        n = avail if k is None else k
        self._wait_ahead()
        if n > 0 and self.used > 0:
            if self._blk_tmp is None:
                self._blk_tmp = ctx.empty((2 * self.MOVES_CAP, self.blk.shape[1]))
            ctx.call("nh_copy", self._blk_tmp, self.blk.ptr + sb * self.used, sb * n)
            ctx.call("nh_copy", self.blk, self._blk_tmp, sb * n)
        if k is None:
            self.have, self.used = avail, 0
        else:
            self.used += k  # (what is left stays where it is, behind the part now at the front)
            if self.used == self.have:
                self.have = self.used = 0
