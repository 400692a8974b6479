"""Host arithmetic of an ensemble shared by several ranks: what a rank's launches left on ITS device
only is completed from the other ranks' (``group.allgather_bytes``).  Collective, all of it."""
import numpy as np

# a gathered message is every rank's part together, and the control plane refuses messages
# beyond 64 MiB: the merges travel in slabs of at most this many bytes per rank
SLAB_BYTES = 16 << 20


def sum_over_ranks(group, values):
    """sum over the ranks of a small array of integers -> int64 array"""
    mine = np.ascontiguousarray(values, dtype=np.int64)
    return sum(np.frombuffer(p_, dtype=np.int64).reshape(mine.shape)
               for p_ in group.allgather_bytes(mine.tobytes()))


def merge_current_blobs(group, rank, stamps, hosts):
    """every rank's current blobs := the blobs of where each walker IS -- held by the rank that
    accepted its last move (largest of the ranks' `stamps` [N] int32; below 0: nobody has, and
    every rank's row stands).  hosts[b] [N][m_b]: this rank's copies, completed in place."""
    allst = np.array([np.frombuffer(p_, dtype=np.int32) for p_ in
                      group.allgather_bytes(stamps.tobytes())])
    owner, has = allst.argmax(axis=0), allst.max(axis=0) >= 0
    mine = has & (owner == rank)
    idx = np.arange(len(stamps))
    for host in hosts:
        m = host.shape[1]
        step = max(1, SLAB_BYTES // (8 * m))
        for lo in range(0, len(stamps), step):
            slab = (idx >= lo) & (idx < lo + step)
            parts = group.allgather_bytes(np.ascontiguousarray(host[mine & slab]).tobytes())
            for r, p_ in enumerate(parts):
                if r != rank:
                    host[has & (owner == r) & slab] = np.frombuffer(p_, dtype=float).reshape(-1, m)


def merge_history_rows(group, rank, own, shared_rows, cur0, c, l, per):
    """the rows a shared ensemble's launches wrote, gathered from the ranks that moved each
    walker (c [n][N][ndim], l [n][N], per[b] [n][N][m_b]: this rank's copies, completed in
    place), blob rows of rejected moves filled from the row before (cur0[b] [N][m_b] before the
    first).  own [n][N]: -1 | 0 | 1 where this rank did not move | moved | moved and accepted,
    in the rows [r0, r1) of `shared_rows`; any other row is whole on every rank."""
    n, N, ndim = c.shape
    valid = np.zeros(n, dtype=bool)
    for r0, r1 in shared_rows:
        valid[r0:r1] = True
    own[~valid] = -1
    ms = [p_.shape[2] for p_ in per]
    moved, acc = own >= 0, own > 0
    rows_per = max(1, SLAB_BYTES // (N * (8 * (ndim + 1 + sum(ms)) + 1)))
    for t0 in range(0, n, rows_per):
        t1 = min(n, t0 + rows_per)
        mv, ac = moved[t0:t1], acc[t0:t1]
        flags = own[t0:t1].astype(np.int8).tobytes()
        flags += b"\0" * (-len(flags) % 8)
        payload = flags + c[t0:t1][mv].tobytes() + l[t0:t1][mv].tobytes() + \
            b"".join(p_[t0:t1][ac].tobytes() for p_ in per)
        for r, blob in enumerate(group.allgather_bytes(payload)):
            if r == rank:
                continue
            nel = (t1 - t0) * N
            o = np.frombuffer(blob, dtype=np.int8, count=nel).reshape(t1 - t0, N)
            off = nel + (-nel % 8)
            mv_r, ac_r = o >= 0, o > 0
            cnt, cnta = int(mv_r.sum()), int(ac_r.sum())
            c[t0:t1][mv_r] = np.frombuffer(blob, dtype=float, count=cnt * ndim,
                                           offset=off).reshape(cnt, ndim)
            off += 8 * cnt * ndim
            l[t0:t1][mv_r] = np.frombuffer(blob, dtype=float, count=cnt, offset=off)
            off += 8 * cnt
            for p_, m in zip(per, ms):
                p_[t0:t1][ac_r] = np.frombuffer(blob, dtype=float, count=cnta * m,
                                                offset=off).reshape(cnta, m)
                off += 8 * cnta * m
            moved[t0:t1] |= mv_r
            acc[t0:t1] |= ac_r
    for t in range(n if per else 0):
        rej = moved[t] & ~acc[t]
        if rej.any():
            for p_, c0 in zip(per, cur0):
                p_[t][rej] = (p_[t - 1] if t > 0 else c0)[rej]
