"""Test infrastructure: S Nelder-Mead searches advanced in lock-step, in NumPy -- what
naima_amd/csrc/nh_simplex.hip does on the device, restated from naima_amd/neldermead.py.

Simplex s is ``minimize_batched`` on the reduced function of its free coordinates, with the two
rules the kernels fix: a function value that is NaN counts as +inf, and the sort is
``np.argsort(kind="stable")`` (the replaced point sits last before the sort).  The points are
evaluated in exactly the batches the device loop evaluates, column for column -- the initial
points ``X[p * S + s]`` (the start itself for p > n_free(s)), the four candidates of an
iteration ``X[c * S + s]`` (a finished simplex: its best point four times), and the points of a
shrink ``X[(j - 1) * ns + k]`` for the k-th of the ns simplexes that asked for one, in index
order -- so that a batched function that is evaluated by the device gives the same bits.
Only tests may import it.
"""
import numpy as np

RHO, CHI, PSI, SIGMA = 1.0, 2.0, 0.5, 0.5
NONZDELT, ZDELT = 0.05, 0.00025


def _clean(f, m):
    f = np.array(f, dtype=float).reshape(-1)
    assert f.shape == (m,)
    f[np.isnan(f)] = np.inf
    return f


def minimize_lockstep(fbatch, starts, frozen=None, values=None, xtol=1e-4, ftol=1e-4, maxiter=None,
                      maxfev=None, on_batch=None):
    """``fbatch(X[m, ndim]) -> f[m]``.  Returns dict(x[S, ndim], fun, nfev, nit, status, success)
    as arrays over the S simplexes, ``batches``, the number of calls of ``fbatch``, and ``ties``,
    the number of sorts that met two equal function values (where a stable and an unstable sort
    may differ)."""
    starts = np.atleast_2d(np.array(starts, dtype=float))
    S, D = starts.shape
    frozen = np.zeros((S, D), dtype=bool) if frozen is None else \
        np.broadcast_to(np.asarray(frozen, dtype=bool), (S, D))
    x0 = starts.copy() if values is None else \
        np.where(frozen, np.broadcast_to(np.asarray(values, dtype=float), (S, D)), starts)
    free = [np.flatnonzero(~frozen[s]) for s in range(S)]
    N = [len(f) for f in free]
    assert min(N) >= 1
    nmax = max(N)
    maxit = [n * 200 if maxiter is None else maxiter for n in N]
    maxfe = [n * 200 if maxfev is None else maxfev for n in N]
    calls, ties = [0], [0]

    def evaluate(X):
        calls[0] += 1
        if on_batch is not None:
            on_batch(X)
        return _clean(fbatch(X), len(X))

    def full(s, y):
        x = x0[s].copy()
        x[free[s]] = y
        return x

    def finished(s):
        """neldermead.py:36-38 and :75: None while the search goes on"""
        if not (nfev[s] < maxfe[s] and nit[s] < maxit[s]):
            return 1 if nfev[s] >= maxfe[s] else 2
        a, f = sim[s], fsim[s]
        with np.errstate(divide="ignore", invalid="ignore"):
            if (np.max(np.abs((a[1:] - a[0]) / a[0])) <= xtol
                    and np.max(np.abs((f[0] - f[1:]) / f[0])) <= ftol):
                return 0
        return None

    def sort(s):
        ties[0] += len(np.unique(fsim[s])) < len(fsim[s])
        order = np.argsort(fsim[s], kind="stable")
        sim[s], fsim[s] = sim[s][order], fsim[s][order]

    # the initial simplexes, one batch
    sim, fsim = [], [None] * S
    X = np.empty(((nmax + 1) * S, D))
    for s in range(S):
        y0 = x0[s, free[s]]
        a = np.tile(y0, (N[s] + 1, 1))
        for k in range(N[s]):
            a[k + 1, k] = (1 + NONZDELT) * y0[k] if y0[k] != 0 else ZDELT
        sim.append(a)
        for p in range(nmax + 1):
            X[p * S + s] = full(s, a[p]) if p <= N[s] else x0[s]
    f = evaluate(X)
    nfev, nit, status = [0] * S, [1] * S, [None] * S
    for s in range(S):
        fsim[s] = f[np.arange(N[s] + 1) * S + s]
        nfev[s] = N[s] + 1
        sort(s)
        status[s] = finished(s)

    while any(st is None for st in status):
        X = np.empty((4 * S, D))
        cands = [None] * S
        for s in range(S):
            if status[s] is not None:
                X[s::S] = full(s, sim[s][0])
                continue
            xbar = np.add.reduce(sim[s][:-1], 0) / N[s]
            worst = sim[s][-1]
            cands[s] = np.stack([(1 + RHO) * xbar - RHO * worst,
                                 (1 + RHO * CHI) * xbar - RHO * CHI * worst,
                                 (1 + PSI * RHO) * xbar - PSI * RHO * worst,
                                 (1 - PSI) * xbar + PSI * worst])
            for c in range(4):
                X[c * S + s] = full(s, cands[s][c])
        f = evaluate(X)
        shrinkers = []
        for s in range(S):
            if status[s] is not None:
                continue
            fxr, fxe, fxc, fxcc = f[s], f[S + s], f[2 * S + s], f[3 * S + s]
            a, fs, cand = sim[s], fsim[s], cands[s]
            nfev[s] += 1
            shrink = False
            if fxr < fs[0]:
                nfev[s] += 1
                if fxe < fxr:
                    a[-1], fs[-1] = cand[1], fxe
                else:
                    a[-1], fs[-1] = cand[0], fxr
            elif fxr < fs[-2]:
                a[-1], fs[-1] = cand[0], fxr
            else:
                nfev[s] += 1
                if fxr < fs[-1]:
                    if fxc <= fxr:
                        a[-1], fs[-1] = cand[2], fxc
                    else:
                        shrink = True
                elif fxcc < fs[-1]:
                    a[-1], fs[-1] = cand[3], fxcc
                else:
                    shrink = True
            if shrink:
                shrinkers.append(s)
            else:
                sort(s)
                nit[s] += 1
                status[s] = finished(s)
        if shrinkers:
            ns = len(shrinkers)
            X = np.empty((nmax * ns, D))
            for k, s in enumerate(shrinkers):
                sim[s][1:] = sim[s][0] + SIGMA * (sim[s][1:] - sim[s][0])
                for j in range(1, nmax + 1):
                    X[(j - 1) * ns + k] = full(s, sim[s][j] if j <= N[s] else sim[s][0])
            f = evaluate(X)
            for k, s in enumerate(shrinkers):
                fsim[s][1:] = f[np.arange(N[s]) * ns + k]
                nfev[s] += N[s]
                sort(s)
                nit[s] += 1
                status[s] = finished(s)

    status = np.array(status, dtype=np.int64)
    return dict(x=np.array([full(s, sim[s][0]) for s in range(S)]),
                fun=np.array([fsim[s][0] for s in range(S)]), nfev=np.array(nfev, dtype=np.int64),
                nit=np.array(nit, dtype=np.int64), status=status, success=status == 0,
                batches=calls[0], ties=ties[0])
