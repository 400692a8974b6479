"""The function, starts and option sets that test_simplex_host.py and test_gpu_simplex.py share."""
import numpy as np

OPTION_SETS = (dict(xtol=1e-1, ftol=1e-3, maxfev=500), dict(xtol=1e-6, ftol=1e-8, maxfev=60), dict())
FROZEN_OPTS = dict(xtol=1e-4, ftol=1e-6, maxfev=400)


def f3(x):
    """test_host.py's function of three coordinates"""
    return 100 * (x[1] - x[0] ** 2) ** 2 + (1 - x[0]) ** 2 + 3 * (x[2] - 2) ** 2 + 1


def fb3(X):
    return np.array([f3(x) for x in X])


def fb3_region(bad):
    """f3 with the region x0 <= -1.5 returning ``bad`` (NaN or +inf)"""
    def fb(X):
        return np.array([bad if x[0] <= -1.5 else f3(x) for x in X])
    return fb


def starts37():
    rng = np.random.default_rng(20261020)
    cols = [rng.uniform(-2, 2, 37), rng.uniform(-1, 3, 37), rng.uniform(-1, 4, 37)]
    starts = np.stack(cols, axis=1)
    starts[5, 2] = 0.0
    return starts


def frozen42():
    """x2 frozen at each of 7 values from each of 6 starts: (starts, frozen, values)"""
    s6 = starts37()[:6, :2]
    starts, values = [], []
    for v in np.linspace(0.5, 3.5, 7):
        for xy in s6:
            starts.append([xy[0], xy[1], v])
            values.append([0.0, 0.0, v])
    frozen = np.zeros((42, 3), dtype=bool)
    frozen[:, 2] = True
    return np.array(starts), frozen, np.array(values)


def same(a, b, keys=("x", "fun", "nfev", "nit", "status")):
    """bitwise equality of two results over the simplexes"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if x.dtype.kind == "f":
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), \
                (k, np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[:5])
        else:
            assert np.array_equal(x, y), (k, np.flatnonzero(x != y)[:5], x[x != y][:5], y[x != y][:5])
