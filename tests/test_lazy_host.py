"""The fold algebra of naima_amd/darray.py, without a GPU.

A model function's arithmetic on ``pars[i]`` is folded by ``DVec`` into five numbers,
``a * tf(b * x + c)``, which the device code evaluates (nh_lazy_apply, nh_common.h).  Here the
folding itself is held to NumPy: ``DVec``s live on a stub context whose "device memory" is a set
of NumPy arrays behind made-up addresses and whose ``call`` restates the glue kernels
(nh_pack_rows, nh_ew_binary, nh_lincomb; nh_device.hip) in NumPy and counts them.  The SAME
Python expression is applied to the device values and to the host arrays, and the folded
``(a, b, c, tf)`` is evaluated by ``lazy_apply_np``, a NumPy restatement of nh_lazy_apply.

Tolerance (derived, not measured).  Every operation of the expression costs NumPy one rounding
(half an ulp, 2**-53; a library function up to one ulp), and costs the fold the same rounding in
another place: a scale rounds ``a * k``, a shift ``a * c + k``, and the evaluation adds the three
roundings of ``a * tf(b * x + c)``.  As long as no operation AMPLIFIES the error that came before
it, the two results differ by at most ``(2 + depth) * 2**-52`` relative.  "Does not amplify" is
asserted, not assumed: the evaluator carries, next to every value, the error bound ``e`` of a
float64 evaluation in units of 2**-53, ``e' = cond * e + 1`` with the operation's condition number
at the operand (|v| / |v + k| for a shift, |p| for a power, |v ln base| for base ** v, |v| for exp,
1 / |ln v| for the logarithms, 1/2 for sqrt, 2 for square, 1 for the rest), and every expression
used must end with ``e <= depth`` (so a square may only stand where nothing was rounded before,
a subtraction may not cancel, and 10 ** v needs |v| <= 1 / ln 10).  The random generator draws
operations until one keeps that bound; the bound is asserted again on the finished tree.

Checked on the CPU before relying on it: of the 300 seeded trees 161 fold completely (asserted
>= half); the others reach ``_binary`` / ``dense`` on the stub, which is counted and asserted.

Findings this file pins (test_dmat_operand_dispatch fails in both shapes before the fix):
  * ``dmat / dvec`` downloaded the divisor and took ``1 / array`` for a per-ENERGY factor: on a
    device ValueError "unsupported operand shape (7,) for a device matrix" when N != nE, and
    column k divided by walker k's value when N == nE;
  * ``dvec * dmat`` downloaded the matrix ("cannot combine a device vector of 7 walkers with
    shape (7, 3)").
  On the stub there is nothing to download from, so both show as
  ``AttributeError: 'NoneType' object has no attribute 'nh_download'`` (darray.py, DVec.get).
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from naima_amd import darray as D
from naima_amd.darray import DMat, DPars, DVec

EPS = 2.0 ** -52


# ------------------------------------------------------------------ the stub device
def lazy_apply_np(a, b, c, tf, raw):
    """nh_lazy_apply (nh_common.h) in NumPy"""
    with np.errstate(all="ignore"):
        x = b * raw + c
        x = [lambda v: v, lambda v: 10.0 ** v, np.exp, np.log, np.log10, np.sqrt, lambda v: v * v,
             lambda v: 1.0 / v][tf](x)
        return a * x


class Buf:
    def __init__(self, ptr, host):
        self.ptr, self.host, self.shape = ptr, host, host.shape

    def get(self):
        return self.host.copy()


class StubCtx:
    """device memory as NumPy arrays behind made-up addresses; call() restates the glue kernels"""
    h = None

    def __init__(self):
        self.bufs, self.next, self.calls = [], 0x10000, []

    def array(self, a):
        host = np.ascontiguousarray(a, dtype=float).copy()
        b = Buf(self.next, host)
        self.next += 8 * host.size + 4096
        self.bufs.append(b)
        return b

    def empty(self, shape):
        return self.array(np.full(shape, np.nan))

    const = array

    def flush(self, *bufs):
        pass

    def flat(self, ptr):
        """(flat array, element offset) of the buffer that holds address ptr"""
        for b in self.bufs:
            if b.ptr <= ptr < b.ptr + 8 * b.host.size:
                assert (ptr - b.ptr) % 8 == 0
                return b.host.reshape(-1), (ptr - b.ptr) // 8
        raise AssertionError("address %#x is not device memory" % ptr)

    def lazy(self, z, n):
        if not z.base:
            return np.full(n, z.a)
        flat, off = self.flat(z.base)
        return lazy_apply_np(z.a, z.b, z.c, z.tf, flat[off + z.stride * np.arange(n)])

    def call(self, name, *a):
        self.calls.append(name)
        with np.errstate(all="ignore"):
            if name == "nh_pack_rows":
                cols, ncols, n, out, ld = a
                for j in range(ncols):
                    out.host.reshape(-1)[j + ld * np.arange(n)] = self.lazy(cols[j], n)
            elif name == "nh_ew_binary":
                op, x, y, n, out = a
                x, y = self.lazy(x._obj, n), self.lazy(y._obj, n)
                f = [np.add, np.subtract, np.multiply, np.divide, np.power, np.fmax, np.fmin,
                     np.less, np.less_equal, np.greater, np.greater_equal][op]
                out.host.reshape(-1)[:n] = f(x, y).astype(float)
            elif name == "nh_lincomb":
                comps, ncomp, cf, rf, N, m, out, ldo = a
                s = np.zeros((N, m))
                for j in range(ncomp):
                    flat, off = self.flat(comps[j].ptr)
                    s += comps[j].scale * flat[off + comps[j].ld * np.arange(N)[:, None] + np.arange(m)]
                if cf is not None:
                    s *= cf.host
                if rf:
                    s *= self.lazy(D.nh_lazy.from_address(rf), N)[:, None]
                out.host[:, :m] = s
            else:
                raise AssertionError("unexpected library call %s" % name)


def value(ctx, v):
    """the host values of a DVec: its five numbers through lazy_apply_np"""
    return ctx.lazy(v.lazy(), v.n)


def dmat_value(ctx, m):
    N, n = m.shape
    s = np.zeros((N, n))
    for _, p, ld, sc in m.terms:
        flat, off = ctx.flat(p)
        s += sc * flat[off + ld * np.arange(N)[:, None] + np.arange(n)]
    return s if m.colfac is None else s * m.colfac


X = np.array([[0.53, 0.71, 0.94, 1.18, 1.37, 1.66, 1.93],
              [-1.91, -1.52, -1.13, -0.97, -0.74, -0.61, -0.52],
              [1.21, 0.64, 1.87, 0.55, 1.02, 1.49, 0.83]])


@pytest.fixture()
def dev():
    ctx = StubCtx()
    return ctx, DPars(ctx, ctx.array(X), X.shape[0], X.shape[1])


def close(got, ref, depth):
    ref = np.asarray(ref, dtype=float)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (got, ref)
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= (2 + depth) * EPS * np.abs(ref[fin])), \
        (np.max(err / np.maximum(np.abs(ref[fin]), 1e-300)) / EPS, depth)


def five(v):
    return (v.a, v.b, v.c, v.tf)


# ------------------------------------------------------------------------ the fold rules
# (expression, depth, expected (a, b, c, tf) or None: needs a kernel, leaf, number of kernels)
LN25 = float(np.log(2.5))
RULES = [
    ("scale", lambda p: p * 3.0, 1, (3.0, 1.0, 0.0, D.TF_ID), 0, 0),
    ("rscale", lambda p: 3.0 * p, 1, (3.0, 1.0, 0.0, D.TF_ID), 0, 0),
    ("div", lambda p: p / 4.0, 1, (0.25, 1.0, 0.0, D.TF_ID), 0, 0),
    ("shift-id", lambda p: p * 3.0 + 2.0, 2, (1.0, 3.0, 2.0, D.TF_ID), 0, 0),
    ("shift-zero", lambda p: p * 3.0 + 0.0, 1, (3.0, 1.0, 0.0, D.TF_ID), 0, 0),
    ("sub", lambda p: p - 2.5, 1, (1.0, 1.0, -2.5, D.TF_ID), 1, 0),
    ("shift-transformed", lambda p: 10 ** (p * 0.25) + 1.0, 3, None, 0, 1),
    ("apply", lambda p: np.exp(p * 0.5 + 0.125), 3, (1.0, 0.5, 0.125, D.TF_EXP), 0, 0),
    ("apply-transformed", lambda p: np.log(10 ** p * 8.0), 3, None, 2, 1),
    ("neg", lambda p: -p, 1, (-1.0, 1.0, 0.0, D.TF_ID), 0, 0),
    ("rsub", lambda p: 5.0 - p, 1, (1.0, -1.0, 5.0, D.TF_ID), 1, 0),
    ("rtruediv", lambda p: 2.0 / (p * 4.0), 2, (0.5, 1.0, 0.0, D.TF_RECIP), 0, 0),
    ("rtruediv-affine", lambda p: 2.0 / (p * 4.0 + 1.0), 3, (2.0, 4.0, 1.0, D.TF_RECIP), 0, 0),
    ("rtruediv-a0", lambda p: 2.0 / (p * 0.0), 2, None, 0, 1),
    ("rtruediv-transformed", lambda p: 2.0 / np.sqrt(p), 2, None, 0, 1),
    ("pow1", lambda p: (p * 3.0) ** 1, 1, (3.0, 1.0, 0.0, D.TF_ID), 0, 0),
    ("pow2", lambda p: (p * 3.0) ** 2, 2, (9.0, 1.0, 0.0, D.TF_SQUARE), 0, 0),
    ("pow2-affine", lambda p: (p - 3.0) ** 2, 2, (1.0, 1.0, -3.0, D.TF_SQUARE), 1, 0),
    ("pow0.5", lambda p: (p * 4.0) ** 0.5, 2, (2.0, 1.0, 0.0, D.TF_SQRT), 0, 0),
    ("pow0.5-negative-a", lambda p: (p * -4.0) ** 0.5, 2, None, 1, 1),
    ("pow-1", lambda p: (p * 4.0) ** -1, 2, (0.25, 1.0, 0.0, D.TF_RECIP), 0, 0),
    ("pow-generic", lambda p: p ** 1.75, 1, None, 0, 1),
    ("pow2-transformed", lambda p: np.sqrt(p) ** 2, 2, None, 0, 1),
    ("rpow10", lambda p: 10 ** (p * 0.25), 2, (1.0, 0.25, 0.0, D.TF_POW10), 0, 0),
    ("rpow-e", lambda p: np.e ** (p * 0.5), 2, (1.0, 0.5 * float(np.log(np.e)), 0.0, D.TF_EXP), 0, 0),
    ("rpow-2.5", lambda p: 2.5 ** (p * 0.5), 2, (1.0, 0.5 * LN25, 0.0, D.TF_EXP), 0, 0),
    ("rpow-zero-base", lambda p: 0.0 ** p, 1, None, 0, 1),
    ("rpow-negative-base", lambda p: (-2.0) ** p, 1, None, 0, 1),
    ("chain", lambda p: -(10 ** (2.0 * p - 3.0)) / 4.0, 4, (-0.25, 2.0, -3.0, D.TF_POW10), 2, 0),
]
for _n, _tf in DVec._UFUNCS.items():
    RULES.append(("ufunc-" + _n, (lambda f: lambda p: f(p * 0.5 + 2.75))(getattr(np, _n)), 3,
                  (1.0, 0.5, 2.75, _tf), 0, 0))
RULES.append(("ufunc-negative", lambda p: np.negative(p), 1, (-1.0, 1.0, 0.0, D.TF_ID), 0, 0))


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
def test_fold_rule(dev, rule):
    """one rule of DVec at a time: the five numbers it must produce (or the kernel it must
    reach), and their value against NumPy on the same expression"""
    ctx, P = dev
    _, f, depth, want, leaf, ncalls = rule
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = f(P[leaf])
        ref = f(X[leaf])
    assert isinstance(got, DVec)
    assert len(ctx.calls) == ncalls, ctx.calls
    if want is not None:
        assert five(got) == want
        assert got.ptr == P[leaf].ptr and got.stride == 1
    close(value(ctx, got), ref, depth)


_BIN_NP = {"add": 0, "subtract": 0, "multiply": 0, "true_divide": 0, "divide": 0, "power": 0,
           "less": 0, "less_equal": 0, "greater": 0, "greater_equal": 0}


@pytest.mark.parametrize("name", sorted(DVec._BIN))
@pytest.mark.parametrize("first", [True, False], ids=["device-first", "device-second"])
@pytest.mark.parametrize("other", ["number", "array", "device"])
def test_binary_ufuncs(dev, name, first, other):
    """every entry of DVec._BIN through __array_ufunc__, the device value as first and as second
    operand, against a number (folds where a rule exists), a host array and another device
    value (one nh_ew_binary each)"""
    assert set(_BIN_NP) == set(DVec._BIN)
    ctx, P = dev
    uf = getattr(np, name)
    k = {"number": 1.25, "array": X[2], "device": P[2]}[other]
    kh = X[2] if other == "device" else k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = uf(P[0], k) if first else uf(k, P[0])
        ref = uf(X[0], kh) if first else uf(kh, X[0])
    assert isinstance(got, DVec)
    folds = other == "number" and (name in ("add", "subtract", "multiply")
                                   or name in ("true_divide", "divide")
                                   or (name == "power" and not first))  # (1.25 ** v: EXP)
    assert len(ctx.calls) == (0 if folds else 1), ctx.calls
    assert not ctx.calls or ctx.calls == ["nh_ew_binary"]
    close(value(ctx, got), np.asarray(ref, dtype=float), 2 if name == "power" else 1)


def test_power_of_number_base_folds(dev):
    ctx, P = dev
    got = np.power(10.0, P[0])
    assert five(got) == (1.0, 1.0, 0.0, D.TF_POW10) and not ctx.calls
    got = np.power(P[0], 2)
    assert five(got) == (1.0, 1.0, 0.0, D.TF_SQUARE) and not ctx.calls


# ---------------------------------------------------------------- random expression trees
CONSTS = [0.25, 0.5, 1.5, 2.0, 3.0, -0.5, -2.0, 0.75, -1.25, 4.0]


def _ops(rng):
    """(name, expression on v, condition number at the host values h) of one random operation"""
    k = float(rng.choice(CONSTS))
    base = float(rng.choice([10.0, np.e, 2.5, 2.0]))
    p = float(rng.choice([1, 2, 0.5, -1, 1.75, -0.5]))
    one = lambda h: np.ones_like(h)
    ln = lambda h: 1.0 / np.abs(np.log(h))
    return [
        ("mul", lambda v: v * k, one), ("rmul", lambda v: k * v, one),
        ("div", lambda v: v / k, one), ("rdiv", lambda v: k / v, one),
        ("add", lambda v: v + k, lambda h: np.abs(h) / np.abs(h + k)),
        ("radd", lambda v: k + v, lambda h: np.abs(h) / np.abs(h + k)),
        ("sub", lambda v: v - k, lambda h: np.abs(h) / np.abs(h - k)),
        ("rsub", lambda v: k - v, lambda h: np.abs(h) / np.abs(k - h)),
        ("neg", lambda v: -v, one),
        ("pow", lambda v: v ** p, lambda h: abs(p) * one(h)),
        ("rpow", lambda v: base ** v, lambda h: np.abs(h) * np.log(base)),
        ("exp", np.exp, np.abs), ("log", np.log, ln), ("log10", np.log10, ln),
        ("sqrt", np.sqrt, lambda h: 0.5 * one(h)), ("square", np.square, lambda h: 2.0 * one(h)),
        ("reciprocal", np.reciprocal, one),
        ("np.multiply", lambda v: np.multiply(k, v), one),
        ("np.subtract", lambda v: np.subtract(k, v), lambda h: np.abs(h) / np.abs(k - h)),
    ]


def random_tree(rng, depth):
    """a chain of ``depth`` operations on one leaf, with a second device value joined in at a
    random place in one tree of five: [(name, f, cond)] and the join (position, op, leaf)"""
    leaf = int(rng.integers(0, 3))
    h, e, chain = X[leaf].copy(), 0.0, []
    join = (int(rng.integers(0, depth)), str(rng.choice(["mul", "div"])), int(rng.integers(0, 3))) \
        if rng.random() < 0.2 else None
    for d in range(depth):
        if join and join[0] == d:  # (a product or quotient of two values: e1 + e2 + 1)
            h = h * X[join[2]] if join[1] == "mul" else h / X[join[2]]
            e = e + 1.0
            chain.append(("join", None, None))
            continue
        for _ in range(200):
            name, f, cond = _ops(rng)[int(rng.integers(0, 19))]
            with np.errstate(all="ignore"):
                hn = np.asarray(f(h), dtype=float)
                en = float(np.max(cond(h))) * e + 1.0
            if np.all(np.isfinite(hn)) and np.all(np.abs(hn) > 1e-3) and np.all(np.abs(hn) < 1e6) \
                    and np.isfinite(en) and en <= d + 1:
                break
        else:
            raise AssertionError("no well-conditioned operation found")
        h, e = hn, en
        chain.append((name, f, cond))
    return leaf, chain, join


def run_tree(tree, leaves):
    """the tree's expression on ``leaves`` (host arrays or device values)"""
    leaf, chain, join = tree
    v = leaves[leaf]
    for name, f, _ in chain:
        if name == "join":
            v = v * leaves[join[2]] if join[1] == "mul" else v / leaves[join[2]]
        else:
            v = f(v)
    return v


def tree_bound(tree):
    """the error bound e (units of 2**-53) of a float64 evaluation, recomputed on the tree"""
    leaf, chain, join = tree
    h, e = X[leaf].copy(), 0.0
    for name, f, cond in chain:
        if name == "join":
            h, e = (h * X[join[2]] if join[1] == "mul" else h / X[join[2]]), e + 1.0
        else:
            e = float(np.max(cond(h))) * e + 1.0
            h = np.asarray(f(h), dtype=float)
    return e


def test_random_expression_trees():
    """300 seeded trees of depth 1 .. 4 over the operations above: the device value's five
    numbers (after whatever kernels it needed, restated by the stub) against NumPy on the same
    expression, to (2 + depth) 2**-52; the conditioning that bound needs asserted per tree; a tree
    that does not fold has reached _binary / dense (counted), and at least half fold"""
    rng = np.random.default_rng(20240607)
    folded = eager = 0
    worst = 0.0
    for t in range(300):
        depth = 1 + t % 4
        tree = random_tree(rng, depth)
        assert tree_bound(tree) <= depth, [c[0] for c in tree[1]]
        ctx = StubCtx()
        P = DPars(ctx, ctx.array(X), 3, X.shape[1])
        got = run_tree(tree, P)
        ref = np.asarray(run_tree(tree, X), dtype=float)
        assert isinstance(got, DVec), [c[0] for c in tree[1]]
        if ctx.calls:
            eager += 1
            assert set(ctx.calls) <= {"nh_ew_binary", "nh_pack_rows"}
            if tree[2] is None:  # (without a second value, only a transform of a transform ...)
                assert sum(c[0] not in ("mul", "rmul", "div", "neg", "np.multiply")
                           for c in tree[1]) >= 2, [c[0] for c in tree[1]]
        else:
            folded += 1
            assert tree[2] is None
            assert got.ptr == P[tree[0]].ptr  # (still on its coordinate)
        val = value(ctx, got)
        close(val, ref, depth)
        worst = max(worst, float(np.max(np.abs(val - ref) / np.abs(ref))) / ((2 + depth) * EPS))
    print("\nrandom trees: %d folded, %d through a kernel; worst error / bound %.2f"
          % (folded, eager, worst))
    assert folded + eager == 300 and folded >= 150, (folded, eager)
    assert eager >= 30, eager  # (the eager path is exercised too)


# -------------------------------------------------------------------- DMat operand dispatch
@pytest.mark.parametrize("nE", [3, 7], ids=["N!=nE", "N==nE"])
def test_dmat_operand_dispatch(dev, nE):
    """a device vector is a per-WALKER factor of a device matrix, whichever side it stands on and
    whether it multiplies or divides -- also when N == nE, where a per-energy reading would go
    through unnoticed; a host vector of nE numbers is a per-energy factor; one of N != nE numbers
    is refused"""
    ctx, P = dev
    N = X.shape[1]
    M = np.random.default_rng(3).uniform(1.0, 2.0, (N, nE))
    m = DMat.from_buffer(ctx, ctx.array(M), N, nE)
    v, vh = 10 ** P[0], 10 ** X[0]
    for got, ref in ((m / v, M / vh[:, None]), (v * m, M * vh[:, None]), (m * v, M * vh[:, None]),
                     (m / P[2], M / X[2][:, None]), (np.sqrt(P[0]) * (m * 2.0), 2 * M * np.sqrt(X[0])[:, None])):
        assert isinstance(got, DMat) and got.shape == (N, nE)
        np.testing.assert_allclose(dmat_value(ctx, got), ref, rtol=4 * EPS)
    # (1 / 10**x is one elementwise kernel; 1 / x folds: the row factors stay on the device)
    assert ctx.calls.count("nh_lincomb") == 5 and ctx.calls.count("nh_ew_binary") == 1, ctx.calls
    with pytest.raises(TypeError):
        v / m
    ctx.calls.clear()
    ce = np.linspace(1.0, 2.0, nE)
    for got, ref in ((m * ce, M * ce), (ce * m, M * ce), (m / ce, M / ce)):
        assert isinstance(got, DMat) and not ctx.calls
        np.testing.assert_allclose(dmat_value(ctx, got), ref, rtol=4 * EPS)
    if nE != N:
        with pytest.raises(ValueError):
            m * np.ones(N)
        with pytest.raises(ValueError):
            m / np.ones(N)
