"""The glue kernels that evaluate a lazy per-walker value, against a high-precision reference.

``a * tf(b * x + c)`` with one of eight transforms is how every user model's parameter arithmetic
reaches the device (naima_amd/darray.py).  nh_pack_rows, nh_ew_binary, nh_priors and nh_lincomb's
row factor evaluate it through nh_lazy_apply / nh_prior_sum (nh_common.h); here they are called
through the C ABI on inputs no model in the repository produces:

  * all eight transforms x affine (a, b, c) with negative a and b, c = 0 and a c that nearly cancels
    b x (y = b x + c about 2**-20 of b x); strides 1 and NH_PD_NPAR; N = 1, 63, 64, 65, 257, 4097;
    1 and 8 columns with ld > ncols (the cells between, and the row behind the last, stay untouched);
  * ordinary values, +-0, denormals, +-inf, NaN, arguments outside a transform's domain, 10**x and
    exp(x) on both sides of overflow, of the first denormal and of the underflow to zero.

Reference.  Wherever NumPy's float64 evaluation of the same five numbers gives NaN, an infinity or
a zero, the kernel must give the same NaN-ness, the same signed infinity, the same signed zero.
Everywhere else the reference is mpmath (200 bits) on the float64 inputs, and the bound is derived
per point, not measured:

      |got - ref| <= (2 + cond) 2**-52 |ref| + (1 + |a|) 2**-1074

``cond`` the transform's condition number at y = b x + c (|y| ln 10 for POW10, |y| for EXP,
1 / |ln y| for LOG and LOG10, 1/2 for SQRT, 2 for SQUARE, 1 for RECIP and the identity): y carries
one rounding (two without an FMA -- then y is good to an ulp of b x, and the test says so for the
nearly cancelling c), the library function at most one ulp, ``a *`` half an ulp; the absolute term
is one spacing of the denormals for the function and the product's rounding.  ``nh_common.h``
says exp10 is within one ulp: this is where that is tested.

nh_ew_binary: + - * / max min and the four comparisons on exact operands (identity transform) are
IEEE operations and must equal NumPy bit for bit (NaN-ness for NaN); pow is held to mpmath at
2 ulp (2 * 2**-52: the library's documented one ulp, nothing propagated -- the operands are exact)
and to NumPy's special values (pow(x, 0) = 1 for NaN x, pow(-0, -1) = -inf, ...).  With transformed
operands the operands' own bounds are propagated through the product and the quotient.

nh_priors through LazyPrior.evaluate: the four kinds on identity and transformed values; 1, 15,
16, 17 and 31 terms (the chaining through a VALUE term: 1, 1, 2, 2, 3 launches) with and without a
constant; a constant-only prior; the edges v == p0, v == p1 (inclusive both), v NaN (uniform and
log-uniform -inf, normal NaN, as core.py on the host), log-uniform at v = 0 and with umax = inf.
The bound of a sum is the terms' bounds (each term re-evaluated by mpmath at v (1 +- its bound))
plus one rounding per addition on the sum of the terms' magnitudes.

Measured on an MI355X (error / bound, the largest over all points; pytest -s prints them;
profiles/NOTES_transforms.md): ID 0.245, POW10 0.410, EXP 0.419, LOG 0.348, LOG10 0.348, SQRT 0.364,
SQUARE 0.355, RECIP 0.364 -- exp10 at 10**307.9 (cond 709) and next to the denormals stays inside
its one ulp; pow on exact operands 0.362; products and quotients of transformed operands 0.347;
prior sums 0.074.  The kernel's b x + c is one FMA: the nearly cancelling c passes at the strict
bound.

Mutation checks (by hand, on a scratch copy of the library; the failure observed):
  * the LOG and SQRT labels of nh_lazy_apply swapped: 23 tests of this file fail (test_pack_rows:
    ('LOG', (1.0, 1.0, 0.0), 'x = 709.7', 'got 26.64019519448009', 'NumPy 6.564842345530938'),
    ('LOG', 'x = 0.0', 'got 0.0', 'NumPy -inf'); test_lincomb_row_factor,
    test_ew_binary_transformed_operands, test_priors_chained), and in test_gpu_transforms.py
    [square-sqrt-recip] and [mixed-wave-syn+tables]; test_gpu_parity.py's test_lazy_device_values
    and test_device_lnprob_equals_host_lnprob pass;
  * a prior term evaluated on the raw coordinate (nh_prior_sum): all of test_priors_chained at
    15 .. 31 terms fail ('got -inf', 'NumPy -15.137285184984158'); test_lazy_device_values, whose
    priors sit on plain coordinates, passes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TINY = 2.0 ** -1074
TF_NAMES = ["ID", "POW10", "EXP", "LOG", "LOG10", "SQRT", "SQUARE", "RECIP"]
NPAR = 8  # NH_PD_NPAR

# ------------------------------------------------------------------------------ the inputs
_rng = np.random.default_rng(77)
POOL = np.concatenate([
    [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.3e-308, np.inf, -np.inf, np.nan],
    [1.0, -1.0, 0.5, 2.0, 3.7, -3.7, 1e-5, -1e-5, 1e5, 1.37, 1.0000001, 0.9999999, 10.0, 100.0],
    [307.9, 308.2, 308.3, 309.0, -307.6, -308.5, -310.0, -323.3, -324.0, -400.0],  # 10**x edges
    [709.7, 709.8, 711.0, -708.0, -709.0, -740.0, -745.0, -746.0, -800.0],  # exp(x) edges
    [1e300, -1e300, 1e-300, 1e154, 1.4e154, 1e-154, 1e-162],  # square over / underflow, recip
    _rng.uniform(-3.0, 3.0, 30), 10.0 ** _rng.uniform(-8, 8, 20), -10.0 ** _rng.uniform(-8, 8, 6)])
X0 = 1.37  # (the value the nearly cancelling c is built around)
AFFINES = [(1.0, 1.0, 0.0), (-2.5, 1.0, 0.0), (1.0, -1.0, 0.0), (0.75, -3.0, 0.0),
           (1.0, 2.0, -30.0), (3.0, 0.5, 1.25), (-1e-3, 1.0, 300.0),
           (1.0, 3.0, -(3.0 * X0) * (1.0 - 2.0 ** -20))]


def lazy_np(a, b, c, tf, raw):
    """nh_lazy_apply in NumPy float64: decides which results are special"""
    with np.errstate(all="ignore"):
        y = b * np.asarray(raw, dtype=float) + c
        v = [lambda v: v, lambda v: np.power(10.0, v), np.exp, np.log, np.log10, np.sqrt,
             lambda v: v * v, lambda v: 1.0 / v][tf](y)
        return a * v


def _mp():
    import mpmath
    mp = mpmath.mp
    mp.prec = 200
    return mpmath, mp


def mp_value(a, b, c, tf, x):
    """(a tf(b x + c), cond at y) by mpmath on the float64 inputs; None where y is outside the
    transform's domain or the result is not a finite real number"""
    mpmath, mp = _mp()
    if not np.isfinite(x):
        return None
    y = mp.mpf(b) * mp.mpf(x) + mp.mpf(c)
    if tf in (3, 4):
        if y <= 0:
            return None
        v = mp.log(y) if tf == 3 else mp.log10(y)
        cond = 1 / abs(mp.log(y)) if y != 1 else mp.inf
    elif tf == 5:
        if y < 0:
            return None
        v, cond = mp.sqrt(y), mp.mpf(0.5)
    elif tf == 7:
        if y == 0:
            return None
        v, cond = 1 / y, mp.mpf(1)
    elif tf == 1:
        v, cond = mp.power(10, y), abs(y) * mp.log(10)
    elif tf == 2:
        v, cond = mp.exp(y), abs(y)
    elif tf == 6:
        v, cond = y * y, mp.mpf(2)
    else:
        v, cond = y, mp.mpf(1)
    return mp.mpf(a) * v, cond


@functools.lru_cache(maxsize=None)
def pool_reference(a, b, c, tf):
    """per POOL value: (NumPy float64 value, mp value or None: special, relative bound, absolute
    bound).  Special is what NumPy makes NaN or infinite, and a zero that is an exact zero; a zero
    by underflow (10 ** -324, (1e-162) ** 2) is an ordinary value held by the absolute bound."""
    ref_np = lazy_np(a, b, c, tf, POOL)
    out = []
    for x, r in zip(POOL, ref_np):
        ref = None if (np.isnan(r) or np.isinf(r)) else mp_value(a, b, c, tf, float(x))
        if ref is None or ref[0] == 0:
            out.append((r, None, 0.0, 0.0))
        else:
            out.append((r, ref[0], (2 + ref[1]) * EPS, (1 + abs(a)) * TINY))
    return out


def same_special(got, ref):
    """same NaN-ness, same signed infinity, same signed zero"""
    if np.isnan(ref):
        return bool(np.isnan(got))
    return bool(got == ref and np.signbit(got) == np.signbit(ref))


_VERIFIED = {}


def check_lazy(got, idx, a, b, c, tf, worst, where, skip=None):
    """got[i] is the kernel's value at POOL[idx[i]] (skip[j]: POOL[j] is not checked)"""
    mpmath, mp = _mp()
    refs = pool_reference(a, b, c, tf)
    done = _VERIFIED.setdefault((a, b, c, tf), set())
    got = np.ascontiguousarray(got, dtype=float)
    pairs = np.unique(np.stack([np.asarray(idx, dtype=np.int64), got.view(np.int64)]), axis=1)
    for i, bits in pairs.T.tolist():
        if (i, bits) in done or (skip is not None and skip[i]):
            continue
        g = float(np.int64(bits).view(np.float64))
        r, v, rt, at = refs[i]
        tag = (where, TF_NAMES[tf], (a, b, c), "x = %r" % POOL[i], "got %r" % g, "NumPy %r" % r)
        if v is None:
            assert same_special(g, r), tag
        else:
            assert np.isfinite(g), tag
            err, bound = abs(mp.mpf(g) - v), rt * abs(v) + at
            assert err <= bound, tag + ("error / bound %s" % mpmath.nstr(err / bound, 5),)
            worst[tf] = max(worst.get(tf, 0.0), float(err / bound))
        done.add((i, bits))


@pytest.fixture(scope="module")
def lib():
    import naima_amd  # noqa: F401
    from naima_amd import _lib, darray
    return _lib.get_context(), darray


def _columns(ctx, D, N, stride, ncols, rng):
    """ncols coordinates of N walkers drawn from POOL (every value when N allows), laid out
    [ncols][N] (stride 1) or [N][NH_PD_NPAR] (stride NH_PD_NPAR): (device buffer, idx[ncols][N],
    base address of column j)"""
    idx = np.stack([(np.arange(N) * (1 + 2 * j) + int(rng.integers(0, POOL.size))) % POOL.size
                    for j in range(ncols)])
    if stride == 1:
        dev = ctx.array(POOL[idx])
        return dev, idx, [dev.ptr + 8 * j * N for j in range(ncols)]
    host = np.full((N, stride), 12345.0)
    host[:, :ncols] = POOL[idx].T
    dev = ctx.array(host)
    return dev, idx, [dev.ptr + 8 * j for j in range(ncols)]


WORST = {}


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("stride", [1, NPAR], ids=["stride1", "strideNPAR"])
@pytest.mark.parametrize("ncols,ld", [(1, 1), (1, 3), (8, 8), (8, 11)])
def test_pack_rows(lib, N, stride, ncols, ld):
    """nh_pack_rows: every transform in every column position (column j takes transform
    (j + shift) % 8, shift = 0 .. 7), every affine set"""
    ctx, D = lib
    rng = np.random.default_rng(N * 100 + stride * 10 + ld)
    dev, idx, bases = _columns(ctx, D, N, stride, ncols, rng)
    for ai, (a, b, c) in enumerate(AFFINES):
        for shift in range(8):
            cols = (D.nh_lazy * ncols)()
            for j in range(ncols):
                cols[j] = D.nh_lazy(bases[j], stride, a, b, c, (j + shift) % 8, 0)
            out = ctx.array(np.full((N + 1, ld), 777.0))
            ctx.call("nh_pack_rows", cols, ncols, N, out, ld)
            got = out.get()
            assert np.all(got[N] == 777.0) and np.all(got[:N, ncols:] == 777.0)
            for j in range(ncols):
                check_lazy(got[:N, j], idx[j], a, b, c, (j + shift) % 8, WORST,
                           ("pack_rows", N, stride, ncols, ld, "column %d" % j))
    del dev


def test_pack_rows_constant_column(lib):
    """base == NULL: the constant a, whatever b, c and tf say"""
    ctx, D = lib
    cols = (D.nh_lazy * 2)(D.nh_lazy(None, 0, -2.75, 3.0, 4.0, D.TF_LOG, 0),
                           D.nh_lazy(None, 0, np.inf, 0.0, 0.0, D.TF_ID, 0))
    out = ctx.array(np.zeros((65, 2)))
    ctx.call("nh_pack_rows", cols, 2, 65, out, 2)
    got = out.get()
    assert np.all(got[:, 0] == -2.75) and np.all(got[:, 1] == np.inf)


def test_lincomb_row_factor(lib):
    """nh_lincomb with a lazy row factor: out[w][k] = rf[w] colfac[k] sum_j scale_j comp_j[w][k].
    The components are powers of two, so the row factor's own error is all there is"""
    ctx, D = lib
    N, m = 257, 5
    rng = np.random.default_rng(5)
    dev, idx, bases = _columns(ctx, D, N, 1, 1, rng)
    M = 2.0 ** rng.integers(-3, 4, (N, m)).astype(float)
    Md = ctx.array(M)
    comps = (D.nh_comp * 2)(D.nh_comp(Md.ptr, m, 0.5), D.nh_comp(Md.ptr, m, 1.5))  # sum: 2 M
    cf = ctx.array(np.array([1.0, 2.0, 0.25, -1.0, 4.0]))
    for tf in range(8):
        for (a, b, c) in AFFINES[:4]:
            lz = D.nh_lazy(bases[0], 1, a, b, c, tf, 0)
            out = ctx.array(np.full((N, m + 1), 777.0))
            ctx.call("nh_lincomb", comps, 2, cf, C.addressof(lz), N, m, out, m + 1)
            got = out.get()
            assert np.all(got[:, m] == 777.0)
            fac = 2.0 * M * cf.get()
            with np.errstate(all="ignore"):
                rf = np.abs(lazy_np(a, b, c, tf, POOL))
            # (an exact power-of-two factor: divide it out; NaN / inf / zero keep their kind and get
            # their sign back.  Row factors that the factor of up to 64 could push over a range
            # limit are left to test_pack_rows)
            skip = np.isfinite(rf) & (rf != 0.0) & ((rf < 1e-280) | (rf > 1e280))
            for k in range(m):
                check_lazy(got[:, k] / fac[:, k], idx[0], a, b, c, tf, {}, ("lincomb", k), skip)


# ------------------------------------------------------------------------------ nh_ew_binary
OPS_NP = dict(add=np.add, sub=np.subtract, mul=np.multiply, div=np.divide, pow=np.power,
              max=np.fmax, min=np.fmin, lt=np.less, le=np.less_equal, gt=np.greater,
              ge=np.greater_equal)
EW_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 2.0, 0.5, -8.0, 1.0 / 3.0, 3.0, -2.0, np.inf, -np.inf,
                      np.nan, 5e-324, 1e-310, 1e300, -1e300, 1e-300, 1.37, 7.25, 0.99, 1e5, -0.5,
                      308.0, 1024.0, -1074.0])


def _ew(ctx, D, op, x, y, n):
    out = ctx.array(np.full(n + 1, 777.0))
    ctx.call("nh_ew_binary", D.OPS[op], C.byref(x), C.byref(y), n, out)
    got = out.get()
    assert got[n] == 777.0
    return got[:n]


@pytest.mark.parametrize("op", sorted(OPS_NP))
def test_ew_binary_exact_operands(lib, op):
    """all eleven operations on every ordered pair of EW_VALUES (so both operand orders), then
    with a constant (base == NULL) as the first and as the second operand"""
    mpmath, mp = _mp()
    ctx, D = lib
    A, B = [g.reshape(-1) for g in np.meshgrid(EW_VALUES, EW_VALUES, indexing="ij")]
    n = A.size
    Ad, Bd = ctx.array(A), ctx.array(B)
    ident = lambda d: D.nh_lazy(d.ptr, 1, 1.0, 1.0, 0.0, D.TF_ID, 0)
    runs = [(_ew(ctx, D, op, ident(Ad), ident(Bd), n), A, B)]
    for k in (2.0, -0.5, np.inf, np.nan, 0.0):
        runs.append((_ew(ctx, D, op, D.lazy_const(k), ident(Bd), n), np.full(n, k), B))
        runs.append((_ew(ctx, D, op, ident(Ad), D.lazy_const(k), n), A, np.full(n, k)))
    worst = 0.0
    for k, (got, a, b) in enumerate(runs):
        # (an operand read from memory passes 1 * (1 * x + 0): -0 becomes +0; a constant does not)
        a = a if k >= 1 and k % 2 == 1 else a + 0.0
        b = b if k >= 1 and k % 2 == 0 else b + 0.0
        with np.errstate(all="ignore"):
            ref = OPS_NP[op](a, b).astype(float)
        for g, r, ai, bi in zip(got.tolist(), ref.tolist(), a.tolist(), b.tolist()):
            tag = (op, ai, bi, "got %r" % g, "NumPy %r" % r)
            if op in ("max", "min") and ai == 0.0 and bi == 0.0:
                assert g == 0.0, tag  # (which zero fmax(+0, -0) returns is left open by C)
            elif op != "pow" or np.isnan(r) or np.isinf(r) or r == 0.0 or not np.isfinite(ai) \
                    or not np.isfinite(bi):
                assert same_special(g, r) if (np.isnan(r) or r == 0.0 or np.isinf(r)) else g == r, tag
            else:
                v = mp.power(mp.mpf(ai), mp.mpf(bi))
                assert isinstance(v, mp.mpf), tag
                err, bound = abs(mp.mpf(g) - v), 2 * EPS * abs(v) + TINY
                assert err <= bound, tag + (mpmath.nstr(err / bound, 5),)
                worst = max(worst, float(err / bound))
    print("\new_binary %s: %d operand pairs; pow error / bound %.3f" % (op, n * len(runs), worst))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4097])
def test_ew_binary_transformed_operands(lib, N):
    """a product and a quotient of two transformed operands at strides 1 and NH_PD_NPAR: each
    operand's bound propagated (relative errors add), half an ulp for the operation"""
    mpmath, mp = _mp()
    ctx, D = lib
    rng = np.random.default_rng(N)
    xs = rng.uniform(0.3, 2.5, (N, NPAR))
    dev = ctx.array(xs)
    cases = [(D.TF_POW10, (2.0, 1.5, -1.0), D.TF_SQRT, (1.0, 4.0, 0.5)),
             (D.TF_EXP, (-1.0, -2.0, 0.25), D.TF_RECIP, (3.0, 1.0, 1.0)),
             (D.TF_LOG, (1.0, 1.0, 2.0), D.TF_SQUARE, (0.5, -1.0, 0.0)),
             (D.TF_LOG10, (2.0, 3.0, 3.0), D.TF_ID, (1.0, 2.0, -7.0))]
    worst = 0.0
    for tx, (ax, bx, cx), ty, (ay, by, cy) in cases:
        x = D.nh_lazy(dev.ptr + 8 * 2, NPAR, ax, bx, cx, tx, 0)
        y = D.nh_lazy(dev.ptr + 8 * 7, NPAR, ay, by, cy, ty, 0)
        for op in ("mul", "div"):
            for first, second, swap in ((x, y, False), (y, x, True)):
                got = _ew(ctx, D, op, first, second, N)
                for w in range(N):
                    vx, kx = mp_value(ax, bx, cx, tx, xs[w, 2])
                    vy, ky = mp_value(ay, by, cy, ty, xs[w, 7])
                    p, q = (vy, vx) if swap else (vx, vy)
                    v = p * q if op == "mul" else p / q
                    bound = (4 + kx + ky + 0.5) * EPS * abs(v)
                    err = abs(mp.mpf(float(got[w])) - v)
                    assert err <= bound, (op, swap, w, xs[w], mpmath.nstr(err / bound, 5))
                    worst = max(worst, float(err / bound))
    print("\new_binary on transformed operands, N = %d: error / bound %.3f" % (N, worst))


# ------------------------------------------------------------------------------ nh_priors
def _prior_term_mp(kind, v, p0, p1):
    """one term of core.py:34-58 at the mp value v (None: NaN)"""
    mpmath, mp = _mp()
    if kind == 0:
        return mp.mpf(0) if p0 <= v <= p1 else -mp.inf
    if kind == 1:
        return -mp.mpf(0.5) * (2 * mp.pi * mp.mpf(p1)) - (v - mp.mpf(p0)) ** 2 / (2 * mp.mpf(p1))
    if kind == 2:
        return 1 / v if (v > 0 and v >= p0 and v <= p1) else -mp.inf
    return v


def _prior_term_np(kind, v, p0, p1):
    with np.errstate(all="ignore"):
        if kind == 0:
            return np.where((p0 <= v) & (v <= p1), 0.0, -np.inf)
        if kind == 1:
            return -0.5 * (2 * np.pi * p1) - (v - p0) ** 2 / (2.0 * p1)
        if kind == 2:
            return np.where((v > 0) & (v >= p0) & (v <= p1), 1.0 / v, -np.inf)
        return v


def check_prior_sum(got, terms, xs, const, where):
    """terms: (kind, (a, b, c, tf, coordinate) or None for a constant p0, p0, p1); xs[coordinate][w]"""
    mpmath, mp = _mp()
    worst = 0.0
    n = got.size
    with np.errstate(all="ignore"):
        ref_np = np.zeros(n)
        for kind, lz, p0, p1 in terms:
            v = np.full(n, p0) if lz is None else lazy_np(lz[0], lz[1], lz[2], lz[3], xs[lz[4]])
            ref_np = ref_np + _prior_term_np(kind, v, p0, p1)
        ref_np = ref_np + const
    for w in range(n):
        tag = (where, w, "got %r" % got[w], "NumPy %r" % ref_np[w])
        if not np.isfinite(ref_np[w]):
            assert same_special(got[w], ref_np[w]), tag
            continue
        s, mag, slack = mp.mpf(const), abs(mp.mpf(const)), mp.mpf(0)
        for kind, lz, p0, p1 in terms:
            if lz is None:
                v, dv = mp.mpf(p0), mp.mpf(0)
            else:
                v, cond = mp_value(lz[0], lz[1], lz[2], lz[3], float(xs[lz[4]][w]))
                dv = (2 + cond) * EPS * abs(v)
            t = _prior_term_mp(kind, v, p0, p1)
            lo, hi = _prior_term_mp(kind, v - dv, p0, p1), _prior_term_mp(kind, v + dv, p0, p1)
            assert mp.isfinite(lo) and mp.isfinite(hi), tag  # (no value within its bound of an edge)
            # (the term's own arithmetic: four roundings on its largest intermediate)
            big = abs(t) + ((v - p0) ** 2 / (2 * p1) if kind == 1 else 0)
            slack += max(abs(lo - t), abs(hi - t)) + 4 * EPS * big
            s += t
            mag += abs(t)
        bound = slack + (len(terms) + 2) * EPS * mag + TINY
        err = abs(mp.mpf(float(got[w])) - s)
        assert err <= bound, tag + (mpmath.nstr(err / bound, 5),)
        worst = max(worst, float(err / bound))
    return worst


def _lazy_prior(ctx, D, n, terms, const, bases):
    lp = D.LazyPrior(ctx, n, [], const)
    for kind, lz, p0, p1 in terms:
        x = None if lz is None else D.DVec(ctx, None, bases[lz[4]], n, 1, lz[0], lz[1], lz[2], lz[3])
        lp.terms.append((kind, x, p0, p1))
    return lp


@pytest.mark.parametrize("nterms", [1, 15, 16, 17, 31])
@pytest.mark.parametrize("const", [0.0, 0.25])
@pytest.mark.parametrize("N", [1, 65, 4097])
def test_priors_chained(lib, nterms, const, N):
    """sums of 1 .. 31 terms of all four kinds on identity and transformed values through
    LazyPrior.evaluate (15 terms per launch, chained through a VALUE term)"""
    ctx, D = lib
    rng = np.random.default_rng(nterms * 7 + N)
    xs = rng.uniform(0.4, 2.2, (3, N))
    xs[1] *= -1.0
    dev = ctx.array(xs)
    bases = [dev.ptr + 8 * j * N for j in range(3)]
    menu = [(0, (1.0, 1.0, 0.0, 0, 0), 0.7, 1.9), (1, (1.0, 1.0, 0.0, 0, 1), -1.0, 0.5),
            (2, (1.0, 1.0, 0.0, 0, 2), 0.6, 2.0), (3, (2.0, 1.0, 0.0, 0, 1), 0.0, 0.0),
            (0, (1.0, 1.0, 0.0, 1, 0), 3.0, 100.0), (1, (1.0, 1.0, 0.0, 4, 2), 0.1, 0.3),
            (2, (1.0, 1.0, 0.0, 6, 1), 0.1, np.inf), (1, (1.0, -1.0, 0.5, 2, 1), 3.0, 2.0),
            (3, (0.5, 1.0, 0.0, 5, 0), 0.0, 0.0), (0, (1.0, 1.0, 0.0, 7, 1), -3.0, -0.3)]
    terms = [menu[(3 * t + nterms) % len(menu)] for t in range(nterms)]
    lp = _lazy_prior(ctx, D, N, terms, const, bases)
    calls = []
    orig = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        got = lp.evaluate().get()
    finally:
        del ctx.call
    total = nterms + (1 if const else 0)
    nl, left = 1, total - 15  # (15 terms, then 14 more per launch behind the chained VALUE term)
    while left > 0:
        nl, left = nl + 1, left - 15
    assert calls.count("nh_priors") == nl, (calls, total)
    worst = check_prior_sum(got, terms, xs, const, ("priors", nterms, const, N))
    assert np.isfinite(got).sum() > 0 or N == 1
    print("\npriors, %d terms + %r, N = %d: error / bound %.3f" % (nterms, const, N, worst))
    del dev


def test_prior_constant_only(lib):
    ctx, D = lib
    for const in (0.0, -1.5):
        got = D.LazyPrior(ctx, 65, [], const).evaluate().get()
        assert got.shape == (65,) and np.all(got == const)


def test_prior_edges(lib):
    """v == p0 and v == p1 are inside (uniform, log-uniform); NaN gives -inf / NaN / -inf;
    log-uniform at v = +-0 and below p0 is -inf, with umax = inf any v >= p0 counts; a normal
    prior at +-inf is -inf; the VALUE kind hands the value through"""
    ctx, D = lib
    v = np.array([0.5, 2.0, np.nextafter(0.5, 0), np.nextafter(2.0, 3), np.nan, 0.0, -0.0, np.inf,
                  -np.inf, 1.0, 5e-324, 1e300, -1.0])
    dev = ctx.array(v)
    n = v.size
    ident = (1.0, 1.0, 0.0, 0, 0)
    inf = np.inf
    for kind, p0, p1 in ((0, 0.5, 2.0), (2, 0.5, 2.0), (2, 0.0, inf), (2, 0.5, inf), (1, 1.0, 0.5),
                         (0, -inf, inf), (0, 0.0, 0.0), (3, 0.0, 0.0), (2, 0.0, 5e-324)):
        lp = _lazy_prior(ctx, D, n, [(kind, ident, p0, p1)], 0.0, [dev.ptr])
        got = lp.evaluate().get()
        with np.errstate(all="ignore"):
            ref = _prior_term_np(kind, v, p0, p1) + 0.0
        for g, r, vi in zip(got.tolist(), np.asarray(ref, dtype=float).tolist(), v.tolist()):
            tag = (kind, p0, p1, "v = %r" % vi, "got %r" % g, "NumPy %r" % r)
            if np.isnan(r) or np.isinf(r):
                assert same_special(g, r), tag
            else:
                assert abs(g - r) <= 4 * EPS * abs(r), tag
    # the host's own functions agree with the restatement used above
    from naima_amd import log_uniform_prior, normal_prior, uniform_prior
    with np.errstate(all="ignore"):
        assert np.array_equal(uniform_prior(v, 0.5, 2.0), _prior_term_np(0, v, 0.5, 2.0))
        assert np.array_equal(log_uniform_prior(v, 0.5), _prior_term_np(2, v, 0.5, inf))
        assert np.array_equal(normal_prior(v, 1.0, 0.5), _prior_term_np(1, v, 1.0, 0.5),
                              equal_nan=True)


def test_print_worst_ratios():
    """(last in the file: the largest error / bound per transform over test_pack_rows)"""
    assert set(WORST) == set(range(8)), WORST
    print("\nlazy transforms, largest error / bound: " +
          ", ".join("%s %.3f" % (TF_NAMES[t], WORST[t]) for t in sorted(WORST)))
    assert max(WORST.values()) <= 1.0
