"""Device-resident values for the step loop.

When the sampler keeps the ensemble in HBM it hands the model function a ``DPars``
whose ``pars[i]`` are ``DVec`` -- lazy per-walker scalars
``a * tf(b * base[w*stride] + c)`` living on the device.  The arithmetic a naima
model function does on its parameters (``10 ** pars[0] / u.eV``, ``pars[3] * u.uG``)
folds into those five numbers without launching anything; the kernel that finally
consumes the value (``nh_pack_rows``, ``nh_priors``) evaluates it.  Anything the lazy
form cannot express falls back to an eager elementwise kernel.  ``DMat`` is the
matching (N, n_E) object: a lazy linear combination of spectra that the fused
likelihood kernel (``nh_lnprob``) consumes directly, so ``IC.flux(...) +
SYN.flux(...)`` never becomes a kernel or a host array.

``np.asarray(x)`` / ``x.get()`` bring a value to the host (and synchronise).
"""
import ctypes as C

import numpy as np

from . import _lib

TF_ID, TF_POW10, TF_EXP, TF_LOG, TF_LOG10, TF_SQRT, TF_SQUARE, TF_RECIP = range(8)
OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "pow": 4, "max": 5, "min": 6, "lt": 7, "le": 8,
       "gt": 9, "ge": 10}


class nh_lazy(C.Structure):
    _fields_ = [("base", C.c_void_p), ("stride", C.c_longlong), ("a", C.c_double),
                ("b", C.c_double), ("c", C.c_double), ("tf", C.c_int), ("pad", C.c_int)]


class nh_comp(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_longlong), ("scale", C.c_double)]


class nh_pair_field(C.Structure):
    """include/naima_hip.h: one photon field of nh_pairabs_apply"""
    _fields_ = [("kappa", C.c_void_p), ("ld", C.c_longlong), ("L_cm", nh_lazy), ("dens", nh_lazy),
                ("T_K", nh_lazy), ("thermal", C.c_int), ("pad", C.c_int)]


class nh_grid(C.Structure):
    _fields_ = [("e_eV", C.c_void_p), ("xg", C.c_void_p), ("w", C.c_void_p), ("dlw", C.c_void_p),
                ("unit_scale", C.c_double), ("nG", C.c_int), ("pad", C.c_int),
                ("ln_e", C.c_void_p), ("lx", C.c_void_p)]


class nh_pack(C.Structure):
    _fields_ = [("cols", nh_lazy * 8), ("ncols", C.c_int), ("ld", C.c_int), ("out", C.c_void_p)]


class nh_moment(C.Structure):
    _fields_ = [("grid", C.c_int), ("pad", C.c_int), ("Kt", C.c_void_p), ("dlnKt", C.c_void_p),
                ("out", C.c_void_p)]


class nh_accept(C.Structure):
    _fields_ = [("coords", C.c_void_p), ("logp", C.c_void_p), ("blk", C.c_void_p),
                ("cursor", C.c_void_p), ("ns", C.c_int), ("ndim", C.c_int), ("lo", C.c_int),
                ("pad", C.c_int), ("accepted", C.c_void_p), ("naccepted", C.c_void_p),
                ("sel", C.c_void_p)]


class nh_prior(C.Structure):
    _fields_ = [("x", nh_lazy), ("p0", C.c_double), ("p1", C.c_double), ("kind", C.c_int),
                ("pad", C.c_int)]


class nh_hs_table(C.Structure):
    _fields_ = [("grid", C.c_int), ("nK", C.c_int), ("ldo", C.c_int), ("nonnegative", C.c_int),
                ("KD", C.c_void_p), ("reserved", C.c_void_p), ("scale", C.c_void_p),
                ("out", C.c_void_p)]


class nh_hs_syn(C.Structure):
    _fields_ = [("grid", C.c_int), ("nE", C.c_int), ("ldo", C.c_int), ("bcol", C.c_int),
                ("ldB", C.c_int), ("n1", C.c_int), ("E_eV", C.c_void_p), ("B", C.c_void_p),
                ("out", C.c_void_p), ("out2", C.c_void_p), ("ldo2", C.c_int), ("pad2", C.c_int)]


class nh_hs_blob(C.Structure):
    _fields_ = [("kind", C.c_int), ("mom", C.c_int), ("m", C.c_int), ("pad", C.c_int),
                ("lazy", nh_lazy), ("cur", C.c_void_p), ("hist", C.c_void_p)]


class nh_hs_desc(C.Structure):
    """include/naima_hip.h: the descriptor of nh_half_step_create"""
    _fields_ = [("coords", C.c_void_p), ("logp", C.c_void_p), ("blk", C.c_void_p),
                ("cursor", C.c_void_p), ("reserved", C.c_void_p),
                ("ns", C.c_int), ("ndim", C.c_int), ("lo", C.c_int), ("nloc", C.c_int),
                ("qT", C.c_void_p), ("factors", C.c_void_p), ("hist", C.c_void_p),
                ("accepted", C.c_void_p), ("naccepted", C.c_void_p), ("sel", C.c_void_p),
                ("do_accept", C.c_int), ("write_weights", C.c_int),
                ("packs", nh_pack * 4), ("npacks", C.c_int),
                ("kind", C.c_int), ("params", C.c_void_p),
                ("grids", nh_grid * 4), ("ngrids", C.c_int),
                ("moms", nh_moment * 4), ("nmoms", C.c_int),
                ("tab", nh_hs_table * 4), ("ntab", C.c_int),
                ("syn", nh_hs_syn),
                ("comps", nh_comp * 8), ("ncomp", C.c_int), ("nE", C.c_int),
                ("conv", C.c_void_p), ("flux", C.c_void_p), ("err_lo", C.c_void_p),
                ("err_hi", C.c_void_p), ("ul", C.c_void_p), ("cl", C.c_void_p),
                ("lp", C.c_void_p),
                ("terms", nh_prior * 16), ("nterms", C.c_int),
                ("model_out", C.c_void_p), ("total", C.c_void_p),
                ("blobs", nh_hs_blob * 4), ("nblobs", C.c_int), ("send_width", C.c_int)]


# __array_priority__ of every device-resident class (above Quantity's and Unit's, so that
# ndarray, Quantity and Unit operators defer to them); is_device() is the one test for it
DEVICE_PRIORITY = 30000


def is_device(x):
    """True for a device-resident lazy value (DVec, DMat, DFactor, LazyPrior) and for the
    parameter block they come from (DPars)"""
    return getattr(x, "__array_priority__", 0) == DEVICE_PRIORITY or isinstance(x, DPars)


def lazy_const(v):
    return nh_lazy(None, 0, float(v), 0.0, 0.0, TF_ID, 0)


def as_lazy(v):
    """the kernel argument of a number or a DVec"""
    return v.lazy() if isinstance(v, DVec) else lazy_const(v)


def _defer(x):
    """operands that own the operation: units and quantities (their reflected methods
    wrap the device value), so DVec/DMat return NotImplemented for them"""
    return type(x).__name__ in ("Unit", "Quantity")


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) or (
        isinstance(x, np.ndarray) and x.ndim == 0)


class DVec:
    """lazy per-walker scalar on the device (see module docstring)"""
    __array_priority__ = DEVICE_PRIORITY
    ndim = 1

    def __init__(self, ctx, owner, ptr, n, stride=1, a=1.0, b=1.0, c=0.0, tf=TF_ID):
        self.ctx, self.owner, self.ptr, self.n, self.stride = ctx, owner, ptr, int(n), int(stride)
        self.a, self.b, self.c, self.tf = float(a), float(b), float(c), tf

    # ---- array protocol ----------------------------------------------------
    @property
    def shape(self):
        return (self.n,)

    @property
    def size(self):
        return self.n

    def __len__(self):
        return self.n

    def _with(self, **kw):
        d = dict(a=self.a, b=self.b, c=self.c, tf=self.tf)
        d.update(kw)
        return DVec(self.ctx, self.owner, self.ptr, self.n, self.stride, **d)

    def lazy(self):
        return nh_lazy(self.ptr, self.stride, self.a, self.b, self.c, self.tf, 0)

    def is_plain(self):
        return self.tf == TF_ID and self.a == 1.0 and self.b == 1.0 and self.c == 0.0 \
            and self.stride == 1

    def dense(self):
        """a contiguous device vector holding the values (one tiny launch unless plain)"""
        if self.is_plain():
            return self
        out = self.ctx.empty((self.n,))
        cols = (nh_lazy * 1)(self.lazy())
        self.ctx.call("nh_pack_rows", cols, 1, self.n, out, 1)
        return DVec(self.ctx, out, out.ptr, self.n)

    def get(self):
        d = self.dense()
        host = np.empty(self.n)
        _lib._chk(_lib._lib.nh_download(self.ctx.h, host.ctypes.data, d.ptr, host.nbytes))
        return host

    def __array__(self, dtype=None, copy=None):
        return self.get()

    # ---- lazy arithmetic -----------------------------------------------------
    def _scale(self, k):
        return self._with(a=self.a * k)

    def _shift(self, k):
        if k == 0:
            return self
        if self.tf == TF_ID:  # a*(b x + c) + k
            return self._with(a=1.0, b=self.a * self.b, c=self.a * self.c + k)
        return self._binary("add", k)

    def _apply(self, tf):
        """tf(value) for a value that is still affine in x"""
        if self.tf == TF_ID:
            return self._with(a=1.0, b=self.a * self.b, c=self.a * self.c, tf=tf)
        d = self.dense()
        return d._with(tf=tf)

    def _binary(self, op, other, reverse=False):
        x = self.lazy()
        if isinstance(other, DVec):
            y = other.lazy()
            keep = (self.owner, other.owner)
        elif _is_number(other):
            y = lazy_const(other)
            keep = (self.owner,)
        else:
            o = np.asarray(other, dtype=float)
            if o.shape != (self.n,):
                raise ValueError("cannot combine a device vector of %d walkers with shape %r"
                                 % (self.n, o.shape))
            dev = self.ctx.array(o)
            y = nh_lazy(dev.ptr, 1, 1.0, 1.0, 0.0, TF_ID, 0)
            keep = (self.owner, dev)
        if reverse:
            x, y = y, x
        out = self.ctx.empty((self.n,))
        self.ctx.call("nh_ew_binary", OPS[op], C.byref(x), C.byref(y), self.n, out)
        del keep
        return DVec(self.ctx, out, out.ptr, self.n)

    def __mul__(self, o):
        if _defer(o) or isinstance(o, (DMat, DFactor)):  # (a matrix takes the per-walker factor)
            return NotImplemented
        return self._scale(float(o)) if _is_number(o) else self._binary("mul", o)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if _defer(o) or isinstance(o, (DMat, DFactor)):
            return NotImplemented
        return self._scale(1.0 / float(o)) if _is_number(o) else self._binary("div", o)

    def __rtruediv__(self, o):
        if _defer(o):
            return NotImplemented
        if _is_number(o) and self.tf == TF_ID and self.a != 0.0:
            return self._with(a=float(o) / self.a, tf=TF_RECIP)
        return self._binary("div", o, reverse=True)

    def __add__(self, o):
        if _defer(o) or isinstance(o, LazyPrior):
            return NotImplemented
        return self._shift(float(o)) if _is_number(o) else self._binary("add", o)

    __radd__ = __add__

    def __sub__(self, o):
        if _defer(o):
            return NotImplemented
        return self._shift(-float(o)) if _is_number(o) else self._binary("sub", o)

    def __rsub__(self, o):
        return (-self).__add__(o)

    def __neg__(self):
        return self._scale(-1.0)

    def __pow__(self, p):
        if _is_number(p):
            if p == 1:
                return self
            if p == 2 and self.tf == TF_ID:
                return self._with(a=self.a * self.a, tf=TF_SQUARE)
            if p == 0.5 and self.tf == TF_ID and self.a >= 0:
                return self._with(a=np.sqrt(self.a), tf=TF_SQRT)
            if p == -1:
                return self.__rtruediv__(1.0)
        return self._binary("pow", p)

    def __rpow__(self, base):
        if _is_number(base) and base > 0:
            if base == 10:
                return self._apply(TF_POW10)
            return (self * float(np.log(base)))._apply(TF_EXP)
        return self._binary("pow", base, reverse=True)

    def __lt__(self, o):
        return self._binary("lt", o)

    def __le__(self, o):
        return self._binary("le", o)

    def __gt__(self, o):
        return self._binary("gt", o)

    def __ge__(self, o):
        return self._binary("ge", o)

    __hash__ = None

    _UFUNCS = {"exp": TF_EXP, "log": TF_LOG, "log10": TF_LOG10, "sqrt": TF_SQRT,
               "square": TF_SQUARE, "reciprocal": TF_RECIP}
    _BIN = {"add": ("__add__", "__radd__"), "subtract": ("__sub__", "__rsub__"),
            "multiply": ("__mul__", "__rmul__"), "true_divide": ("__truediv__", "__rtruediv__"),
            "divide": ("__truediv__", "__rtruediv__"), "power": ("__pow__", "__rpow__"),
            "less": ("__lt__", "__gt__"), "less_equal": ("__le__", "__ge__"),
            "greater": ("__gt__", "__lt__"), "greater_equal": ("__ge__", "__le__")}

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        """np.log10(pars[0]), ndarray * pars[1] ... stay on the device"""
        if method != "__call__" or kwargs:
            return NotImplemented
        name = ufunc.__name__
        if name in self._UFUNCS and len(inputs) == 1:
            return self._apply(self._UFUNCS[name])
        if name == "negative":
            return -self
        if name in self._BIN and len(inputs) == 2:
            fwd, rev = self._BIN[name]
            if inputs[0] is self:
                return getattr(self, fwd)(inputs[1])
            return getattr(self, rev)(inputs[0])
        return NotImplemented


class DPars:
    """the parameter block a device-resident sampler passes to the model function:
    qT[ndim][n] in HBM; ``pars[i]`` is the DVec of parameter i over the n walkers"""

    def __init__(self, ctx, buf, ndim, n):
        self.ctx, self.buf, self.ndim, self.n = ctx, buf, int(ndim), int(n)

    def __len__(self):
        return self.ndim

    @property
    def shape(self):
        return (self.ndim, self.n)

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            if i < 0:
                i += self.ndim
            if not 0 <= i < self.ndim:
                raise IndexError(i)
            return DVec(self.ctx, self.buf, self.buf.ptr + 8 * i * self.n, self.n)
        raise TypeError("a device parameter block is indexed by parameter number")

    def __iter__(self):
        return (self[i] for i in range(self.ndim))

    def get(self):
        return self.buf.get().reshape(self.ndim, self.n)

    def __array__(self, dtype=None, copy=None):
        return self.get()


class DMat:
    """lazy (N, m) device matrix: colfac[k] * sum_j scale_j * buf_j[w*ld_j + k]"""
    __array_priority__ = DEVICE_PRIORITY
    __array_ufunc__ = None
    ndim = 2

    def __init__(self, ctx, terms, shape, colfac=None):
        self.ctx, self.terms, self.shape, self.colfac = ctx, list(terms), tuple(shape), colfac

    @classmethod
    def from_buffer(cls, ctx, buf, N, m, ld=None, col0=0, scale=1.0):
        return cls(ctx, [(buf, buf.ptr + 8 * col0, ld if ld is not None else m, float(scale))],
                   (N, m))

    @property
    def size(self):
        return self.shape[0] * self.shape[1]

    def __len__(self):
        return self.shape[0]

    def _scaled(self, k):
        return DMat(self.ctx, [(b, p, ld, s * k) for b, p, ld, s in self.terms], self.shape,
                    self.colfac)

    def __mul__(self, o):
        if _defer(o):
            return NotImplemented
        if _is_number(o):
            return self._scaled(float(o))
        o = lift_factor(o, self.shape[0])  # (an absorption with nothing free: N equal rows)
        if isinstance(o, DFactor):  # per-walker, per-energy factor (absorption at a free z, L ...)
            return o.apply(self)
        if isinstance(o, DVec):  # per-walker factor (a target density that is a fit parameter)
            if o.n != self.shape[0]:
                raise ValueError("factor has %d walkers, matrix has %d" % (o.n, self.shape[0]))
            return self._rows_scaled(o)
        o = np.asarray(o, dtype=float)
        if o.shape == (self.shape[1],):  # per-energy factor (e.g. E**2 of sed())
            cf = o if self.colfac is None else self.colfac * o
            return DMat(self.ctx, self.terms, self.shape, cf)
        raise ValueError("unsupported operand shape %r for a device matrix" % (o.shape,))

    __rmul__ = __mul__

    def __truediv__(self, o):
        if _defer(o):
            return NotImplemented
        if _is_number(o):
            return self._scaled(1.0 / float(o))
        if isinstance(o, DVec):  # per-walker divisor: the reciprocal stays lazy, a row factor
            return self.__mul__(1.0 / o)
        if isinstance(o, (DMat, DFactor)):
            return NotImplemented
        return self.__mul__(1.0 / np.asarray(o, dtype=float))

    def __neg__(self):
        return self._scaled(-1.0)

    def __add__(self, o):
        if isinstance(o, DMat):
            if o.shape != self.shape:
                raise ValueError("shape mismatch %r vs %r" % (self.shape, o.shape))
            same_cf = (self.colfac is None and o.colfac is None) or (
                self.colfac is not None and o.colfac is not None
                and np.array_equal(self.colfac, o.colfac))
            if same_cf and len(self.terms) + len(o.terms) <= 8:
                return DMat(self.ctx, self.terms + o.terms, self.shape, self.colfac)
            a, b = self.dense(), o.dense()
            return DMat(self.ctx, a.terms + b.terms, self.shape)
        if _is_number(o) and o == 0:
            return self
        raise TypeError("cannot add %r to a device matrix" % type(o).__name__)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-o)

    def comps(self):
        arr = (nh_comp * len(self.terms))()
        for j, (_, p, ld, s) in enumerate(self.terms):
            arr[j] = nh_comp(p, ld, s)
        return arr

    def _rows_scaled(self, rf):
        import ctypes as C
        self.ctx.flush(*[t[0] for t in self.terms])
        N, m = self.shape
        out = self.ctx.empty((N, m))
        cf = self.ctx.const(self.colfac) if self.colfac is not None else None
        lz = rf.lazy()
        self.ctx.call("nh_lincomb", self.comps(), len(self.terms), cf, C.addressof(lz), N, m, out,
                      m)
        return DMat.from_buffer(self.ctx, out, N, m)

    def dense(self):
        """one contiguous [N][m] buffer (nh_lincomb) unless already so"""
        self.ctx.flush(*[t[0] for t in self.terms])
        N, m = self.shape
        if len(self.terms) == 1 and self.colfac is None and self.terms[0][3] == 1.0 \
                and self.terms[0][2] == m:
            return self
        out = self.ctx.empty((N, m))
        cf = self.ctx.const(self.colfac) if self.colfac is not None else None
        self.ctx.call("nh_lincomb", self.comps(), len(self.terms), cf, None, N, m, out, m)
        return DMat.from_buffer(self.ctx, out, N, m)

    def buffer(self):
        d = self.dense()
        return d.terms[0][0], d.terms[0][1]

    def get(self):
        d = self.dense()
        host = np.empty(self.shape)
        _lib._chk(_lib._lib.nh_download(self.ctx.h, host.ctypes.data, d.terms[0][1], host.nbytes))
        return host

    def __array__(self, dtype=None, copy=None):
        return self.get()

    def __getitem__(self, k):
        return self.get()[k]


class FactorRow(np.ndarray):
    """the (n_e,) factor of an absorption model whose values are all scalars: a host array that
    remembers its device form.  ``device(N)`` is the ``DFactor`` of N equal rows, which a ``DMat``
    multiplies with and the device loop keeps as a blob, so that a model function with nothing
    free in its absorber stays on the device.  Arrays derived from it are plain numbers."""
    _make = None

    def __new__(cls, values, make):
        a = np.asarray(values, dtype=float).view(cls)
        a._make = make
        return a

    def __array_finalize__(self, obj):
        self._make = None

    def device(self, N):
        return self._make(int(N)) if self._make is not None else None


def lift_factor(b, n):
    """a ``FactorRow`` as its device factor over n walkers; anything else as it is"""
    if isinstance(b, FactorRow) and b._make is not None:
        return b.device(n)
    return b


class DFactor:
    """a lazy (N, nE) per-walker, per-energy factor of a device flux (an absorption): a subclass
    gives ``apply(m)`` -- the ``DMat`` of factor * m, or of the factor itself without m, in one
    launch that also forms m's linear combination -- and ``shape``"""
    __array_priority__ = DEVICE_PRIORITY
    __array_ufunc__ = None
    ndim = 2

    @property
    def size(self):
        return self.shape[0] * self.shape[1]

    def __len__(self):
        return self.shape[0]

    def _terms_of(self, m):
        """(comps, ncomp, colfac) of the matrix to multiply; its held-back launches flushed"""
        if m is None:
            return None, 0, None
        if m.shape != self.shape:
            raise ValueError("%s factor of shape %r times a device matrix of shape %r"
                             % (self._what, self.shape, m.shape))
        self.ctx.flush(*[t[0] for t in m.terms])
        cf = self.ctx.const(m.colfac) if m.colfac is not None else None
        return m.comps(), len(m.terms), cf

    def __mul__(self, o):
        if _defer(o):
            return NotImplemented
        if isinstance(o, DMat):
            return self.apply(o)
        return self.apply() * o  # numbers, per-energy factors, per-walker DVec

    __rmul__ = __mul__

    def get(self):
        return self.apply().get()

    def __array__(self, dtype=None, copy=None):
        return self.get()

    def __getitem__(self, k):
        return self.get()[k]


class DEbl(DFactor):
    """lazy (N, nE) EBL factor: row row(z_w) of a walker-independent table Tab[400][nE]
    (nh_ebl_table, cached per set of energies) for a lazy per-walker redshift z.  Times a
    ``DMat`` it is one ``nh_ebl_apply`` launch that also forms the matrix's linear combination;
    ``.get()`` gathers the rows themselves."""
    _what = "EBL"

    def __init__(self, ctx, tab, zl, z, nE):
        self.ctx, self.tab, self.zl, self.z = ctx, tab, zl, z
        self.shape = (z.n, int(nE))

    def apply(self, m=None):
        """DMat of Tab[row(z_w)][k] * (m[w][k], or 1 without m): one nh_ebl_apply launch"""
        N, nE = self.shape
        comps, ncomp, cf = self._terms_of(m)
        out = self.ctx.empty((N, nE))
        lz = self.z.lazy()
        self.ctx.call("nh_ebl_apply", self.tab, nE, self.zl.shape[0] + 1, self.zl,
                      self.zl.shape[0], C.byref(lz), comps, ncomp, cf, N, nE, out, nE)
        return DMat.from_buffer(self.ctx, out, N, nE)


class DPairAbs(DFactor):
    """lazy (N, nE) pair-production transmission exp(-tau) (or, with ``tau``, the opacity
    itself): tau_w[k] = sum_f L_f(w) a_f(w) kappa_f[row_f(w)][k] over at most 8 photon fields.
    ``fields`` is a list of (kappa, per_walker, L_cm, dens, T_K or None): kappa the DeviceArray
    of nh_pairabs_rows -- one shared row, or with ``per_walker`` one row per walker --, the
    others a number or a ``DVec``.  Times a ``DMat`` it is one ``nh_pairabs_apply`` launch that
    also forms the matrix's linear combination."""
    _what = "pair-absorption"

    def __init__(self, ctx, fields, N, nE, tau=False):
        if len(fields) > 8:
            raise ValueError("at most 8 photon fields in one absorption factor, got %d"
                             % len(fields))
        self.ctx, self.fields, self.tau = ctx, list(fields), bool(tau)
        self.shape = (int(N), int(nE))

    def apply(self, m=None):
        N, nE = self.shape
        if self.tau and m is not None:
            raise TypeError("an opacity is not a factor of a flux: multiply with the transmission")
        comps, ncomp, cf = self._terms_of(m)
        arr = (nh_pair_field * max(len(self.fields), 1))()
        for j, (kappa, per_walker, L, dens, T) in enumerate(self.fields):
            arr[j] = nh_pair_field(kappa.ptr, nE if per_walker else 0, as_lazy(L),
                                   as_lazy(dens), as_lazy(T if T is not None else 0.0),
                                   int(T is not None), 0)
        out = self.ctx.empty((N, nE))
        self.ctx.call("nh_pairabs_apply", arr, len(self.fields), comps, ncomp, cf,
                      int(self.tau), N, nE, out, nE)
        return DMat.from_buffer(self.ctx, out, N, nE)


class DSsa(DFactor):
    """lazy (N, nE) synchrotron self-absorption escape fraction f(tau) of a homogeneous source
    (or, with ``tau``, the optical depth itself): ``kappa`` is the DeviceArray of
    nh_syn_absorption -- one shared row, or with ``per_walker`` one row per walker --, ``R_cm``
    a number or a ``DVec`` and ``geometry`` 'sphere' or 'slab'.  Times a ``DMat`` it is one
    ``nh_ssa_apply`` launch that also forms the matrix's linear combination."""
    _what = "self-absorption"

    def __init__(self, ctx, kappa, per_walker, R_cm, geometry, N, nE, tau=False):
        if geometry not in _lib.NH_SSA_GEOMETRY:
            raise ValueError("geometry should be one of: %s" % sorted(_lib.NH_SSA_GEOMETRY))
        self.ctx, self.kappa, self.per_walker, self.R_cm = ctx, kappa, bool(per_walker), R_cm
        self.geometry, self.tau = geometry, bool(tau)
        self.shape = (int(N), int(nE))

    def apply(self, m=None):
        N, nE = self.shape
        if self.tau and m is not None:
            raise TypeError("an optical depth is not a factor of a flux: multiply with the "
                            "transmission")
        comps, ncomp, cf = self._terms_of(m)
        lz = as_lazy(self.R_cm)
        out = self.ctx.empty((N, nE))
        self.ctx.call("nh_ssa_apply", self.kappa, nE if self.per_walker else 0, C.byref(lz),
                      _lib.NH_SSA_GEOMETRY[self.geometry], comps, ncomp, cf, int(self.tau), N, nE,
                      out, nE)
        return DMat.from_buffer(self.ctx, out, N, nE)


class LazyPrior:
    """sum of prior terms on device scalars, evaluated by nh_priors"""
    __array_priority__ = DEVICE_PRIORITY
    __array_ufunc__ = None

    def __init__(self, ctx, n, terms=(), const=0.0):
        self.ctx, self.n, self.terms, self.const = ctx, n, list(terms), float(const)

    def __add__(self, o):
        if isinstance(o, LazyPrior):
            return LazyPrior(self.ctx, self.n, self.terms + o.terms, self.const + o.const)
        if isinstance(o, DVec):
            return LazyPrior(self.ctx, self.n, self.terms + [(3, o, 0.0, 0.0)], self.const)
        if _is_number(o):
            return LazyPrior(self.ctx, self.n, self.terms, self.const + float(o))
        return NotImplemented

    __radd__ = __add__

    def packed(self):
        """(ctypes nh_prior array, n) when the sum fits one kernel argument block,
        else (None, 0)"""
        terms = list(self.terms)
        if self.const != 0.0:
            terms.append((3, None, self.const, 0.0))
        if len(terms) > 16:
            return None, 0
        if not terms:
            return None, 0
        arr = (nh_prior * len(terms))()
        for j, (kind, x, p0, p1) in enumerate(terms):
            lz = x.lazy() if x is not None else lazy_const(p0)
            arr[j] = nh_prior(lz, float(p0), float(p1), int(kind), 0)
        self._keep = arr
        return arr, len(terms)

    def evaluate(self):
        """dense device vector lp[n]"""
        terms = list(self.terms)
        if self.const != 0.0 or not terms:
            terms.append((3, None, self.const, 0.0))
        out = self.ctx.empty((self.n,))
        for i in range(0, len(terms), 15):  # NH_MAX_PRIOR = 16; chain through a VALUE term
            chunk = terms[i:i + 15]
            if i > 0:
                chunk = [(3, DVec(self.ctx, out, out.ptr, self.n), 0.0, 0.0)] + chunk
                nxt = self.ctx.empty((self.n,))
            else:
                nxt = out
            arr = (nh_prior * len(chunk))()
            for j, (kind, x, p0, p1) in enumerate(chunk):
                lz = x.lazy() if x is not None else lazy_const(p0)
                arr[j] = nh_prior(lz, float(p0), float(p1), int(kind), 0)
            self.ctx.call("nh_priors", arr, len(chunk), self.n, nxt)
            out = nxt
        return DVec(self.ctx, out, out.ptr, self.n)
