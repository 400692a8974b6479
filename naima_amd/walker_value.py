"""The three forms a physical parameter may arrive in, answered in one place.

    SCALAR   one number for every walker (naima's API)
    HOST     a host array with the walkers on its leading axis (1-D, one value per walker)
    DEVICE   a device-resident value (``darray.DVec``, built from ``pars[i]`` on the device loop)

``classify`` says which form a value has and how many walkers it implies, ``merge`` brings the
walker counts of several values to one, and ``lazy`` turns a value into the ``nh_lazy`` argument
of a kernel plus the buffer to keep alive until the launch is issued.  Nothing here launches a
kernel; a host array costs the one upload its site always made.
"""
import numpy as np

from .darray import TF_ID, DVec, is_device, lazy_const, nh_lazy
from .units import Quantity

SCALAR, HOST, DEVICE = "scalar", "host", "device"

# The predicates below run some fifty times per model evaluation of a host-loop fit, mostly on
# plain numbers: those are answered by their type, before np.ndim would make an array of them.
_NUMBER = frozenset((float, int, np.float64))


def raw(x):
    return x.value if isinstance(x, Quantity) else x


def classify(x):
    """(form, walkers) of a Quantity or a bare value.  A host array of any rank is HOST with
    the walkers on its leading axis; sites that take one value per walker ask ``is_vector``."""
    v = x.value if isinstance(x, Quantity) else x
    if type(v) in _NUMBER:
        return SCALAR, 1
    if is_device(v):
        return DEVICE, v.shape[0]
    if np.ndim(v) > 0:
        return HOST, np.shape(v)[0]
    return SCALAR, 1


def per_walker(x):
    """True for a parameter given per walker: host array or device value"""
    v = x.value if isinstance(x, Quantity) else x
    return type(v) not in _NUMBER and (np.ndim(v) > 0 or is_device(v))


def is_vector(x):
    """True for exactly one value per walker: a 1-D host array or a ``DVec``"""
    return np.ndim(raw(x)) == 1


def on_device(values):
    for x in values:
        if is_device(x.value if isinstance(x, Quantity) else x):
            return True
    return False


def is_batched(values):
    for x in values:
        if per_walker(x):
            return True
    return False


def merge(counts, where=None, broadcast_one=True):
    """the common walker count of ``counts``, or ValueError.  A count of 1 goes with any other
    (the result is 1 when nothing is larger); with ``broadcast_one=False`` every count has to
    agree, None makes no claim and is also the answer when nothing does."""
    n = None
    for c in counts:
        if c is None or (broadcast_one and c == 1):
            continue
        if n is not None and c != n:
            raise ValueError("inconsistent walker-batch sizes%s: %d vs %d"
                             % (" in " + where if where else "", n, c))
        n = c
    return 1 if n is None and broadcast_one else n


def counts(values):
    """the walker count each of ``values`` implies, for ``merge``"""
    out = []
    for x in values:
        v = x.value if isinstance(x, Quantity) else x
        # (classify's count: a device value has a shape too)
        out.append(1 if type(v) in _NUMBER or np.ndim(v) == 0 else np.shape(v)[0])
    return out


def _convert(ctx, x, unit, fold):
    """the value of ``x`` as a float, a ``DVec``, or a host array that is still to be broadcast
    to the batch and uploaded: see ``resolve``"""
    if fold and not x.on_device:
        v = np.asarray(x.value, dtype=float)
        if v.ndim > 1 or (v.ndim == 1 and v.size == 0):
            raise TypeError("a per-walker value must be a non-empty 1-D array, got shape %r"
                            % (v.shape,))
        if v.size == 1:  # (a scalar, or a batch of one walker)
            return float(np.ravel(x.to(unit).value)[0])
        d = ctx.array(v)
        x = Quantity(DVec(ctx, d, d.ptr, v.shape[0]), x.unit)
    v = x.to(unit).value if unit is not None else x.value if isinstance(x, Quantity) else x
    if isinstance(v, DVec):
        return v
    return float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=float)


def _checked(v, N, mismatch):
    if mismatch is not None and v.n != N:
        raise ValueError(mismatch % (v.n, N))
    return v


def resolve(ctx, x, unit=None, N=None, fold=False, mismatch=None):
    """the value of ``x`` (in ``unit`` when that is given) as a float or a ``DVec``.

    A host array is, by default, converted on the host, broadcast to ``N`` and uploaded.  With
    ``fold`` it is uploaded as given and converted as a device value is, by a factor folded
    into the ``DVec``, so that a host batch and the same numbers on the device give the same
    bits; an array of one element is then a float and anything but a non-empty 1-D array a
    TypeError.  ``unit=None`` converts nothing: the value travels in its own unit.
    ``mismatch``: the ValueError text, with (walkers, N) to fill in, for a ``DVec`` whose length
    is not ``N``; without it the length is left to the kernel's caller."""
    v = _convert(ctx, x, unit, fold)
    if isinstance(v, DVec):
        return _checked(v, N, mismatch)
    if type(v) is float:
        return v
    d = ctx.array(np.broadcast_to(v, (N,)))
    return DVec(ctx, d, d.ptr, N)


def lazy(ctx, x, unit=None, N=None, fold=False, mismatch=None):
    """(``nh_lazy``, what to keep alive until the launch is issued) of ``x``, converted as
    ``resolve`` converts it"""
    v = _convert(ctx, x, unit, fold)
    if isinstance(v, DVec):
        return _checked(v, N, mismatch).lazy(), v
    if type(v) is float:
        return lazy_const(v), None
    d = ctx.array(np.broadcast_to(v, (N,)))
    return nh_lazy(d.ptr, 1, 1.0, 1.0, 0.0, TF_ID, 0), d
