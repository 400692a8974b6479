"""Convenience functions with naima.utils' names: ``trapz_loglog`` (utils.py:285-355 of the
reference) evaluated by the ``nh_trapz_loglog`` kernel -- or, for a device-resident spectrum,
by ``nh_trapz_loglog_comps`` without leaving HBM -- and ``sed_conversion``."""
import numpy as np

from . import units as u
from ._lib import get_context
from .darray import DFactor, DMat, DVec
from .core import sed_conversion  # noqa: F401  (re-export, utils.py:219-282)
from .datatable import (build_data_table, generate_energy_edges,  # noqa: F401
                        validate_data_table)

__all__ = ["trapz_loglog", "sed_conversion", "estimate_B", "build_data_table",
           "generate_energy_edges", "validate_data_table"]


def trapz_loglog(y, x, axis=-1, intervals=False):
    """Integrate ``y(x)`` along ``axis`` with the composite trapezoid rule in log-log
    space (exact for power laws).  Quantity-aware like the reference.

    A device-resident ``y`` (the ``(N, n_E)`` flux of a walker batch on device parameters,
    times ``E`` or not) is integrated where it lies: the result is a lazy per-walker device
    scalar (``DVec``; with ``intervals`` the ``DMat`` of segment terms), wrapped in a Quantity
    by the same unit rule, and ``np.asarray`` of it gives the numbers.  ``axis`` must then be
    the energy axis (-1 or 1)."""
    y_unit = x_unit = u.dimensionless_unscaled
    if isinstance(y, u.Quantity):
        y, y_unit = y.value, y.unit
    if isinstance(x, u.Quantity):
        x, x_unit = x.value, x.unit
    x = np.asarray(x, dtype=float)
    if x.ndim != 1:
        raise ValueError("x must be one-dimensional")
    if isinstance(y, (DMat, DFactor)):
        res = _trapz_loglog_device(y, x, axis, intervals)
        unit = y_unit * x_unit
        if unit.dims == u.dimensionless_unscaled.dims and unit.scale == 1.0:
            return res
        return u.Quantity(res, unit)
    y = np.asarray(y, dtype=float)
    ym = np.ascontiguousarray(np.moveaxis(y, axis, -1))
    n = ym.shape[-1]
    if n != x.size:
        raise ValueError("x and y have different lengths along the integration axis")
    rows = ym.reshape(-1, n)
    ctx = get_context()
    if intervals:  # the per-segment terms, along the integration axis (utils.py:350-351)
        out = ctx.empty((rows.shape[0], n - 1))
        ctx.call("nh_trapz_loglog_intervals", ctx.array(rows), ctx.array(x), rows.shape[0], n, out)
        res = np.moveaxis(out.get().reshape(ym.shape[:-1] + (n - 1,)), -1, axis)
    else:
        out = ctx.empty((rows.shape[0],))
        ctx.call("nh_trapz_loglog", ctx.array(rows), ctx.array(x), rows.shape[0], n, out)
        res = out.get().reshape(ym.shape[:-1])
    if res.ndim == 0:
        res = float(res)
    unit = y_unit * x_unit
    if unit.dims == u.dimensionless_unscaled.dims and unit.scale == 1.0:
        return res
    return u.Quantity(res, unit)


def _trapz_loglog_device(m, x, axis, intervals):
    """the integral of every row of a lazy device matrix (the flux of a walker batch held in
    HBM) over its energies: a ``DVec`` of one value per walker, or with ``intervals`` the
    ``DMat`` of the (N, n-1) segment terms.  One launch that reads the matrix's terms where they
    lie; nothing is downloaded and nothing synchronises, so a model function may return the
    result as a blob, or put a prior on it, inside the device step loop."""
    if axis not in (-1, 1):
        raise ValueError("a device matrix is integrated along its energy axis (axis=-1 or 1), "
                         "not axis=%r" % (axis,))
    if isinstance(m, DFactor):  # a bare transmission factor: its rows gathered first
        m = m.apply()
    N, n = m.shape
    if n != x.size:
        raise ValueError("x and y have different lengths along the integration axis")
    ctx = m.ctx if m.ctx is not None else get_context()
    ctx.flush(*[t[0] for t in m.terms])  # held-back launches that write these spectra
    cf = ctx.const(m.colfac) if m.colfac is not None else None
    xd = ctx.const(x)
    if intervals:
        if n < 2:
            raise ValueError("intervals=True needs two nodes at least")
        out = ctx.empty((N, n - 1))
        ctx.call("nh_trapz_loglog_comps_intervals", m.comps(), len(m.terms), cf, None, xd, N, n,
                 out, n - 1)
        return DMat.from_buffer(ctx, out, N, n - 1)
    out = ctx.empty((N,))
    ctx.call("nh_trapz_loglog_comps", m.comps(), len(m.terms), cf, None, xd, N, n, out, 1)
    return DVec(ctx, out, out.ptr, N)


def estimate_B(xray_table, vhe_table, photon_energy_density=0.261 * u.eV / u.cm ** 3):
    """Magnetic field from the ratio of X-ray to gamma-ray luminosity,
    L_x / L_gamma = u_B / u_ph = B^2 / (8 pi u_ph) (utils.py:484-542 of the reference;
    Thomson regime, both bands assumed to hold the bulk of the emission): a starting
    value of B for joint X-ray / gamma-ray fits.  Tables as for ``get_sampler``."""
    from .datatable import validate_data_table
    xray = validate_data_table(xray_table, sed=False)
    vhe = validate_data_table(vhe_table, sed=False)
    lum = []
    for t in (xray, vhe):
        e = t["energy"].to("erg")
        f = t["flux"].to("1/(s cm2 erg)")
        lum.append(float(trapz_loglog(f.value * e.value, e.value)))  # erg / (cm2 s)
    uph = photon_energy_density.to("erg/cm3").value
    return u.Quantity(np.sqrt(lum[0] / lum[1] * 8 * np.pi * uph) * 1e6, u.uG)
