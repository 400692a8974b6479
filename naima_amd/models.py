"""Particle-distribution models with naima's class API (models.py:49-422 of the
reference), vectorised over walkers.

Every parameter may be a scalar (one walker, the reference's usage) or a 1-D
array over walkers; a model called inside ``model(pars, data)`` with
``pars[ndim, N]`` then describes N particle spectra at once and the radiative
classes evaluate all of them in one batched HIP launch.  Evaluation itself
(``__call__``) runs the ``nh_particle_weights`` kernel; there is no NumPy path.
"""
import numpy as np

from . import units as u
from . import walker_value as wv
from ._lib import NH_PD_NPAR, PD_KIND, get_context
from .darray import DVec, lazy_const, nh_lazy
from .constants import AR_CGS, C_CGS, ERG_TO_EV, HBAR_CGS, MEC2_ERG, MEC2_EV, R0_CM
from .validator import validate_physical_type, validate_scalar_or_batch

__all__ = ["PowerLaw", "ExponentialCutoffPowerLaw", "BrokenPowerLaw",
           "ExponentialCutoffBrokenPowerLaw", "LogParabola", "CooledElectrons",
           "SynchrotronSelfAbsorption"]


def _validate_ene(ene):
    """models.py:33-46 / radiative.py:43-58: Quantity, or dict/table with 'energy'."""
    if isinstance(ene, dict) or (hasattr(ene, "keys") and not isinstance(ene, u.Quantity)):
        try:
            ene = ene["energy"]
        except KeyError:
            raise TypeError("Table or dict does not have 'energy' column")
    if not isinstance(ene, u.Quantity):
        ene = u.Quantity(ene)
    validate_physical_type("energy", ene, physical_type="energy")
    return ene


class _ParticleDistribution:
    """common machinery: parameter broadcasting and device evaluation"""
    _memoize = False
    kind = None
    # (attribute, slot in the NH_PD_NPAR row, is_energy)
    _slots = ()

    def __setattr__(self, name, value):
        # any parameter change invalidates the packed device rows and weights
        self.__dict__.pop("_rows_dev", None)
        self.__dict__.pop("_w_dev", None)
        self.__dict__.pop("_slot7_packed", None)
        object.__setattr__(self, name, value)

    def _own_values(self):
        """every value that may be given per walker (walker_value)"""
        return [getattr(self, name) for name in self.param_names]

    @property
    def batch_size(self):
        """number of walkers this distribution describes (1 if all parameters are scalars)"""
        return wv.merge(wv.counts(self._own_values()), type(self).__name__)

    @property
    def is_batched(self):
        return wv.is_batched(self._own_values())

    @property
    def on_device(self):
        return wv.on_device(self._own_values())

    def _amplitude_unit(self):
        a = self.amplitude
        return a.unit if isinstance(a, u.Quantity) else u.dimensionless_unscaled

    def _slot_values(self, amplitude_to):
        """(name, slot, bare value in the row's units) of every parameter: the amplitude in
        ``amplitude_to`` when that is given, energies in eV, the rest dimensionless"""
        for name, slot, is_energy in self._slots:
            v = getattr(self, name)
            if name == "amplitude":
                if isinstance(v, u.Quantity):
                    v = v.to(amplitude_to).value if amplitude_to is not None else v.value
            elif is_energy:
                v = v.to("eV").value
            elif isinstance(v, u.Quantity):
                v = v.to(u.dimensionless_unscaled).value
            yield name, slot, v

    def param_rows(self, N, amplitude_to=None):
        """[N, NH_PD_NPAR] float64 rows (include/naima_hip.h); amplitude converted to
        ``amplitude_to`` (e.g. 1/eV) when given, energies in eV."""
        rows = np.zeros((N, NH_PD_NPAR))
        for name, slot, v in self._slot_values(amplitude_to):
            rows[:, slot] = np.asarray(v, dtype=float)
        if not any(s[0] == "beta" for s in self._slots):
            rows[:, 4] = 1.0
        return rows

    def device_rows(self, ctx, N, amplitude_to=None):
        """the [N][NH_PD_NPAR] parameter rows in HBM, packed by ``nh_pack_rows`` from
        host scalars, host vectors or lazy device scalars (no host round trip)"""
        cache = self.__dict__.setdefault("_rows_dev", {})
        key = (N, None if amplitude_to is None else amplitude_to.name)
        hit = cache.get(key)
        if hit is not None:
            return hit
        cols = (nh_lazy * NH_PD_NPAR)()
        for j in range(NH_PD_NPAR):
            cols[j] = lazy_const(1.0 if j == 4 else 0.0)
        keep = []
        # slot 7 is free: a Synchrotron built on this distribution parks its (device)
        # magnetic field there so that one pack launch serves every component
        rider = self.__dict__.get("_slot7")
        if isinstance(rider, DVec) and rider.n == N:
            cols[7] = rider.lazy()
            keep.append(rider)
            self.__dict__["_slot7_packed"] = rider
        for name, slot, v in self._slot_values(amplitude_to):
            cols[slot], k = wv.lazy(ctx, v, N=N, mismatch="parameter " + name
                                    + " has %d walkers, batch has %d")
            if k is not None:
                keep.append(k)
        out = ctx.pack_rows(cols, NH_PD_NPAR, N)
        cache[key] = out
        return out

    def __call__(self, e):
        """dN/dE at energies ``e`` -- shape (n_e,) or (N, n_e) for a walker batch.
        Runs on the GPU (nh_particle_weights, n_out)."""
        e = _validate_ene(e)
        scalar_in = e.isscalar
        e_eV = np.atleast_1d(e.to("eV").value).astype(float).ravel()
        N = self.batch_size
        ctx = get_context()
        rows = self.device_rows(ctx, N)
        ed = ctx.const(e_eV)
        nG = e_eV.size
        if nG < 2:  # the kernel wants a grid; pad a single energy
            ed = ctx.const(np.concatenate([e_eV, e_eV * 2.0]))
            nG2 = 2
        else:
            nG2 = nG
        w, lw, n = ctx.empty((N, nG2)), ctx.empty((N, nG2)), ctx.empty((N, nG2))
        ctx.call("nh_particle_weights", PD_KIND[self.kind], rows, N, ed, ed, nG2, 1.0, w, lw, n)
        out = n.get()[:, :nG].reshape((N,) + e.shape if not scalar_in else (N,))
        if not self.is_batched:
            out = out[0]
        return u.Quantity(out, self._amplitude_unit())


class PowerLaw(_ParticleDistribution):
    """f(E) = A (E/E0)^-alpha   (models.py:49-106)"""
    param_names = ["amplitude", "e_0", "alpha"]
    kind = "PowerLaw"
    _slots = (("amplitude", 0, False), ("e_0", 1, True), ("alpha", 2, False))

    def __init__(self, amplitude, e_0, alpha):
        self.amplitude = amplitude
        self.e_0 = validate_scalar_or_batch("e_0", e_0, domain="positive", physical_type="energy")
        self.alpha = alpha


class ExponentialCutoffPowerLaw(_ParticleDistribution):
    """f(E) = A (E/E0)^-alpha exp(-(E/Ecutoff)^beta)   (models.py:109-177)"""
    param_names = ["amplitude", "e_0", "alpha", "e_cutoff", "beta"]
    kind = "ExponentialCutoffPowerLaw"
    _slots = (("amplitude", 0, False), ("e_0", 1, True), ("alpha", 2, False),
              ("e_cutoff", 3, True), ("beta", 4, False))

    def __init__(self, amplitude, e_0, alpha, e_cutoff, beta=1.0):
        self.amplitude = amplitude
        self.e_0 = validate_scalar_or_batch("e_0", e_0, domain="positive", physical_type="energy")
        self.alpha = alpha
        self.e_cutoff = validate_scalar_or_batch("e_cutoff", e_cutoff, domain="positive",
                                                 physical_type="energy")
        self.beta = beta


class BrokenPowerLaw(_ParticleDistribution):
    """A (E/E0)^-alpha_1 below e_break; A (Eb/E0)^(a2-a1) (E/E0)^-alpha_2 above
    (models.py:180-254)"""
    param_names = ["amplitude", "e_0", "e_break", "alpha_1", "alpha_2"]
    kind = "BrokenPowerLaw"
    _slots = (("amplitude", 0, False), ("e_0", 1, True), ("e_break", 5, True),
              ("alpha_1", 2, False), ("alpha_2", 6, False))

    def __init__(self, amplitude, e_0, e_break, alpha_1, alpha_2):
        self.amplitude = amplitude
        self.e_0 = validate_scalar_or_batch("e_0", e_0, domain="positive", physical_type="energy")
        self.e_break = validate_scalar_or_batch("e_break", e_break, domain="positive",
                                                physical_type="energy")
        self.alpha_1 = alpha_1
        self.alpha_2 = alpha_2


class ExponentialCutoffBrokenPowerLaw(_ParticleDistribution):
    """broken power law times exp(-(E/Ecutoff)^beta)   (models.py:257-354)"""
    param_names = ["amplitude", "e_0", "e_break", "alpha_1", "alpha_2", "e_cutoff", "beta"]
    kind = "ExponentialCutoffBrokenPowerLaw"
    _slots = (("amplitude", 0, False), ("e_0", 1, True), ("e_break", 5, True),
              ("alpha_1", 2, False), ("alpha_2", 6, False), ("e_cutoff", 3, True),
              ("beta", 4, False))

    def __init__(self, amplitude, e_0, e_break, alpha_1, alpha_2, e_cutoff, beta=1.0):
        self.amplitude = amplitude
        self.e_0 = validate_scalar_or_batch("e_0", e_0, domain="positive", physical_type="energy")
        self.e_break = validate_scalar_or_batch("e_break", e_break, domain="positive",
                                                physical_type="energy")
        self.alpha_1 = alpha_1
        self.alpha_2 = alpha_2
        self.e_cutoff = validate_scalar_or_batch("e_cutoff", e_cutoff, domain="positive",
                                                 physical_type="energy")
        self.beta = beta


class LogParabola(_ParticleDistribution):
    """f(E) = A (E/E0)^(-alpha - beta ln(E/E0))   (models.py:357-422)"""
    param_names = ["amplitude", "e_0", "alpha", "beta"]
    kind = "LogParabola"
    _slots = (("amplitude", 0, False), ("e_0", 1, True), ("alpha", 2, False),
              ("beta", 4, False))

    def __init__(self, amplitude, e_0, alpha, beta):
        self.amplitude = amplitude
        self.e_0 = validate_scalar_or_batch("e_0", e_0, domain="positive", physical_type="energy")
        self.alpha = alpha
        self.beta = beta


class TableModel:
    """A model from a table of energies and values, interpolated with a cubic spline in
    log-log space; zero outside the table (models.py:425-467).  As the particle
    distribution of a radiative model its SHAPE on the particle grid is
    walker-independent (evaluated once on the host, as the reference does, and cached in
    HBM); only ``amplitude`` may vary per walker or live on the device."""
    param_names = ["amplitude"]
    kind = "table"

    def __init__(self, energy, values, amplitude=1):
        from scipy.interpolate import interp1d

        from .validator import validate_array
        self._energy = validate_array("energy", energy, domain="positive", physical_type="energy")
        self._values = values
        self.amplitude = amplitude
        loge = np.log10(self._energy.to("eV").value)
        if isinstance(values, u.Quantity):
            self.unit = values.unit
            with np.errstate(divide="ignore"):
                logy = np.log10(values.value)
        else:
            self.unit = u.dimensionless_unscaled
            with np.errstate(divide="ignore"):
                logy = np.log10(values)
        self._interplogy = interp1d(loge, logy, fill_value=-np.inf, bounds_error=False,
                                    kind="cubic")

    def __setattr__(self, name, value):
        self.__dict__[name] = value
        if name == "amplitude":
            self.__dict__.pop("_w_dev", None)

    def _shape(self, e_eV):
        """10**interp(log10 E): the table's values (in ``self.unit``) at E [eV]"""
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            return np.power(10, self._interplogy(np.log10(np.asarray(e_eV, dtype=float))))

    @property
    def _amp(self):
        a = self.amplitude
        return a.value if isinstance(a, u.Quantity) else a

    @property
    def on_device(self):
        return wv.classify(self._amp)[0] is wv.DEVICE

    @property
    def batch_size(self):
        return int(wv.classify(self._amp)[1])

    @property
    def is_batched(self):
        return wv.per_walker(self._amp)

    def __call__(self, e):
        e = _validate_ene(e)
        interpy = self._shape(e.to("eV").value)
        a = self._amp
        if np.ndim(a) > 0 and np.ndim(interpy) > 0:
            a = np.asarray(a, dtype=float)[:, None]
        return u.Quantity(a * interpy, self.unit)


_EBL_FILE = ("data", "tau_dominguez11.npz")
_ebl_cache = {}


def _ebl_spline():
    """the Dominguez table as the scalar path interpolates it, every tabulated redshift at
    once: (log10 E/eV of the table, the tabulated redshifts, knots, coefficients [n][399]).
    make_interp_spline of all the columns is what interp1d(kind="cubic") evaluates column by
    column (the same coefficients, bit for bit); built once per process."""
    hit = _ebl_cache.get("spline")
    if hit is None:
        import os

        from scipy.interpolate import make_interp_spline

        from .validator import validate_array
        tab = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), *_EBL_FILE))
        energy = validate_array("energy", tab["energy_TeV"] * u.TeV, domain="positive",
                                physical_type="energy")
        loge = np.log10(energy.to("eV").value)
        v = np.array(tab["table"], dtype=float)
        v[v > 150.0] = 150.0
        with np.errstate(divide="ignore"):
            logy = np.log10((10 ** v * u.dimensionless_unscaled).value)
        spl = make_interp_spline(loge, logy, k=3)
        hit = (loge, np.arange(0.01, 4, 0.01), np.ascontiguousarray(spl.t),
               np.ascontiguousarray(spl.c))
        _ebl_cache["spline"] = hit
    return hit


def _ebl_codes(e):
    """per energy: log10(E/eV) and the scalar path's decisions, made with its own unit
    conversions (nh_ebl_table's codes: below 1 GeV, above 100 TeV, outside the table)"""
    from ._lib import NH_EBL_HIGH, NH_EBL_ONE, NH_EBL_OUTSIDE
    ev = np.atleast_1d(e.to("eV").value).astype(float).ravel()
    e_GeV = np.atleast_1d(e.to("GeV").value).ravel()
    e_TeV = np.atleast_1d(e.to("TeV").value).ravel()
    loge = _ebl_spline()[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log10(ev)
    code = np.where(e_GeV < 1.0, NH_EBL_ONE, np.where(e_TeV > 100.0, NH_EBL_HIGH, 0))
    code = code | np.where((x < loge[0]) | (x > loge[-1]), NH_EBL_OUTSIDE, 0)
    return x, code.astype(np.int32)


def _ebl_table(ctx, x, code, kind):
    """(Tab[400][nE], ...) of one kind -- "transmission" or "call" (10**S) -- at these
    energies: one nh_ebl_table launch, cached like the emission tables (and pinned with them
    for captured graphs).  The entry keeps the arrays its key and nh_ebl_apply point at."""
    from . import _lib
    xd, cd = ctx.const(x), ctx.const(code, dtype=np.int32)

    def build():
        _, zl, t, c = _ebl_spline()
        td, cfd = ctx.const(t), ctx.const(c)
        out = ctx.empty((c.shape[1] + 1, x.size))
        T, P = (out.ptr, None) if kind == "transmission" else (None, out.ptr)
        # (a table build, not a step-loop launch: called directly, never recorded in a plan)
        _lib._chk(_lib._lib.nh_ebl_table(ctx.h, td.ptr, t.size, cfd.ptr, c.shape[1], xd.ptr,
                                         cd.ptr, x.size, float(np.exp(-np.log10(6000.0))), T, P))
        return out, ctx.const(zl), xd, cd

    return ctx.table(("ebl", kind, xd.ptr, cd.ptr), build)


class EblAbsorptionModel(TableModel):
    """Opacity of the extragalactic background light (Dominguez et al. 2011) at a given
    redshift as a TableModel; ``transmission(e)`` is the factor to multiply a flux with
    (models.py:470-552).  No interpolation in redshift: the closest tabulated z
    (step 0.01) is used, as in the reference.

    ``redshift`` may also be one value per walker: a 1-D host array, or a device parameter
    (``pars[5]`` or ``pars[5] * u.dimensionless_unscaled`` in a model on the device loop).
    ``transmission(e)`` and ``__call__(e)`` then have shape (N, n_e) and come from the GPU:
    a walker-independent table of every tabulated redshift at these energies (built once,
    cached) and one gathered row per walker (nh_ebl_table / nh_ebl_apply).  On the host they
    are an ndarray and a Quantity; on the device a lazy factor (``darray.DEbl``) that
    multiplies a device flux.  A walker whose redshift is negative, NaN or infinite gets a
    NaN row instead of the scalar's ValueError: a prior that excludes z < 0 gives it -inf,
    and without one the sampler's ``nan_policy`` applies (-0.0 is valid, as in the
    reference)."""

    def __init__(self, redshift, ebl_absorption_model="Dominguez"):
        import os

        from .validator import validate_scalar
        if wv.is_vector(redshift):  # one redshift per walker: 1-D host array or DVec
            self._init_batch(redshift, ebl_absorption_model)
            return
        if not isinstance(redshift, u.Quantity):
            redshift = redshift * u.dimensionless_unscaled
        self.redshift = validate_scalar("redshift", redshift, domain="positive",
                                        physical_type="dimensionless")
        self.model = ebl_absorption_model
        if self.model != "Dominguez":
            raise ValueError('Model should be one of: ["Dominguez"]')
        fname = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data",
                             "tau_dominguez11.npz")
        tab = np.load(fname)
        energy = tab["energy_TeV"] * u.TeV
        z = float(self.redshift.value)
        if z >= 0.01:
            redshift_list = np.arange(0.01, 4, 0.01)
            col = int(np.abs(redshift_list - z).argmin())
            table_values = np.array(tab["table"][:, col], dtype=float)
            table_values[table_values > 150.0] = 150.0  # high enough; avoids overflow later
            taus = 10 ** table_values * u.dimensionless_unscaled
        else:
            taus = 10 ** np.zeros(len(tab["energy_TeV"])) * u.dimensionless_unscaled
        super().__init__(energy, taus)

    def _init_batch(self, redshift, ebl_absorption_model):
        from .darray import DVec
        from .validator import validate_physical_type
        if not isinstance(redshift, u.Quantity):
            redshift = u.Quantity(redshift, u.dimensionless_unscaled)
        validate_physical_type("redshift", redshift, physical_type="dimensionless")
        z = redshift.to(u.dimensionless_unscaled).value
        if not isinstance(z, DVec):
            z = np.asarray(z, dtype=float)
        self.redshift = u.Quantity(z, u.dimensionless_unscaled)
        self.model = ebl_absorption_model
        if self.model != "Dominguez":
            raise ValueError('Model should be one of: ["Dominguez"]')
        self.amplitude = 1
        self.unit = u.dimensionless_unscaled

    @property
    def _batch(self):
        return "_interplogy" not in self.__dict__

    def _factor(self, e, kind):
        """the per-walker factor at energies e: a DEbl over the walkers' redshifts"""
        from ._lib import get_context
        from .darray import DEbl, DVec
        x, code = _ebl_codes(_validate_ene(e))
        ctx = get_context()
        tab, zl, _, _ = _ebl_table(ctx, x, code, kind)
        z = self.redshift.value
        if not isinstance(z, DVec):
            zd = ctx.array(z)
            z = DVec(ctx, zd, zd.ptr, z.size)
        return DEbl(ctx, tab, zl, z, x.size)

    def __call__(self, e):
        if not self._batch:
            return super().__call__(e)
        f = self._factor(e, "call")
        return u.Quantity(f if self.redshift.on_device else f.get(), self.unit)

    def transmission(self, e):
        if self._batch:
            f = self._factor(e, "transmission")
            return f if self.redshift.on_device else f.get()
        e = _validate_ene(e)
        ev = np.atleast_1d(e.to("eV").value).astype(float)
        e_GeV = np.atleast_1d(e.to("GeV").value)
        e_TeV = np.atleast_1d(e.to("TeV").value)
        taus = np.zeros(len(ev))
        for i in range(len(ev)):
            if e_GeV[i] < 1.0:
                taus[i] = 0.0
            elif e_TeV[i] > 100.0:
                taus[i] = np.log10(6000.0)
            else:
                taus[i] = np.log10(float(np.asarray(self(ev[i] * u.eV).value)))
        return np.exp(-taus)


# k_B / (m_e c^2) per kelvin, from the radiation constant a = pi^2 k_B^4 / (15 (hbar c)^3)
_K_TO_MEC2 = (15.0 * AR_CGS * (HBAR_CGS * C_CGS) ** 3 / np.pi ** 2) ** 0.25 / MEC2_ERG


_pa_rows = {}  # the (n_e,) rows of scalar models, by content (PairAbsorptionModel._result)


class PairAbsorptionModel:
    """Absorption of gamma rays by pair production (gamma gamma -> e+ e-, the Breit-Wheeler
    cross section) on photon fields along the line of sight: inside the Galaxy on the CMB and
    the dust fields above ~100 TeV, in a binary or a compact nebula on the source's own field.

    ``seed_photon_fields`` follows the grammar of ``InverseCompton``: 'CMB' | 'FIR' | 'NIR' |
    [name, T, u] | [name, T, u, theta] | [name, E, density] (monochromatic: energy density) |
    [name, E[], density[]] (tabulated).  The three-element forms are isotropic; with ``theta``
    the field comes from one direction and 1 - cos(theta) enters (theta = 0: no absorption).
    ``path_length`` is one length, or a sequence with one length per field.

    ``opacity(e)`` is tau(E) = sum over the fields of L * dtau/dl and ``transmission(e)`` is
    exp(-tau), the factor to multiply a flux with (for scalars a ``darray.FactorRow``: an
    ndarray that a device flux multiplies with, and the device loop keeps as a blob, as N equal
    rows from nh_pairabs_apply).  T, u and theta of a thermal field, the
    density of a monochromatic field and every path length may each be a scalar, a 1-D host
    array (one value per walker) or a device parameter (``pars[4] * u.kpc`` in a model function
    on the device loop); the results are then an (n_e,) ndarray, an (N, n_e) ndarray, or a lazy
    device factor (``darray.DPairAbs``) that multiplies a device flux in one launch.  All three
    come from the same kernels (nh_pairabs_rows / nh_pairabs_apply): the opacity per unit
    length and density of a field whose shape every walker shares is built once per set of
    energies and cached; a thermal field with a per-walker T or theta gets a row per walker at
    every evaluation.  The energies of monochromatic and tabulated fields are the same for every
    walker.

    Scalars are validated as in the reference's models (``ValueError`` for a negative or
    non-finite value, a temperature that is not positive).  A walker of a batch whose path
    length, energy density or density is negative, NaN or infinite, or whose temperature is
    <= 0, NaN or infinite, gets a NaN row: a prior that excludes it gives -inf, and without one
    the sampler's ``nan_policy`` applies."""

    def __init__(self, seed_photon_fields, path_length):
        from .radiative import InverseCompton
        from .validator import validate_physical_type, validate_scalar
        self._check_seed_energies(seed_photon_fields)
        self.seed_photon_fields = InverseCompton._process_input_seed(seed_photon_fields)
        nf = len(self.seed_photon_fields)
        if nf > 8:
            raise ValueError("at most 8 photon fields, got %d" % nf)
        if isinstance(path_length, (list, tuple)):
            lengths = list(path_length)
            if len(lengths) != nf:
                raise ValueError("path_length has %d entries for %d photon fields"
                                 % (len(lengths), nf))
        else:
            lengths = [path_length] * nf
        for name, L in zip(self.seed_photon_fields, lengths):
            validate_physical_type("{0}-path_length".format(name), L, "length")
            if not (L.on_device or np.ndim(L.value) > 0):
                validate_scalar("{0}-path_length".format(name), L, domain="positive",
                                physical_type="length")
        self.path_length = lengths
        for name, seed in self.seed_photon_fields.items():
            if seed["type"] == "thermal":
                T = seed["T"]
                if not (T.on_device or np.ndim(T.value) > 0) and not T.value > 0:
                    raise ValueError("{0}-T value should be strictly positive".format(name))
            elif seed["energy"].size == 1:
                d = seed["photon_density"]
                if not d.on_device and np.size(d.value) == 1:
                    validate_scalar("{0}-density".format(name),
                                    u.Quantity(float(np.ravel(d.value)[0]), d.unit),
                                    domain="positive", physical_type="pressure")
            elif seed["photon_density"].on_device or np.ndim(seed["photon_density"].value) != 1:
                raise NotImplementedError(
                    "%s-density must be the same for every walker of a batch (the tabulated "
                    "field's opacity is shared); evaluate walkers with different %s-density in "
                    "separate calls" % (name, name))

    @staticmethod
    def _check_seed_energies(seed_photon_fields):
        """the energies of a monochromatic or tabulated field are walker-independent"""
        if type(seed_photon_fields) is not list:
            return
        for s in seed_photon_fields:
            if type(s) is list and len(s) in (3, 4) and isinstance(s[1], u.Quantity) \
                    and s[1].unit.physical_type != "temperature" \
                    and (s[1].on_device or np.ndim(s[1].value) > 1):
                raise NotImplementedError(
                    "%s-energy must be the same for every walker of a batch (the field's opacity "
                    "is shared); evaluate walkers with different %s-energy in separate calls"
                    % (s[0], s[0]))

    # -- what is given per walker ----------------------------------------------------------
    def _own_values(self):
        """every Quantity that may be given per walker"""
        qs = list(self.path_length)
        for seed in self.seed_photon_fields.values():
            if seed["type"] == "thermal":
                qs += [seed["T"], seed["u"]]
            elif seed["energy"].size == 1:
                qs.append(seed["photon_density"])
            if not seed["isotropic"]:
                qs.append(seed["theta"])
        return qs

    @property
    def on_device(self):
        return wv.on_device(self._own_values())

    @property
    def batch_size(self):
        """walkers of the batch (None: scalars everywhere).  A host array of one element is a
        scalar here, and every other count has to agree, a device value of one walker too"""
        def count(q):
            form, n = wv.classify(q)
            return n if form is wv.DEVICE or (wv.is_vector(q) and n > 1) else None
        return wv.merge([count(q) for q in self._own_values()], broadcast_one=False)

    def _values(self, ctx):
        """per field: (seed, L [cm], dens, T [K] or None, theta [rad] or None) as floats or
        DVecs; dens is u [erg/cm3] of a thermal field, photons/cm3 of a monochromatic one and
        1 for a tabulated one"""
        out = []
        for (name, seed), L in zip(self.seed_photon_fields.items(), self.path_length):
            Lv = wv.resolve(ctx, L, "cm", fold=True)
            th = None if seed["isotropic"] else wv.resolve(ctx, seed["theta"], "rad", fold=True)
            if seed["type"] == "thermal":
                out.append((seed, Lv, wv.resolve(ctx, seed["u"], "erg/cm3", fold=True),
                            wv.resolve(ctx, seed["T"], "K", fold=True), th))
            elif seed["energy"].size == 1:
                d = seed["photon_density"]
                if not d.on_device and np.size(d.value) == 1:
                    d = u.Quantity(float(np.ravel(d.value)[0]), d.unit)
                out.append((seed, Lv, wv.resolve(ctx, d, "eV/cm3", fold=True)
                            / float(seed["energy"].to("eV").value[0]), None, th))
            else:
                out.append((seed, Lv, 1.0, None, th))
        return out

    # -- the kernels -------------------------------------------------------------------------
    @staticmethod
    def _rows_launch(ctx, direct, kind, T, theta, se, sn, ns, xd, nE, nrows, out):
        """one nh_pairabs_rows launch: a cached table build is called directly and is never
        recorded in a plan; per-walker rows go through ctx.call, so a step plan records them"""
        import ctypes as C

        from . import _lib
        from .darray import as_lazy
        lT = as_lazy(T if T is not None else 0.0)
        lth = as_lazy(theta) if theta is not None else None
        args = (kind, _K_TO_MEC2, C.byref(lT), C.byref(lth) if lth is not None else None,
                se.ptr if se is not None else None, sn.ptr if sn is not None else None, ns,
                xd.ptr, nE, nrows, out.ptr, nE)
        if direct:
            _lib._chk(_lib._lib.nh_pairabs_rows(ctx.h, *args))
        else:
            ctx.call("nh_pairabs_rows", *args)

    def _kappa(self, ctx, seed, T, theta, xd, nE, N):
        """(kappa DeviceArray, per_walker) of one field at the energies xd"""
        from ._lib import NH_PAIR_MONO, NH_PAIR_TABLE, NH_PAIR_THERMAL
        from .darray import DVec
        if seed["type"] == "thermal" and (isinstance(T, DVec) or isinstance(theta, DVec)):
            out = ctx.empty((N, nE))
            self._rows_launch(ctx, False, NH_PAIR_THERMAL, T, theta, None, None, 0, xd, nE, N, out)
            return out, True
        if isinstance(theta, DVec):
            raise NotImplementedError(
                "theta of a monochromatic or tabulated field must be the same for every walker "
                "of a batch (the field's opacity is shared); evaluate walkers with different "
                "theta in separate calls")
        if seed["type"] == "thermal":
            key = ("pairabs", "T", T, theta, xd.ptr)
            build_args = (NH_PAIR_THERMAL, T, theta, None, None, 0)
        else:
            se = ctx.const(np.atleast_1d(seed["energy"].to("eV").value).astype(float))
            mono = se.shape[0] == 1
            sn = None if mono else ctx.const(
                np.asarray(seed["photon_density"].to("1/(eV cm3)").value, dtype=float))
            key = ("pairabs", "A", se.ptr, None if mono else sn.ptr, theta, xd.ptr)
            build_args = (NH_PAIR_MONO if mono else NH_PAIR_TABLE, None, theta, se, sn,
                          se.shape[0])

        def build():
            out = ctx.empty((1, nE))
            self._rows_launch(ctx, True, *build_args, xd, nE, 1, out)
            return out, xd, build_args  # (the entry keeps the arrays its key points at)

        return ctx.table(key, build)[0], False

    def _factor(self, e, tau, rows=None):
        """(the DPairAbs at energies e, the batch size or None); ``rows``: that many equal rows
        of a model whose values are all scalars"""
        from .darray import DPairAbs
        e = _validate_ene(e)
        x = np.atleast_1d(e.to("eV").value).astype(float).ravel() / MEC2_EV
        ctx = get_context()
        xd = ctx.const(x)
        N = self.batch_size
        N1 = (rows or 1) if N is None else N
        fields = []
        for seed, L, dens, T, theta in self._values(ctx):
            kappa, per_walker = self._kappa(ctx, seed, T, theta, xd, x.size, N1)
            fields.append((kappa, per_walker, L, dens, T))
        return DPairAbs(ctx, fields, N1, x.size, tau=tau), N

    def _result(self, e, tau):
        f, N = self._factor(e, tau)
        if self.on_device:
            return f
        if N is not None:
            return f.get()
        # scalars everywhere: the row is remembered by what it depends on, so that a model
        # function with nothing free in its absorber downloads nothing at its later evaluations
        # (none is possible while a graph is captured)
        x = np.atleast_1d(_validate_ene(e).to("eV").value).astype(float).ravel()
        key = (id(f.ctx), tau, x.tobytes()) + tuple(
            (seed["type"], L, dens, T, theta,
             None if seed["type"] == "thermal" else (
                 seed["energy"].to("eV").value.tobytes(),
                 np.asarray(seed["photon_density"].value, dtype=float).tobytes(),
                 str(seed["photon_density"].unit)))
            for seed, L, dens, T, theta in self._values(f.ctx))
        row = _pa_rows.get(key)
        if row is None:
            if len(_pa_rows) >= 64:
                _pa_rows.clear()
            row = _pa_rows[key] = f.get()[0]
        if tau:
            return row.copy()
        from .darray import FactorRow
        return FactorRow(row, lambda n: self._factor(e, False, rows=n)[0])

    def opacity(self, e):
        """tau(E): (n_e,) for scalars, (N, n_e) for a host batch, a lazy device factor
        for device values"""
        return self._result(e, True)

    def transmission(self, e):
        """exp(-tau(E)), the factor to multiply a flux with; shapes as for ``opacity``"""
        return self._result(e, False)


class SynchrotronSelfAbsorption:
    """Synchrotron self-absorption of the electron population of a ``Synchrotron`` model in a
    homogeneous source of radius ``radius``: what turns the optically thin spectrum of a compact
    source (a blazar zone, a radio supernova, a young nebula at radio frequencies) over into
    nu^(5/2) below the frequency at which it becomes opaque to itself.

    ``absorption_area(e)`` is kappa(E) = alpha(E) V in cm^2, the absorption coefficient times
    the source's volume, from the same per-electron emissivity, field and particle weights as
    the emission (nh_syn_absorption: the form integrated by parts, which holds no derivative of
    the distribution and is right for a truncated one).  ``opacity(e)`` is the optical depth
    and ``transmission(e)`` the fraction f(tau) of the optically thin flux that escapes:

      'sphere' (default)  tau = 3 kappa / (2 pi R^2) along a diameter,
                          f = 3 u / tau, u = 1/2 + exp(-tau)/tau - (1 - exp(-tau))/tau^2
      'slab'              a face-on cylinder of face radius R, of any depth:
                          tau = kappa / (pi R^2), f = (1 - exp(-tau)) / tau

    ``B`` and the distribution's parameters (the synchrotron model's) and ``radius`` may each
    be scalars, 1-D host arrays (one value per walker) or device parameters; the results are
    then an (n_e,) array (the transmission a ``darray.FactorRow``), an (N, n_e) array, or a
    lazy device factor (``darray.DSsa``) that multiplies a device flux in one launch.  All
    three come from the same two kernels (nh_syn_absorption / nh_ssa_apply).

    A scalar radius is validated as a positive length.  A walker of a batch whose radius is
    <= 0, NaN or infinite, or whose field is, gets a NaN row: a prior that excludes it gives
    -inf, and without one the sampler's ``nan_policy`` applies.  Eemin, Eemax or nEed per walker
    raise ``NotImplementedError``."""

    def __init__(self, synchrotron, radius, geometry="sphere"):
        from ._lib import NH_SSA_GEOMETRY
        from .validator import validate_physical_type, validate_scalar
        if not (hasattr(synchrotron, "_absorption_rows") and hasattr(synchrotron, "B")):
            raise TypeError("SynchrotronSelfAbsorption needs a naima_amd Synchrotron model, got %r"
                            % type(synchrotron).__name__)
        if geometry not in NH_SSA_GEOMETRY:
            raise ValueError("geometry should be one of: %s" % sorted(NH_SSA_GEOMETRY))
        validate_physical_type("radius", radius, "length")
        if not (radius.on_device or np.ndim(radius.value) > 0):
            validate_scalar("radius", radius, domain="strictly-positive", physical_type="length")
        elif not radius.on_device and np.ndim(radius.value) != 1:
            raise TypeError("a per-walker radius must be a 1-D array, got shape %r"
                            % (np.shape(radius.value),))
        self.synchrotron, self.radius, self.geometry = synchrotron, radius, geometry

    @property
    def on_device(self):
        return bool(self.synchrotron.on_device) or wv.on_device([self.radius])

    @property
    def batch_size(self):
        """walkers of the batch (None: scalars everywhere)"""
        syn = self.synchrotron
        form, n = wv.classify(self.radius)
        mine = n if form is wv.DEVICE or (form is wv.HOST and n > 1) else None
        return wv.merge([syn.batch_size if syn.is_batched else None, mine],
                        "SynchrotronSelfAbsorption", broadcast_one=False)

    def _energies(self, e):
        return np.atleast_1d(_validate_ene(e).to("eV").value).astype(float).ravel()

    def _factor(self, e, tau, rows=None):
        """(the DSsa at energies e, the batch size or None); ``rows``: that many equal rows of
        a model whose values are all scalars"""
        from .darray import DSsa
        E_eV = self._energies(e)
        N = self.batch_size
        ctx, Ns, kappa = self.synchrotron._absorption_rows(E_eV)
        N1 = (rows or 1) if N is None else N
        R = wv.resolve(ctx, self.radius, "cm", fold=True)
        return DSsa(ctx, kappa, Ns == N1, R, self.geometry, N1, E_eV.size, tau=tau), N

    def _result(self, e, tau):
        f, N = self._factor(e, tau)
        if self.on_device:
            return f
        if N is not None:
            return f.get()
        row = f.get()[0]
        if tau:
            return row
        from .darray import FactorRow
        return FactorRow(row, lambda n: self._factor(e, False, rows=n)[0])

    def absorption_area(self, e):
        """kappa(E) = alpha(E) V in cm^2: (n_e,) for scalars, (N, n_e) for a batched population
        (on the device a lazy matrix)"""
        from .darray import DMat
        E_eV = self._energies(e)
        ctx, Ns, kappa = self.synchrotron._absorption_rows(E_eV)
        if self.synchrotron.on_device:
            return u.Quantity(DMat.from_buffer(ctx, kappa, Ns, E_eV.size), u.cm ** 2)
        k = kappa.get()
        return u.Quantity(k if self.synchrotron.is_batched else k[0], u.cm ** 2)

    def opacity(self, e):
        """tau(E): (n_e,) for scalars, (N, n_e) for a host batch, a lazy device factor for
        device values"""
        return self._result(e, True)

    def transmission(self, e):
        """f(tau(E)), the factor to multiply the optically thin flux with; shapes as for
        ``opacity``"""
        return self._result(e, False)


# ---- cooled electron populations ---------------------------------------------------------------
_SIGMA_T_CGS = 8.0 * np.pi / 3.0 * R0_CM ** 2
# synchrotron loss rate [eV/s] = _COOL_SYN B[G]^2 E[eV]^2: (4/3) sigma_T c (B^2 / 8 pi) gamma^2
_COOL_SYN = (4.0 / 3.0) * _SIGMA_T_CGS * C_CGS / (8.0 * np.pi) * ERG_TO_EV / (MEC2_EV * MEC2_EV)
_COOL_MAX_NODES = 2048  # nh_cooled_electrons keeps 40 B of LDS per node


def _cool_zgrid(x0, per_decade=200, edge_per_decade=100):
    """the outgoing photon energies, as fractions z = E_ph / E_e of the electron's energy, over
    which an electron's inverse-Compton emissivity on a Planck field is integrated to its loss
    rate; x0 = 4 gamma kT / (m_e c^2) of the LOWEST electron energy.  Log-spaced in z from 1e-4
    of the Thomson peak of that electron (below the peak z^2 K ~ z^2: 1e-8 of the integral is left
    out) to 1/2, then log-spaced in 1 - z down to 1e-7, which resolves the Klein-Nishina edge at
    z -> 1 (its width is 1 / (4 gamma kT) >= 1e-5 for the fields and energies in reach)."""
    z_lo = 1e-4 * x0 / (1.0 + x0)
    l0, l1 = np.log10(z_lo), np.log10(0.5)
    lower = np.logspace(l0, l1, max(2, int(per_decade * (l1 - l0))))
    upper = 1.0 - np.logspace(l1, -7.0, max(2, int(edge_per_decade * (l1 + 7.0))))[1:]
    return np.concatenate([lower, upper])


def _cool_loss_scale(T_K):
    """(energy-weighted integral of the IC kernel over E_ph / mec2) -> eV/s per erg/cm3"""
    return MEC2_EV / (AR_CGS * T_K ** 4)


class CooledElectrons:
    """The electron population that an injection rate Q(E) leaves after a time ``age`` of
    synchrotron and inverse-Compton cooling -- the break energy is no free parameter but follows
    from ``B``, the photon fields and the age:

        n(E) = int_E^E* Q dE' / b(E),   int_E^E* dE' / b = age   (E* = Emax if never reached),
        b(E) = (4/3) sigma_T c (B^2 / 8 pi) gamma^2 + sum_f u_f l_f(E)

    with l_f the inverse-Compton loss per unit energy density of field f, Klein-Nishina included:
    the energy-weighted integral of the emissivity that ``InverseCompton`` itself uses for a
    thermal field of that temperature, so cooling and emission of one fit agree.  ``age=np.inf`` is
    the steady state.  Losses are continuous, B and the injection constant in time, and injection
    above ``Emax`` is ignored: the population falls to zero at ``Emax``.

    ``injection`` is one of the five analytic distributions with an amplitude in 1/(energy time)
    (``PowerLaw(1e36 / u.eV / u.s, ...)``), a ``SecondaryLeptonsKelner06(..., product="electron")``
    (its source spectrum is the rate), or a pair ``(energies, rates)`` with rates of shape (nC,)
    or (N, nC), host or device; the energies of a pair ARE the solve grid (``Emin``, ``Emax`` and
    ``n_per_decade`` are not used then).  ``B``, ``age`` and the energy density u of every field
    may each be a scalar, a 1-D host array (one value per walker) or a device parameter
    (``pars[0] * u.uG``, ``10 ** pars[1] * u.yr``).  ``seed_photon_fields`` follows
    ``InverseCompton``'s grammar for thermal fields; a field given with an angle cools like the
    isotropic field of the same T and u (the electrons are isotropic).  The temperatures are the
    same for every walker; the loss table of each is built in the constructor (two launches per
    field), once per temperature and grid, and cached in HBM.

    The solve runs on the model's own log-uniform grid (2 .. 2048 nodes) in one launch,
    ``nh_cooled_electrons``, one workgroup per walker; ``Synchrotron``, ``InverseCompton`` and
    ``Bremsstrahlung`` resample it onto their particle grids (``nh_cooled_weights``).  A walker
    with age <= 0 or NaN, B NaN, B <= 0 and no positive u, or a negative or non-finite u gets a
    NaN row: put a prior on them.  The amplitude is a rate, so ``set_We`` does not apply;
    ``compute_We`` gives the energy the population holds.  Changing a parameter of the injection
    object after the first evaluation is not seen: build a new model."""
    kind = "cooled"
    _cached = ("_solved", "_w_dev", "_host_rows")

    def __init__(self, injection, B, age, seed_photon_fields=("CMB",), Emin=1 * u.GeV,
                 Emax=510.998 * u.TeV, n_per_decade=100):
        from .radiative import InverseCompton, _log_grid
        from .validator import validate_scalar
        validate_physical_type("B", B, "magnetic flux density")
        validate_physical_type("age", age, "time")
        for name, q in (("B", B), ("age", age)):
            if not q.on_device and np.ndim(q.value) > 1:
                raise TypeError("{0} should be a scalar or a 1-D batch over walkers".format(name))
        fields = seed_photon_fields
        if isinstance(fields, tuple):
            fields = list(fields)
        if type(fields) is list:
            for s in fields:
                if type(s) is list and len(s) in (3, 4) and isinstance(s[1], u.Quantity) \
                        and s[1].unit.physical_type != "temperature":
                    raise NotImplementedError(
                        "%s: cooling on monochromatic or tabulated photon fields is not "
                        "implemented; give thermal fields [name, T, u]" % s[0])
        seeds = InverseCompton._process_input_seed(fields) if fields else {}
        if len(seeds) > 8:
            raise ValueError("at most 8 photon fields, got %d" % len(seeds))
        for name, seed in seeds.items():
            if wv.per_walker(seed["T"]):
                raise NotImplementedError(
                    "%s-T must be the same for every walker of a batch (the loss table is "
                    "shared); evaluate walkers with different %s-T in separate calls"
                    % (name, name))
            if not float(seed["T"].to("K").value) > 0:
                raise ValueError("{0}-T value should be strictly positive".format(name))
        d = self.__dict__
        d["seed_photon_fields"] = seeds
        d["B"], d["age"] = B, age
        d["injection"] = injection
        # -- the injection and the solve grid --
        if isinstance(injection, (tuple, list)) and len(injection) == 2:
            e, r = injection
            e = _validate_ene(e)
            e_eV = np.atleast_1d(e.to("eV").value).astype(float).ravel()
            if not isinstance(r, u.Quantity):
                raise TypeError("injection rates should be given as a Quantity object")
            amp = u.Quantity(1.0, r.unit) * u.s
            if not r.on_device and np.shape(r.value)[-1:] != (e_eV.size,) \
                    or r.on_device and tuple(r.value.shape)[-1:] != (e_eV.size,):
                raise ValueError("injection rates need one value per energy (%d)" % e_eV.size)
            if np.any(~np.isfinite(e_eV)) or np.any(e_eV <= 0) or np.any(np.diff(e_eV) <= 0):
                raise ValueError("injection energies should be positive and ascending")
            d["_inj"] = "rows"
        else:
            lo = validate_scalar("Emin", Emin, domain="strictly-positive", physical_type="energy")
            hi = validate_scalar("Emax", Emax, domain="strictly-positive", physical_type="energy")
            e_eV = _log_grid(float(lo.to("eV").value), float(hi.to("eV").value), n_per_decade)
            if hasattr(injection, "device_rows"):
                amp = injection.amplitude
                if not isinstance(amp, u.Quantity):
                    raise TypeError("the injection amplitude should be given as a Quantity object")
                amp = amp * u.s
                d["_inj"] = "analytic"
            elif getattr(injection, "product", None) == "electron" and hasattr(injection, "flux"):
                amp = u.Quantity(1.0, "1/eV")
                d["_inj"] = "secondary"
            else:
                raise TypeError("injection should be an analytic particle distribution with an "
                                "amplitude in 1/(energy time), a SecondaryLeptonsKelner06 with "
                                "product='electron', or a pair (energies, rates)")
        validate_physical_type("injection amplitude x time", amp, "differential energy")
        if not 2 <= e_eV.size <= _COOL_MAX_NODES:
            raise ValueError("the solve grid has %d nodes; 2 .. %d are possible"
                             % (e_eV.size, _COOL_MAX_NODES))
        d["_e"] = e_eV
        d["amplitude"] = amp
        d["Emin"], d["Emax"], d["n_per_decade"] = Emin, Emax, n_per_decade
        inj_names = ["injection." + n for n in getattr(injection, "param_names", ())] \
            if d["_inj"] != "rows" else ["injection"]
        d["param_names"] = ["B", "age"] + inj_names + [n + "-u" for n in seeds]
        self.batch_size  # (raises on inconsistent batch sizes)
        if seeds:  # the loss table of these temperatures on this grid: built here, once, cached
            ctx = get_context()
            self._loss_table(ctx, ctx.const(e_eV))

    def __setattr__(self, name, value):
        # any parameter change invalidates the cached solves and weights
        for c in self._cached:
            self.__dict__.pop(c, None)
        object.__setattr__(self, name, value)

    # -- what is given per walker ------------------------------------------------------------
    def _own_values(self):
        return [self.B, self.age] + [s["u"] for s in self.seed_photon_fields.values()]

    def _rates(self):
        return self.injection[1] if self._inj == "rows" else None

    @property
    def energies(self):
        """the solve grid"""
        return u.Quantity(self._e.copy(), "eV")

    @property
    def on_device(self):
        if wv.on_device(self._own_values()):
            return True
        if self._inj == "rows":
            return self._rates().on_device
        return bool(getattr(self.injection, "on_device", False))

    @property
    def batch_size(self):
        if self._inj == "rows":  # (rates of shape (N, nC): the walkers on the leading axis)
            sh = tuple(self._rates().value.shape)
            inj = sh[0] if len(sh) == 2 else 1
        else:
            inj = self.injection.batch_size
        return wv.merge(wv.counts(self._own_values()) + [inj], "CooledElectrons")

    @property
    def is_batched(self):
        if wv.is_batched(self._own_values()):
            return True
        if self._inj == "rows":
            return len(tuple(self._rates().value.shape)) == 2
        return bool(self.injection.is_batched)

    def _walker(self, k):
        """this model for walker k alone (host values)"""
        def one(q):
            return q[k] if wv.per_walker(q) else q
        inj = self.injection
        if self._inj == "rows":
            r = self._rates()
            inj = (inj[0], r[k] if np.ndim(r.value) == 2 else r)
        elif inj.is_batched:
            import copy
            src, inj = inj, copy.copy(inj)
            inj.__dict__ = {a: b for a, b in src.__dict__.items() if not a.startswith("_")}
            pd = getattr(inj, "particle_distribution", None)
            if pd is not None:
                pd2 = copy.copy(pd)
                pd2.__dict__ = {a: b for a, b in pd.__dict__.items() if not a.startswith("_")}
                inj.__dict__["particle_distribution"] = pd = pd2
            for obj in (inj, pd):
                for name in getattr(obj, "param_names", ()) if obj is not None else ():
                    v = getattr(obj, name, None)
                    if isinstance(v, u.Quantity) and np.ndim(v.value) > 0 or \
                            not isinstance(v, (u.Quantity, str)) and np.ndim(v) > 0:
                        obj.__dict__[name] = v[k]
        fields = [[n, s["T"], one(s["u"])] for n, s in self.seed_photon_fields.items()]
        return CooledElectrons(inj, one(self.B), one(self.age), fields, self.Emin, self.Emax,
                               self.n_per_decade)

    # -- the loss table ----------------------------------------------------------------------
    def _loss_table(self, ctx, ed):
        """loss[nf][nC] in HBM (eV/s per erg/cm3 of each field at every node of the solve grid),
        built once per (temperatures, grid) and cached like the emission tables: the project's IC
        emissivity on a Planck field (the isotropic kernel of nh_table_ic_planck, by
        nh_cooled_ic_rows on a row of outgoing photon energies per node: two launches per field),
        reduced with the energy weight (nh_trapz_loglog_comps)"""
        import ctypes as C

        from . import _lib
        from .darray import TF_SQUARE, nh_comp, nh_lazy
        Ts = tuple(float(s["T"].to("K").value) for s in self.seed_photon_fields.values())
        if not Ts:
            return None
        e_eV, nC = self._e, self._e.size

        def build():
            gam = e_eV / MEC2_EV
            gd = ctx.const(gam)
            out = ctx.empty((len(Ts), nC))
            for f, T in enumerate(Ts):
                z = _cool_zgrid(4.0 * gam[0] * T * _K_TO_MEC2)
                nE = z.size
                zd = ctx.const(z)
                Kt = ctx.empty((nC, nE))
                # (a table build, not a step-loop launch: called directly, never recorded)
                _lib._chk(_lib._lib.nh_cooled_ic_rows(ctx.h, gd.ptr, nC, zd.ptr, nE, T, Kt.ptr, nE))
                comp = (nh_comp * 1)(nh_comp(Kt.ptr, nE, _cool_loss_scale(T)))
                g2 = nh_lazy(gd.ptr, 1, 1.0, 1.0, 0.0, TF_SQUARE, 0)  # E_ph = gamma z: gamma^2
                _lib._chk(_lib._lib.nh_trapz_loglog_comps(
                    ctx.h, comp, 1, zd.ptr, C.addressof(g2), zd.ptr, nC, nE,
                    out.ptr + 8 * f * nC, 1))
                ctx.sync()  # (Kt goes back to the pool when this scope ends)
                del Kt
            return out, gd, ed

        return ctx.table(("cool-loss", ed.ptr) + Ts, build)[0]

    # -- the solve ---------------------------------------------------------------------------
    def _injection_rows(self, ctx, ed):
        """(owner, pointer, ldq, rows) of Q[rows][nC] in 1/(eV s) on the solve grid"""
        nC = self._e.size
        if self._inj == "analytic":
            inj = self.injection
            Ni = inj.batch_size
            rows = inj.device_rows(ctx, Ni, amplitude_to=u.Unit("1/(eV s)"))
            w, lw, q = ctx.empty((Ni, nC)), ctx.empty((Ni, nC)), ctx.empty((Ni, nC))
            ctx.call("nh_particle_weights", PD_KIND[inj.kind], rows, Ni, ed, ed, nC, 1.0, w, lw, q)
            return q, q.ptr, nC if Ni > 1 else 0, Ni
        if self._inj == "secondary":
            r = self.injection.flux(u.Quantity(self._e, "eV"), distance=0)
        else:
            r = self._rates()
        v = r.to("1/(eV s)").value
        if r.on_device:  # (a device matrix: its dense [N][nC] form, one launch unless it is that)
            own, ptr = v.buffer()
            return own, ptr, nC if v.shape[0] > 1 else 0, v.shape[0]
        v = np.ascontiguousarray(np.atleast_2d(np.asarray(v, dtype=float)))
        own = ctx.array(v)
        return own, own.ptr, nC if v.shape[0] > 1 else 0, v.shape[0]

    def _solve(self, ctx, N=None):
        """n[N][nC] (1/eV) in HBM: one nh_cooled_electrons launch per parameter state"""
        import ctypes as C

        from .darray import nh_lazy
        N = self.batch_size if N is None else N
        cache = self.__dict__.setdefault("_solved", {})
        hit = cache.get(N)
        if hit is not None:
            return hit
        nC = self._e.size
        ed = ctx.const(self._e)
        seeds = list(self.seed_photon_fields.values())
        # (uploaded as given, the unit folded in: a host batch gives a device batch's bits)
        args = dict(N=N, fold=True, mismatch="a per-walker value has %d walkers, the batch has %d")
        Bl, keep_B = wv.lazy(ctx, self.B, "G", **args)
        agel, keep_age = wv.lazy(ctx, self.age, "s", **args)
        ul, keep_u = (nh_lazy * max(len(seeds), 1))(), []
        for f, s in enumerate(seeds):
            ul[f], k = wv.lazy(ctx, s["u"], "erg/cm3", **args)
            keep_u.append(k)
        loss = self._loss_table(ctx, ed)
        own, qptr, ldq, nrows = self._injection_rows(ctx, ed)
        if ldq and nrows != N:
            raise ValueError("the injection has %d rows, the batch has %d" % (nrows, N))
        out = ctx.empty((N, nC))
        ctx.call("nh_cooled_electrons", qptr, ldq, N, ed, nC, C.addressof(Bl),
                 loss.ptr if loss is not None else None, len(seeds), ul, C.addressof(agel), out,
                 cool_status(ctx))
        del own, keep_B, keep_age, keep_u
        cache[N] = out
        return out

    def _resample(self, ctx, n, N, e_eV, xg, unit_scale):
        """(w, dlw) on a target grid: one nh_cooled_weights launch"""
        nG = e_eV.size
        w, lw = ctx.empty((N, nG)), ctx.empty((N, nG))
        ctx.call("nh_cooled_weights", n, ctx.const(self._e), self._e.size, N, ctx.const(e_eV),
                 ctx.const(xg), nG, float(unit_scale), w, lw)
        return w, lw

    def __call__(self, e):
        """dN/dE in 1/eV at energies ``e`` -- (n_e,), (N, n_e), or a device matrix when a
        parameter lives on the device; zero outside the solve grid"""
        from .darray import DMat
        e = _validate_ene(e)
        e_eV = np.atleast_1d(e.to("eV").value).astype(float).ravel()
        ctx = get_context()
        N = self.batch_size
        w, _ = self._resample(ctx, self._solve(ctx), N, e_eV, np.ones(e_eV.size), 1.0)
        if self.on_device:
            return u.Quantity(DMat.from_buffer(ctx, w, N, e_eV.size), "1/eV")
        out = w.get()
        if e.isscalar:
            out = out[:, 0]
        return u.Quantity(out if self.is_batched else out[0], "1/eV")

    # -- host views: cooling time and break energy -------------------------------------------
    def _host_b(self):
        """(b[N][nC] in eV/s on the solve grid, age[N] in s), from downloaded values"""
        hit = self.__dict__.get("_host_rows")
        if hit is None:
            ctx = get_context()
            N = self.batch_size

            def host(q, unit):
                return np.broadcast_to(np.asarray(q.to(unit).value, dtype=float), (N,))
            B = host(self.B, "G")
            b = _COOL_SYN * (B * B)[:, None] * (self._e * self._e)[None, :]
            seeds = list(self.seed_photon_fields.values())
            if seeds:
                loss = self._loss_table(ctx, ctx.const(self._e)).get()
                for f, s in enumerate(seeds):
                    b = b + host(s["u"], "erg/cm3")[:, None] * loss[f][None, :]
            hit = self.__dict__["_host_rows"] = (b, host(self.age, "s"))
        return hit

    def cooling_time(self, e):
        """gamma / |dgamma/dt| in seconds at energies ``e``: (n_e,) or (N, n_e); the loss rate is
        interpolated log-log between the nodes of the solve grid and NaN outside it"""
        e = _validate_ene(e)
        x = np.log(np.atleast_1d(e.to("eV").value).astype(float).ravel())
        b, _ = self._host_b()
        lg = np.log(self._e)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.stack([np.exp(x - np.interp(x, lg, np.log(row), left=np.nan, right=np.nan))
                            for row in b])
        if e.isscalar:
            out = out[:, 0]
        return u.Quantity(out if self.is_batched else out[0], "s")

    def break_energy(self):
        """the energy at which the cooling time equals the age, per walker (bisection in ln E on
        the downloaded loss rows); NaN where the two do not meet inside the solve grid"""
        b, age = self._host_b()
        lg = np.log(self._e)
        with np.errstate(divide="ignore", invalid="ignore"):
            lt = lg[None, :] - np.log(b)  # ln of the cooling time at the nodes
            la = np.log(age)
        out = np.full(b.shape[0], np.nan)
        for k in range(b.shape[0]):
            f = lambda x: np.interp(x, lg, lt[k]) - la[k]  # noqa: E731
            lo, hi = lg[0], lg[-1]
            if not (np.isfinite(la[k]) and f(lo) * f(hi) <= 0):
                continue
            flo = f(lo)
            for _ in range(100):
                mid = 0.5 * (lo + hi)
                if f(mid) * flo > 0:
                    lo = mid
                else:
                    hi = mid
            out[k] = np.exp(0.5 * (lo + hi))
        return u.Quantity(out if self.is_batched else out[0], "eV")


def cool_status_read(ctx, reset=True):
    """NaN rows that nh_cooled_electrons has given out-of-domain walkers on this context since
    the last reset (synchronises; not while a graph is captured)"""
    st = cool_status(ctx)
    n = int(st.get()[0])
    if reset and n:
        st.set(np.zeros(1, dtype=np.int32))
    return n


def cool_status(ctx):
    """the device int nh_cooled_electrons counts NaN rows in (one per context; it only grows
    until cool_status_read resets it)"""
    st = getattr(ctx, "_cool_status", None)
    if st is None:
        st = ctx._cool_status = ctx.array(np.zeros(1, dtype=np.int32), dtype=np.int32)
    return st
