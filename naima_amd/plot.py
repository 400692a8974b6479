"""naima's plotting API (plot.py:273-702 and the figures around it, reference) and the
computation under it.

The confidence bands are exact order statistics per energy, ``np.sort(model[:, i])[nf]``
with naima's rule for ``nf``, taken on the GPU by ``nh_column_select`` -- over every stored
(step, walker) spectrum of the chain's blobs, or over model evaluations at parameter vectors
drawn from the chain when ``e_range`` is given.  Those draws are ONE batched call of the
model function on device parameters (``DPars``): the [n_samples][e_npoints] matrix of spectra
never leaves HBM, only the bands come back.  There is no CPU fallback for the selection.

matplotlib is imported by the plotting functions only: ``import naima_amd.plot`` and the
compute functions (``_calc_CI``, ``_calc_ML``, ``find_ML``, ``_read_or_calc_samples``) work
without it.

On a sampler that spans several ranks every function here reads ``get_chain`` /
``get_blobs`` and is therefore COLLECTIVE: call it on every rank.  Model evaluations stay local
to the rank that calls.
"""
import numpy as np

from . import units as u
from .core import sed_conversion
from .dview import DeviceMatrix, as_matrix, matrix_on
from .validator import validate_array

__all__ = ["plot_chain", "plot_fit", "plot_data", "plot_blob", "plot_corner"]

marker_cycle = ["o", "s", "d", "p", "*"]
# (seaborn's "deep" palette, as the reference uses)
color_cycle = [(0.298, 0.447, 0.690), (0.333, 0.659, 0.408), (0.769, 0.306, 0.322),
               (0.506, 0.447, 0.698), (0.800, 0.725, 0.455), (0.392, 0.710, 0.804)]

_EVAL_BATCH = 8192  # parameter vectors per model call when drawing band samples


# ---------------------------------------------------------------------------------------
# samples: stored blobs or fresh evaluations
# ---------------------------------------------------------------------------------------
def _blob_history(sampler, modelidx):
    blobs = sampler.get_blobs()
    if blobs is None or modelidx >= len(blobs):
        raise TypeError("Model {0} has wrong blob format".format(modelidx))
    units = list(getattr(sampler, "blob_units", None) or [None] * len(blobs))
    return np.asarray(blobs[modelidx], dtype=float), units[modelidx]


def _process_blob(sampler, modelidx, last_step=False):
    """(modelx, model) of stored blob ``modelidx``: model [n][m] over every (step, walker) of the
    chain (the last step only with ``last_step``).  A blob of len(data['energy']) values per
    walker is a spectrum at the data's energies (modelx = data['energy']); a scalar blob gives
    modelx = None and model [n].  (plot.py:273-343; the history is dense here, [nsteps][nwalkers]
    [m], with the blob's unit in ``sampler.blob_units``.)"""
    b, unit = _blob_history(sampler, modelidx)
    if b.ndim == 2:
        modelx = None
        model = b[-1] if last_step else b.reshape(-1)
    elif b.ndim == 3 and b.shape[2] == np.size(sampler.data["energy"].value):
        modelx = sampler.data["energy"]
        model = b[-1] if last_step else b.reshape(-1, b.shape[2])
    else:
        raise TypeError("Model {0} has wrong blob format".format(modelidx))
    return modelx, u.Quantity(model, unit)


def _energy_grid(sampler, e_range, e_npoints):
    """the log-spaced energies and zero-flux data table of an ``e_range`` evaluation
    (plot.py:368-373)"""
    if getattr(sampler, "modelfn", None) is None:
        raise ValueError("e_range needs the model function, and this sampler has none: pass "
                         "modelfn= to read_run() to recompute a saved run's model")
    e_range = validate_array("e_range", u.Quantity(e_range), physical_type="energy",
                             shape=(2,))
    e_unit = e_range.unit
    lo, hi = (float(v) for v in e_range.value)
    if not (lo > 0 and hi > 0):
        raise ValueError("e_range must be two positive energies")
    energy = u.Quantity(np.logspace(np.log10(lo), np.log10(hi), int(e_npoints)), e_unit)
    data = {"energy": energy,
            "flux": u.Quantity(np.zeros(energy.shape), sampler.data["flux"].unit)}
    return energy, data


def _draw(sampler, n_samples, last_step, seed):
    """the parameter vectors of an ``e_range`` evaluation: np.random.randint over the chain
    (plot.py:376-377); ``seed`` draws from RandomState(seed), the stream np.random.seed(seed)
    would give the global functions"""
    chain = sampler.get_chain()[-1] if last_step else sampler.get_chain(flat=True)
    rs = np.random if seed is None else np.random.RandomState(seed)
    return chain[rs.randint(len(chain), size=int(n_samples))]


def _pick(modelout, modelidx):
    """output ``modelidx`` of a model function: a bare output is output 0 (plot.py:387-390 wraps
    it as [modelout]), there is no other"""
    outs = modelout if isinstance(modelout, (tuple, list)) else [modelout]
    if not 0 <= modelidx < len(outs):
        raise IndexError("the model function returns {0} output(s): there is no model {1}"
                         .format(len(outs), modelidx))
    return outs[modelidx]


def _split_model(blob, energy, modelidx):
    """a model output -> (modelx, flux Quantity): a Quantity is a spectrum at ``energy``, a
    pair (energies, flux) a spectrum at its own energies"""
    if isinstance(blob, u.Quantity):
        return energy, blob
    if isinstance(blob, (tuple, list)) and len(blob) == 2 and \
            isinstance(blob[0], u.Quantity) and isinstance(blob[1], u.Quantity):
        return blob[0], blob[1]
    raise TypeError("Model {0} has wrong blob format".format(modelidx))


def _evaluate_device(ctx, sampler, pars, data, modelidx):
    """one model call on device parameters -> (modelx, unit, DeviceMatrix), or None when the model
    cannot take them (what EnsembleSampler._probe_device catches)"""
    from .darray import DFactor, DMat, DPars, lift_factor
    n = len(pars)
    try:
        out = sampler.modelfn(DPars(ctx, ctx.array(np.ascontiguousarray(pars.T)), pars.shape[1], n),
                              data)
        modelx, q = _split_model(_pick(out, modelidx), data["energy"], modelidx)
        v = lift_factor(q.value, n)
        if isinstance(v, DFactor):  # (a transmission blob)
            q = q.__class__(v.apply(), q.unit)
        if not isinstance(q.value, DMat):
            raise TypeError("a host array for device parameters")
        d = q.value.dense()
    except (NotImplementedError, TypeError, ValueError):
        ctx.flush()
        return None
    _check_shape(d.shape, n, modelx, modelidx)
    buf, ptr = d.buffer()
    return modelx, q.unit, DeviceMatrix(ctx, ptr, n, d.shape[1], d.shape[1], buf)


def _check_shape(shape, n, modelx, modelidx):
    """a batch of n draws must give n spectra of len(modelx) values each: anything else (one
    spectrum for the whole batch, parameters broadcast along the energies) is a wrong blob"""
    if tuple(shape) != (n, np.size(modelx.value)):
        raise TypeError("Model {0} has wrong blob format: {1} draws gave an output of shape {2}"
                        .format(modelidx, n, tuple(shape)))


def _evaluate_host(ctx, sampler, pars, data, modelidx):
    """the draws as one host-parameter batch (models that shape a grid per walker)"""
    out = sampler.modelfn(np.ascontiguousarray(pars.T), data)
    modelx, q = _split_model(_pick(out, modelidx), data["energy"], modelidx)
    v = np.asarray(q.value, dtype=float)
    _check_shape(v.shape, len(pars), modelx, modelidx)
    return modelx, q.unit, as_matrix(v)


def _samples_on_device(sampler, modelidx=0, n_samples=100, last_step=False, e_range=None,
                       e_npoints=100, seed=None, batch=None):
    """(modelx, unit, DeviceMatrix): the stored blob history uploaded once, or ``n_samples``
    fresh model evaluations at parameters drawn from the chain, on the device"""
    from . import _lib
    if e_range is None:
        modelx, model = _process_blob(sampler, modelidx, last_step=last_step)
        return modelx, model.unit, as_matrix(model.value)
    _, data = _energy_grid(sampler, e_range, e_npoints)
    pars = _draw(sampler, n_samples, last_step, seed)
    ctx = _lib.get_context()
    batch = int(batch or _EVAL_BATCH)
    if len(pars) <= batch:
        return _evaluate(ctx, sampler, pars, data, modelidx)
    # more draws than one model call takes: chunks of ``batch`` draws, each copied into one
    # device buffer as soon as it is evaluated (stream-ordered) and then released
    whole = modelx = unit = None
    for a in range(0, len(pars), batch):
        mx, un, s = _evaluate(ctx, sampler, pars[a:a + batch], data, modelidx)
        if whole is None:
            modelx, unit = mx, un
            whole = matrix_on(ctx.empty((len(pars), s.ncol)), len(pars), s.ncol)
        elif un != unit or s.ncol != whole.ncol:
            raise TypeError("Model {0} has wrong blob format: chunks of draws differ in unit or "
                            "length".format(modelidx))
        ctx.call("nh_copy", whole.rows(a, a + s.M).ptr, s.ptr, 8 * s.M * s.ncol)
        del s
    return modelx, unit, whole


def _evaluate(ctx, sampler, pars, data, modelidx):
    """the draws on device parameters, or as one host-parameter batch when the model cannot take
    those (a grid-shaping parameter per walker and the like)"""
    got = _evaluate_device(ctx, sampler, pars, data, modelidx)
    return got if got is not None else _evaluate_host(ctx, sampler, pars, data, modelidx)


def _read_or_calc_samples(sampler, modelidx=0, n_samples=100, last_step=False, e_range=None,
                          e_npoints=100, threads=None, seed=None):
    """(modelx, model): the stored blobs, or ``n_samples`` model evaluations at parameters drawn
    from the chain on an ``e_range`` grid (plot.py:346-393; ``threads`` is accepted and
    ignored: the draws are one batched evaluation on the GPU)"""
    if e_range is None:
        return _process_blob(sampler, modelidx, last_step=last_step)
    modelx, unit, s = _samples_on_device(sampler, modelidx, n_samples, last_step, e_range,
                                         e_npoints, seed)
    return modelx, u.Quantity(s.get(), unit)


def column_select(samples, ranks):
    """out[r][c] = np.sort(samples[:, c])[ranks[r]] by nh_column_select (16 ranks per launch);
    ``samples`` is a DeviceMatrix or a host array [M][m]"""
    import ctypes as C
    samples = as_matrix(samples)
    ctx = samples.ctx
    ranks = [int(r) for r in ranks]
    out = np.empty((len(ranks), samples.ncol))
    for a in range(0, len(ranks), 16):
        rk = ranks[a:a + 16]
        arr = (C.c_int * len(rk))(*rk)
        dev = ctx.empty((len(rk), samples.ncol))
        ctx.call("nh_column_select", samples.ptr, samples.M, samples.ncol, samples.ld, arr,
                 len(rk), dev.ptr)
        out[a:a + len(rk)] = dev.get()
    return out


def _band_ranks(nsamples, confs):
    """naima's rank rule (plot.py:484-496): with nwalkers = len(model) - 1, the band of
    ``conf`` sigma is sample int(norm.cdf(-conf) * nwalkers) .. int(norm.cdf(conf) * nwalkers)"""
    from scipy import stats
    nwalkers = nsamples - 1
    ranks = []
    for conf in confs:
        for fr in (stats.norm.cdf(-conf), stats.norm.cdf(conf)):
            ranks.append(int(fr * nwalkers))
    return ranks


def _min_samples(confs):
    """n_samples of an e_range band: min(100, int(1 / norm.cdf(-max(confs)) + 1)) (plot.py:460)"""
    from scipy import stats
    return min(100, int(1 / stats.norm.cdf(-np.max(confs)) + 1))


def _calc_CI(sampler, modelidx=0, confs=[3, 1], last_step=False, e_range=None, e_npoints=100,
             threads=None, n_samples=None, seed=None):
    """(modelx, [(ymin, ymax) per conf]): the confidence bands of model ``modelidx``
    (plot.py:438-501), exact order statistics taken on the GPU.  With ``e_range`` the model is
    evaluated at ``n_samples`` parameter vectors drawn from the chain (default: naima's
    min(100, ...) rule; an integer overrides it without a cap).  Collective on several ranks."""
    if e_range is not None and n_samples is None:
        n_samples = _min_samples(confs)
    modelx, unit, s = _samples_on_device(sampler, modelidx, n_samples, last_step, e_range,
                                         e_npoints, seed)
    vals = column_select(s, _band_ranks(s.M, confs))
    CI = []
    for j in range(len(confs)):
        lo, hi = vals[2 * j], vals[2 * j + 1]
        if modelx is None:
            lo, hi = lo[0], hi[0]
        CI.append((u.Quantity(lo, unit), u.Quantity(hi, unit)))
    return modelx, CI


def find_ML(sampler, modelidx):
    """(ML, MLp, MLerr, (modelx, model_ML)): the chain's most probable sample, the half width of
    each parameter's 16-84 percentile range, and its stored model (plot.py:667-702).  (The
    package-level ``naima_amd.find_ML`` is analysis-time's (ML, MLp).)"""
    lnprobability = np.asarray(sampler.get_log_prob())
    index = np.unravel_index(np.argmax(lnprobability), lnprobability.shape)
    MLp = np.asarray(sampler.get_chain())[index]
    blobs = sampler.get_blobs()
    if modelidx is not None and blobs is not None:
        b, unit = _blob_history(sampler, modelidx)
        v = b[index]
        if np.ndim(v) == 1 and np.size(v) == np.size(sampler.data["energy"].value):
            modelx, model_ML = sampler.data["energy"].copy(), u.Quantity(v.copy(), unit)
        elif np.ndim(v) == 0:
            modelx, model_ML = None, u.Quantity(float(v), unit)
        else:
            raise TypeError("Model {0} has wrong blob format".format(modelidx))
    elif modelidx is not None and getattr(sampler, "modelfn", None) is not None:
        out = _pick(sampler.modelfn(MLp, sampler.data), modelidx)
        modelx, model_ML = _split_model(out, sampler.data["energy"], modelidx)
    else:
        modelx, model_ML = None, None
    MLerr = []
    for dist in np.asarray(sampler.get_chain(flat=True)).T:
        hilo = np.percentile(dist, [16.0, 84.0])
        MLerr.append((hilo[1] - hilo[0]) / 2.0)
    ML = lnprobability[index]
    return ML, MLp, MLerr, (modelx, model_ML)


def _calc_ML(sampler, modelidx=0, e_range=None, e_npoints=100):
    """find_ML, with the model recomputed on an ``e_range`` grid when one is given
    (plot.py:396-436)"""
    ML, MLp, MLerr, ML_model = find_ML(sampler, modelidx)
    if e_range is not None:
        energy, data = _energy_grid(sampler, e_range, e_npoints)
        modelx, model = _split_model(_pick(sampler.modelfn(MLp, data), modelidx), energy,
                                     modelidx)
        ML_model = (modelx.copy(), u.Quantity(np.asarray(model.value, dtype=float).copy(),
                                              model.unit))
    return ML, MLp, MLerr, ML_model


# ---------------------------------------------------------------------------------------
# figures (matplotlib imported inside)
# ---------------------------------------------------------------------------------------
def _unit_label(unit):
    return unit.name if hasattr(unit, "name") else str(unit)


def _tex_number(x, digits=3):
    """x with ``digits`` significant digits, a power of ten written out in TeX"""
    mant, _, exp = "{0:.{1}g}".format(x, digits).partition("e")
    return mant if not exp else r"%s\times 10^{%d}" % (mant, int(exp))


def _value_error(val, elo, ehi):
    """"$v^{+hi}_{-lo}$" with two significant digits on the errors; values beyond 1e-2 .. 1e3 in
    units of their power of ten"""
    order = int(np.floor(np.log10(abs(val)))) if val != 0 and np.isfinite(val) else 0
    if -2 <= order <= 2:
        order = 0
    val, elo, ehi = (x / 10.0 ** order for x in (val, elo, ehi))

    def sig(x):
        return 1 - int(np.floor(np.log10(abs(x)))) if x > 0 and np.isfinite(x) else 2
    n = max(sig(elo), sig(ehi), 0)
    body = r"{0:.{n}f}^{{+{1:.{n}f}}}_{{-{2:.{n}f}}}".format(val, ehi, elo, n=n)
    return "$%s$" % (body if order == 0 else r"(%s)\times 10^{%d}" % (body, order))


def _posterior_hist(ax, dist, label, title):
    """density histogram of ``dist`` with its KDE, median and 16-84 % band; returns the three
    percentiles.  The bar heights and the KDE curve come from the GPU (posterior.histogram,
    posterior.gaussian_kde) over one upload of ``dist``."""
    from . import posterior
    nbins = int(np.clip(np.sqrt(dist.size), 25, 100))
    s = as_matrix(dist)
    counts, edges = posterior.histogram(s, bins=nbins)
    counts, edges = counts[0], edges[0]
    heights = counts / (counts.sum() * np.diff(edges))  # (np.histogram's density=True)
    ax.stairs(heights, edges, fill=True, color=color_cycle[0], lw=0)
    if np.ptp(dist) > 0:
        ax.plot(edges, posterior.gaussian_kde(s, edges)[0], color="k", label="KDE")
    q = np.percentile(dist, [16, 50, 84])
    ax.axvspan(q[0], q[2], color="0.5", alpha=0.25, lw=0, label="68% CI")
    ax.axvline(q[1], color="k", ls="--", lw=2, alpha=0.5, label="50% quantile")
    ax.tick_params(axis="x", labelrotation=45)
    ax.set(xlabel=label, title=title, ylim=(0, 1.05 * heights.max()))
    return tuple(q)


def _chain_text(sampler, label, dist, shape, last_step, tau=None, rhat=None):
    """the summary printed beside a chain plot: run size, the parameter's integrated
    autocorrelation time ``tau`` (left out when None: naima leaves it out for a chain too short to
    estimate it), acceptance, and the posterior's median with 16/84 % errors (de-logged too for a
    log10( ) / log( ) label)."""
    q16, q50, q84 = np.percentile(dist, [16, 50, 84])
    lines = ["Walkers: %d" % shape[0], "Steps in chain: %d" % shape[1]]
    if tau is not None:
        lines.append("Autocorrelation time: %.1f" % tau)
    if rhat is not None:  # (a run of several independent ensembles)
        lines.append("Gelman-Rubin R-hat: %.3f" % rhat)
    lines += ["Mean acceptance fraction: %.3f" % np.mean(sampler.acceptance_fraction),
             "Distribution properties for the %s:" % ("last ensemble" if last_step
                                                      else "whole chain"),
             "    $-$ median: $%s$, std: $%s$" % (_tex_number(q50), _tex_number(np.std(dist))),
             "    $-$ median, 16th / 84th percentile errors:",
             "          %s = %s" % (label, _value_error(q50, q50 - q16, q84 - q50))]
    kind, _, rest = label.partition("(")
    if rest and kind in ("log10", "log"):
        lin = 10 ** dist if kind == "log10" else np.exp(dist)
        l16, l50, l84 = np.percentile(lin, [16, 50, 84])
        lines.append("          %s = %s" % (rest.split(")")[0].rjust(len(label)),
                                            _value_error(l50, l50 - l16, l84 - l50)))
    return "\n".join(lines)


def _chain_rhat(sampler):
    """Gelman-Rubin R-hat of every parameter of a run of several independent ensembles (a sampler,
    or a ``read_run`` result through ``run_info["ensembles"]``), else None; also None for a chain
    of fewer than four rows (split R-hat: two per half)"""
    k = int(getattr(sampler, "run_info", {}).get("ensembles", getattr(sampler, "ensembles", 1)))
    chain = np.asarray(sampler.get_chain())
    if k < 2 or chain.shape[0] < 4:
        return None
    from .posterior import rhat
    return rhat(chain, k)


def _plot_chain_func(sampler, p, last_step=False, rhat=None):
    """one parameter: walker traces (top left), posterior (right), summary (bottom left);
    ``rhat``: what ``_chain_rhat`` gave for the sampler"""
    import matplotlib.pyplot as plt
    from .autocorr import AutocorrError, integrated_time
    chain = np.asarray(sampler.get_chain())
    traces = chain[:, :, p].T  # (walker, step)
    try:  # (plot.py:202-209: on the chain, so that read_run results get the line too)
        # in ensemble steps: a run thinned as it was made (run_sampler(thin_by=)) stores a row
        # every thin_by steps
        tau = integrated_time(chain)[p] * getattr(sampler, "run_info", {}).get("thin_by", 1)
    except AutocorrError:  # too short a chain for a meaningful estimate
        tau = None
    label = sampler.labels[p]
    dist = traces[:, -1] if last_step else traces.ravel()
    fig = plt.figure()
    grid = fig.add_gridspec(2, 2, left=0.1, bottom=0.15, right=0.95, top=0.9, wspace=0.3)
    ax_tr, ax_post = fig.add_subplot(grid[0, 0]), fig.add_subplot(grid[:, 1])
    # every trace in light grey, a handful (5 %, never fewer than three) highlighted on top
    nhi = min(len(traces), max(3, int(np.ceil(0.05 * len(traces)))))
    steps = np.arange(traces.shape[1])
    for k, t in enumerate(traces):
        hi = k >= len(traces) - nhi
        ax_tr.plot(steps, t, lw=1.5 if hi else 1.0, alpha=0.75 if hi else 0.25,
                   color=color_cycle[0] if hi else "0.1", rasterized=not hi)
    ax_tr.set(xlabel="step number", ylabel=label, title="Walker traces")
    _posterior_hist(ax_post, dist, label, "posterior distribution")
    fig.text(0.05, 0.45, _chain_text(sampler, label, dist, traces.shape, last_step, tau,
                                     None if rhat is None else rhat[p]),
             ha="left", va="top")
    return fig


def plot_chain(sampler, p=None, **kwargs):
    """Diagnostic figure of parameter ``p``'s walker traces and posterior (all parameters, one
    figure each, when ``p`` is None: returns None then).  plot.py:26-52."""
    rhat = _chain_rhat(sampler)  # (once for all the figures)
    if p is None:
        for pp in range(np.asarray(sampler.get_chain()).shape[-1]):
            _plot_chain_func(sampler, pp, rhat=rhat, **kwargs)
        return None
    return _plot_chain_func(sampler, p, rhat=rhat, **kwargs)


def _plot_MLmodel(ax, sampler, modelidx, e_range, e_npoints, e_unit, sed):
    _, _, _, (mx, my) = _calc_ML(sampler, modelidx, e_range=e_range, e_npoints=e_npoints)
    f_unit, sedf = sed_conversion(mx, my.unit, sed)
    ax.loglog(mx.to(e_unit).value, (my * sedf).to(f_unit).value, color="k", lw=2, alpha=0.8)


def plot_CI(ax, sampler, modelidx=0, sed=True, confs=[3, 1, 0.5], e_unit=u.eV, label=None,
            e_range=None, e_npoints=100, threads=None, last_step=False, n_samples=None,
            seed=None):
    """Confidence bands of model ``modelidx`` on ``ax``, widest first, with the ML model on top
    (plot.py:518-588).  ``confs`` is not modified."""
    confs = sorted(confs, reverse=True)
    modelx, CI = _calc_CI(sampler, modelidx=modelidx, confs=confs, e_range=e_range,
                          e_npoints=e_npoints, last_step=last_step, n_samples=n_samples,
                          seed=seed)
    f_unit, sedf = sed_conversion(modelx, CI[0][0].unit, sed)
    for (ymin, ymax), conf in zip(CI, confs):
        grey = np.log(conf) / np.log(20) + 0.4
        ax.fill_between(modelx.to(e_unit).value, (ymax * sedf).to(f_unit).value,
                        (ymin * sedf).to(f_unit).value, lw=0.001, color=(grey,) * 3, alpha=0.6,
                        zorder=-10)
    _plot_MLmodel(ax, sampler, modelidx, e_range, e_npoints, e_unit, sed)
    if label is not None:
        ax.set_ylabel("{0} [{1}]".format(label, _unit_label(f_unit)))


def plot_samples(ax, sampler, modelidx=0, sed=True, n_samples=100, e_unit=u.eV, e_range=None,
                 e_npoints=100, threads=None, label=None, last_step=False, seed=None):
    """``n_samples`` model spectra drawn from the chain on ``ax``, with the ML model on top
    (plot.py:591-664)."""
    modelx, model = _read_or_calc_samples(sampler, modelidx, last_step=last_step,
                                          e_range=e_range, e_npoints=e_npoints, seed=seed)
    f_unit, sedf = sed_conversion(modelx, model.unit, sed)
    alpha = min(5.0 / n_samples, 0.5)
    rs = np.random if seed is None else np.random.RandomState(seed)
    vals = np.asarray(model.value)
    for my in vals[rs.randint(len(vals), size=n_samples)]:
        ax.loglog(modelx.to(e_unit).value, (u.Quantity(my, model.unit) * sedf).to(f_unit).value,
                  color=(0.1,) * 3, alpha=alpha, lw=1.0)
    _plot_MLmodel(ax, sampler, modelidx, e_range, e_npoints, e_unit, sed)
    if label is not None:
        ax.set_ylabel("{0} [{1}]".format(label, _unit_label(f_unit)))


def plot_distribution(samples, label, figure=None):
    """Histogram, KDE and 16/50/84 percentiles of a scalar blob's samples (plot.py:1303-1390)."""
    import matplotlib.pyplot as plt
    samples = u.Quantity(samples)
    dist = np.asarray(samples.value, dtype=float).ravel()
    un = samples.unit
    xlabel = label if un is None or un == u.dimensionless_unscaled else \
        "{0} [{1}]".format(label, _unit_label(un))
    f = plt.figure() if figure is None else figure
    ax = f.add_subplot(111)
    _posterior_hist(ax, dist, xlabel, "Posterior distribution of {0}".format(label))
    return f


def plot_blob(sampler, blobidx=0, label=None, last_step=False, figure=None, **kwargs):
    """Blob ``blobidx`` as a fit to the data (a spectrum; extra keywords go to plot_fit) or as
    the distribution of its values (a scalar) (plot.py:705-760)."""
    modelx, model = _process_blob(sampler, blobidx, last_step)
    if label is None:
        label = "Model output {0}".format(blobidx)
    if modelx is None:
        return plot_distribution(model, label, figure=figure)
    for k in ("n_samples", "confs"):
        kwargs.setdefault(k, None if k == "confs" else 100)
    return plot_fit(sampler, modelidx=blobidx, last_step=last_step, label=label, figure=figure,
                    **kwargs)


def plot_fit(sampler, modelidx=0, label=None, sed=True, last_step=False, n_samples=100,
             confs=None, ML_info=False, figure=None, plotdata=None, plotresiduals=None,
             e_unit=None, e_range=None, e_npoints=100, threads=None, xlabel=None, ylabel=None,
             ulim_opts={}, errorbar_opts={}, seed=None):
    """Data with the model's confidence bands (``confs``) or ``n_samples`` sample spectra, the ML
    model and the residuals against it (plot.py:763-993)."""
    import matplotlib.pyplot as plt
    ML, MLp, MLerr, model_ML = find_ML(sampler, modelidx)
    infostr = "Maximum log probability: {0:.3g}\n".format(ML)
    infostr += "Maximum Likelihood values:\n"
    maxlen = max(len(str(lb)) for lb in sampler.labels)
    for p, v, e in zip(sampler.labels, MLp, MLerr):
        infostr += "{2:>{0}}: {1:.3g} +/- {3:.3g}\n".format(maxlen, v, p, e)
    data = sampler.data
    if plotdata is None:
        # the data go on the plot when the model is a spectrum at the data's energies in units
        # that convert to the data's
        mx, my = model_ML
        plotdata = False
        if mx is not None and np.size(mx.value) == np.size(data["energy"].value):
            mu, _ = sed_conversion(data["energy"], my.unit, sed)
            du, _ = sed_conversion(data["energy"], data["flux"].unit, sed)
            plotdata = mu.is_equivalent(du)
    if plotresiduals is None:
        plotresiduals = bool(plotdata and (confs is not None or n_samples))
    f = plt.figure() if figure is None else figure
    if plotdata and plotresiduals:
        ax1 = plt.subplot2grid((4, 1), (0, 0), rowspan=3, fig=f)
        ax2 = plt.subplot2grid((4, 1), (3, 0), sharex=ax1, fig=f)
    else:
        ax1 = f.add_subplot(111)
    if e_unit is None:
        e_unit = data["energy"].unit
    if confs is not None:
        plot_CI(ax1, sampler, modelidx, sed=sed, confs=confs, e_unit=e_unit, label=label,
                e_range=e_range, e_npoints=e_npoints, last_step=last_step, seed=seed)
    elif n_samples:
        plot_samples(ax1, sampler, modelidx, sed=sed, n_samples=n_samples, e_unit=e_unit,
                     e_range=e_range, e_npoints=e_npoints, last_step=last_step, seed=seed)
    else:
        _plot_MLmodel(ax1, sampler, modelidx, e_range, e_npoints, e_unit, sed)
    if plotdata:
        _plot_data_to_ax(data, ax1, e_unit=e_unit, sed=sed, ylabel=ylabel, ulim_opts=ulim_opts,
                         errorbar_opts=errorbar_opts)
        if plotresiduals:
            _, _, _, ml = _calc_ML(sampler, modelidx, e_range=e_range, e_npoints=e_npoints)
            _plot_residuals_to_ax(data, ml, ax2, e_unit=e_unit, sed=sed,
                                  errorbar_opts=errorbar_opts)
    if ylabel is not None:
        ax1.set_ylabel(ylabel)
    if ML_info:
        ax1.text(0.05, 0.05, infostr, ha="left", va="bottom", transform=ax1.transAxes,
                 family="monospace")
    if label is not None:
        ax1.set_title(label)
    bottom = ax2 if plotdata and plotresiduals else ax1
    if plotdata and plotresiduals:
        for t in ax1.get_xticklabels():
            t.set_visible(False)
    bottom.set_xlabel(xlabel if xlabel is not None else
                      r"$\mathrm{Energy}$" + " [{0}]".format(_unit_label(e_unit)))
    ax1.set_xscale("log")
    ax1.set_yscale("log")
    f.subplots_adjust(hspace=0)
    return f


def _plot_ulims(ax, x, y, xerr, color, capsize=5, height_fraction=0.25, elinewidth=2):
    """upper limits as a bar with a downward arrow"""
    ax.errorbar(x, y, xerr=xerr, ls="", color=color, elinewidth=elinewidth, capsize=0)
    ax.errorbar(x, (1 - height_fraction) * y, yerr=height_fraction * y, ls="", color=color,
                elinewidth=elinewidth, capsize=capsize, uplims=True)


def _groups(data):
    g = data["group"] if "group" in data.keys() else np.zeros(np.size(data["energy"].value))
    return np.asarray(g)


def _energy_errors(data, e_unit):
    """(lo, hi) energy error bars; none (zeros) for a table without energy errors"""
    if "energy_error_lo" in data.keys() and "energy_error_hi" in data.keys():
        return data["energy_error_lo"].to(e_unit).value, data["energy_error_hi"].to(e_unit).value
    z = np.zeros(np.shape(data["energy"].value))
    return z, z


def _plot_data_to_ax(data, ax1, e_unit=None, sed=True, ylabel=None, ulim_opts={},
                     errorbar_opts={}):
    """flux points (error bars) and upper limits (arrows) of every data group"""
    if e_unit is None:
        e_unit = data["energy"].unit
    groups = _groups(data)
    df_unit, dsedf = sed_conversion(data["energy"], data["flux"].unit, sed)
    ene = data["energy"].to(e_unit).value
    flux = (data["flux"] * dsedf).to(df_unit).value
    elo = (data["flux_error_lo"] * dsedf).to(df_unit).value
    ehi = (data["flux_error_hi"] * dsedf).to(df_unit).value
    xlo, xhi = _energy_errors(data, e_unit)
    ul = np.asarray(data["ul"], dtype=bool)
    for g in np.unique(groups):
        sel = groups == g
        color = color_cycle[int(g) % len(color_cycle)]
        marker = marker_cycle[int(g) % len(marker_cycle)]
        opts = dict(zorder=100, marker=marker, ls="", elinewidth=2, capsize=0, mec=color,
                    mew=0.1, ms=5, color=color)
        opts.update(errorbar_opts)
        p = sel & ~ul
        ax1.errorbar(ene[p], flux[p], yerr=[elo[p], ehi[p]], xerr=[xlo[p], xhi[p]], **opts)
        q = sel & ul
        if np.any(q):
            uo = dict(capsize=5, height_fraction=0.25, elinewidth=2)
            uo.update(ulim_opts)
            _plot_ulims(ax1, ene[q], flux[q], [xlo[q], xhi[q]], color, **uo)
    ax1.set_xscale("log")
    ax1.set_yscale("log")
    xmin = 10 ** np.floor(np.log10(np.min(ene - xlo)))
    xmax = 10 ** np.ceil(np.log10(np.max(ene + xhi)))
    ax1.set_xlim(xmin, xmax)
    if ylabel is not None:
        ax1.set_ylabel(ylabel)
    elif ax1.get_ylabel() == "":
        name = "Flux" if df_unit.physical_type in ("flux", "differential flux") else "Luminosity"
        ax1.set_ylabel(r"$E^2\mathrm{d}N/\mathrm{d}E$" + " [{0}]".format(_unit_label(df_unit))
                       if sed else "{0} [{1}]".format(name, _unit_label(df_unit)))


def _plot_residuals_to_ax(data, model_ML, ax, e_unit=u.eV, sed=True, errorbar_opts={}):
    """(data - ML model) / error of every flux point that is not an upper limit"""
    mf_unit, msedf = sed_conversion(model_ML[0], model_ML[1].unit, sed)
    mene = model_ML[0].to(e_unit).value
    mflux = (model_ML[1] * msedf).to(mf_unit).value
    df_unit, dsedf = sed_conversion(data["energy"], data["flux"].unit, sed)
    ene = data["energy"].to(e_unit).value
    flux = (data["flux"] * dsedf).to(mf_unit).value
    dflux = ((data["flux_error_lo"] + data["flux_error_hi"]) / 2.0 * dsedf).to(mf_unit).value
    if mene.size != ene.size or not np.allclose(mene, ene):
        from scipy.interpolate import interp1d
        mflux = interp1d(mene, mflux, bounds_error=False)(ene)
    ul = np.asarray(data["ul"], dtype=bool)
    groups = _groups(data)
    xlo, xhi = _energy_errors(data, e_unit)
    ax.axhline(0, color="k", lw=1, ls="--")
    for g in np.unique(groups):
        p = (groups == g) & ~ul
        color = color_cycle[int(g) % len(color_cycle)]
        opts = dict(zorder=100, marker=marker_cycle[int(g) % len(marker_cycle)], ls="",
                    elinewidth=2, capsize=0, mec=color, mew=0.1, ms=6, color=color)
        opts.update(errorbar_opts)
        ax.errorbar(ene[p], (flux[p] - mflux[p]) / dflux[p], yerr=np.ones(p.sum()),
                    xerr=[xlo[p], xhi[p]], **opts)
    from matplotlib.ticker import MaxNLocator
    ax.yaxis.set_major_locator(MaxNLocator(5, integer=True, prune="upper", symmetric=True))
    ax.set_ylabel(r"$\Delta\sigma$")
    ax.set_xscale("log")


def plot_data(input_data, xlabel=None, ylabel=None, sed=True, figure=None, e_unit=None,
              ulim_opts={}, errorbar_opts={}):
    """The flux points of a data table (or of a sampler's ``data``) (plot.py:1207-1300)."""
    import matplotlib.pyplot as plt
    from .datatable import validate_data_table
    if hasattr(input_data, "data") and not isinstance(input_data, dict):
        data = input_data.data
    else:
        try:
            data = validate_data_table(input_data)
        except TypeError:
            if isinstance(input_data, dict) and "energy" in input_data:
                data = input_data
            else:
                raise
    f = plt.figure() if figure is None else figure
    ax1 = f.axes[0] if f.axes else f.add_subplot(111)
    if e_unit is None:
        e_unit = data["energy"].unit
    _plot_data_to_ax(data, ax1, e_unit=e_unit, sed=sed, ylabel=ylabel, ulim_opts=ulim_opts,
                     errorbar_opts=errorbar_opts)
    if xlabel is not None:
        ax1.set_xlabel(xlabel)
    elif ax1.get_xlabel() == "":
        ax1.set_xlabel(r"$\mathrm{Energy}$" + " [{0}]".format(_unit_label(e_unit)))
    ax1.autoscale()
    return f


def plot_ppc(sampler, modelidx=0, confs=(0.68, 0.95), seed=0, sed=True, figure=None):
    """The posterior predictive check of a fit (``naima_amd.predictive``): the data over the
    PREDICTIVE bands of central probability ``confs`` -- quantiles per energy of one replicated
    data set per stored spectrum, so they hold the noise of the data, unlike ``plot_fit``'s model
    bands -- and below them the probability integral transform of every flux point; the three
    Bayesian p-values in the title.  Replicates, quantiles and statistics are taken on the GPU."""
    from .infocrit import sampler_spectra
    from .predictive import posterior_predictive, ppc, predictive_quantiles
    confs = sorted((float(c) for c in confs), reverse=True)
    if not confs or not all(0.0 < c < 1.0 for c in confs):
        raise ValueError("confs must be probabilities in (0, 1)")
    import matplotlib.pyplot as plt
    model, data = sampler_spectra(sampler, modelidx=modelidx)
    spectra = as_matrix(model.value)  # (uploaded once for both calls)
    res = ppc(spectra, data, unit=model.unit, seed=seed)
    y = posterior_predictive(spectra, data, unit=model.unit, seed=seed)
    q = [0.5] + [v for c in confs for v in ((1.0 - c) / 2.0, (1.0 + c) / 2.0)]
    df_unit, dsedf = sed_conversion(data["energy"], data["flux"].unit, sed)
    fac = (u.Quantity(np.ones(y.ncol), data["flux"].unit) * dsedf).to(df_unit).value
    bands = predictive_quantiles(y, q) * fac
    e_unit = data["energy"].unit
    ene = data["energy"].to(e_unit).value
    f = plt.figure() if figure is None else figure
    ax1 = plt.subplot2grid((4, 1), (0, 0), rowspan=3, fig=f)
    ax2 = plt.subplot2grid((4, 1), (3, 0), sharex=ax1, fig=f)
    color = color_cycle[3]
    for i, c in enumerate(confs):
        ax1.fill_between(ene, bands[1 + 2 * i], bands[2 + 2 * i], lw=0.0, color=color,
                         alpha=0.25 + 0.25 * i / max(len(confs) - 1, 1),
                         label="{0:g}% predictive".format(100 * c))
    ax1.plot(ene, bands[0], color=color, lw=1)
    _plot_data_to_ax(data, ax1, e_unit=e_unit, sed=sed)
    ax1.legend(loc="lower left", frameon=False)
    ax1.set_title(r"$p_{{\chi^2}}$ = {0:.3f}   $p_\mathrm{{max}}$ = {1:.3f}   "
                  r"$p_\mathrm{{runs}}$ = {2:.3f}".format(res["p_chi2"], res["p_max"],
                                                          res["p_runs"]))
    ax2.axhline(0.5, color="k", lw=1, ls="--")
    ax2.plot(ene, res["pit"], ls="", marker="o", ms=5, color=color_cycle[0])
    ax2.plot(ene, res["ul_violation"], ls="", marker="v", ms=5, color=color_cycle[2])
    ax2.set_ylim(0.0, 1.0)
    ax2.set_ylabel("PIT")
    ax2.set_xlabel(r"$\mathrm{Energy}$" + " [{0}]".format(_unit_label(e_unit)))
    for t in ax1.get_xticklabels():
        t.set_visible(False)
    f.subplots_adjust(hspace=0)
    return f


def plot_profile(result, figure=None):
    """A profile likelihood (``optimize.ProfileResult``, or a list of them, one panel each):
    2 Delta lnL against the parameter, with the 1 sigma and 2 sigma lines at 1 and 4 and the
    68.3 % interval shaded where the grid brackets it."""
    import warnings

    import matplotlib.pyplot as plt
    results = list(result) if isinstance(result, (list, tuple)) else [result]
    if not results or not all(hasattr(r, "delta_chi2") for r in results):
        raise ValueError("plot_profile takes a ProfileResult or a list of them")
    f = plt.figure() if figure is None else figure
    for k, r in enumerate(results):
        ax = f.add_subplot(1, len(results), k + 1)
        ax.plot(r.grid, r.delta_chi2, marker="o", ms=3, lw=1, color=color_cycle[0])
        for level, ls in ((1.0, "--"), (4.0, ":")):
            ax.axhline(level, color="k", lw=1, ls=ls)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lo, hi = r.interval(0.683)
        if np.isfinite(lo) and np.isfinite(hi):
            ax.axvspan(lo, hi, color=color_cycle[0], alpha=0.15, lw=0)
        ax.axvline(r.ml.x[r.par], color=color_cycle[3], lw=1)
        ax.set_xlabel(r.label)
        finite = r.delta_chi2[np.isfinite(r.delta_chi2)]
        ax.set_ylim(0.0, max(6.0, min(float(finite.max()) if finite.size else 6.0, 25.0)))
        if k == 0:
            ax.set_ylabel(r"$2\,\Delta\ln\mathcal{L}$")
    return f


def plot_corner(sampler, show_ML=True, **kwargs):
    """Corner plot of the chain (plot.py:1393-1439): through ``corner.corner`` when the corner
    package is installed; else, after a warning, the built-in figure ``posterior.corner`` draws
    from histograms taken on the GPU (of the keywords, those it knows are passed on)."""
    import warnings
    try:
        import corner
    except ImportError:
        corner = None
        warnings.warn("The corner package is not installed; corner plot not available from it: "
                      "drawing the built-in corner figure (naima_amd.posterior.corner)")
    import matplotlib.pyplot as plt
    oldlw = plt.rcParams["lines.linewidth"]
    plt.rcParams["lines.linewidth"] = 0.7
    try:
        opts = dict(labels=sampler.labels, quantiles=[0.16, 0.5, 0.84], verbose=False,
                    truth_color=color_cycle[0])
        if show_ML:
            _, MLp, _, _ = find_ML(sampler, None)
            opts["truths"] = MLp
        opts.update(kwargs)
        chain = np.asarray(sampler.get_chain(flat=True))
        if corner is not None:
            f = corner.corner(chain, **opts)
        else:
            from . import posterior
            known = ("labels", "truths", "quantiles", "bins", "range", "levels", "truth_color",
                     "fig")
            f = posterior.corner(chain, **{k: v for k, v in opts.items() if k in known})
    finally:
        plt.rcParams["lines.linewidth"] = oldlw
    return f
