"""Results on disk with the layout of naima's ``save_run`` (analysis.py:366-471 of the
reference: group ``mcmc`` with ``chain, log_prob, blobN, data`` + attributes).  With h5py
the file IS the reference's HDF5 file (naima's own ``read_run`` reads it: checked when the
golden schema is generated, tests/golden/gen_golden_run.py); h5py is not installed on the
target image, where the same objects go into a ``.npz`` under the same names.  ``read_run``
rebuilds a read-only result object with the attributes naima's post-processing reads."""
import json

import numpy as np

from . import units as u
from .datatable import DataTable
from .infocrit import InfoCritMixin
from .predictive import PredictiveMixin
from .reweight import ReweightMixin

__all__ = ["save_run", "read_run", "save_results_table", "find_ML", "save_diagnostic_plots"]


def _unit_string(unit):
    """unit -> the string stored with a dataset, in astropy's spelling where the unit's name
    is a plain product / quotient of named units: ``1 / (cm2 s TeV)``, ``erg / (cm2 s)`` --
    factors by decreasing power, then alphabetically (case-insensitive), as
    ``astropy.units.UnitBase.to_string()`` writes them.  Anything else is stored as named;
    the reference reads either back with ``u.Quantity(..., unit=str)``."""
    import re
    if unit is None:
        return ""
    name = unit.name.strip()
    m = re.fullmatch(r"([^/()]*?)\s*(?:/\s*\(?([^/()]*?)\)?)?", name)
    tok = r"[A-Za-z]+\d*"
    if not m:
        return name
    num, den = (m.group(1) or "").strip(), (m.group(2) or "").strip()
    if num == "1":
        num = ""
    parts = []
    for side in (num, den):
        toks = side.split()
        if any(not re.fullmatch(tok, t) for t in toks):
            return name
        split = [re.fullmatch(r"([A-Za-z]+)(\d*)", t).groups() for t in toks]
        split.sort(key=lambda bp: (-int(bp[1] or 1), bp[0].lower()))
        parts.append(" ".join(b + p for b, p in split))
    num, den = parts
    if not den:
        return num
    den = "(%s)" % den if " " in den else den
    return "%s / %s" % (num or "1", den)


def run_layout(sampler):
    """What ``save_run`` writes, container-independent -- exactly the objects of the
    reference's HDF5 file (analysis.py:366-471):

      group ``mcmc``: attrs = run_info + ``acceptance_fraction`` + ``label<i>``
        ``chain``     [nsteps][nwalkers][ndim]
        ``log_prob``  [nsteps][nwalkers]
        ``blob<i>``   blob i of every (step, walker), FLATTENED over steps x walkers
                      (analysis.py:433-438), attr ``unit``
        ``data``      the data table as a structured array (astropy ``write_table_hdf5``)
        ``data.__table_column_meta__``  its YAML column / unit description, one line per row

    Returns (attrs, datasets) with datasets[name] = (array, dataset attrs)."""
    attrs = {}
    for k, v in dict(getattr(sampler, "run_info", {})).items():
        attrs[k] = v
    attrs["acceptance_fraction"] = float(np.mean(sampler.acceptance_fraction))
    for i, label in enumerate(sampler.labels):
        attrs["label{0}".format(i)] = str(label)
    ds = {"chain": (np.asarray(sampler.get_chain(), dtype=float), {}),
          "log_prob": (np.asarray(sampler.get_log_prob(), dtype=float), {})}
    blobs = sampler.get_blobs() or []
    units = list(getattr(sampler, "blob_units", None) or [None] * len(blobs))
    for j, b in enumerate(blobs):
        b = np.asarray(b, dtype=float)
        ds["blob{0}".format(j)] = (b.reshape((-1,) + b.shape[2:]), {"unit": _unit_string(units[j])})
    data = getattr(sampler, "data", None)
    if data is not None:
        fields, lines, ser = [], ["datatype:"], {}
        for k, v in data.items():
            if isinstance(v, u.Quantity):
                arr, un = np.asarray(v.value, dtype=float), _unit_string(v.unit)
            else:
                arr, un = np.asarray(v), None
            if arr.dtype.kind == "i":
                arr = arr.astype(np.int64)
            fields.append((k, arr))
            dt = {"f": "float64", "i": "int64", "b": "bool"}[arr.dtype.kind]
            lines.append("- {{name: {0}, {1}datatype: {2}}}".format(
                k, "unit: {0}, ".format(un) if un is not None else "", dt))
            if un is not None:
                ser[k] = un
        n = len(fields[0][1])
        table = np.zeros(n, dtype=[(k, a.dtype.str.replace("|b1", "?")) for k, a in fields])
        for k, a in fields:
            table[k] = a
        # astropy's serialisation of the Quantity columns (alphabetical, one YAML anchor per
        # distinct unit, in order of first appearance)
        lines += ["meta: !!omap", "- __serialized_columns__:"]
        anchors = {}
        for k in sorted(ser):
            un = ser[k]
            lines += ["    {0}:".format(k), "      __class__: astropy.units.quantity.Quantity"]
            if un in anchors:
                lines.append("      unit: *{0}".format(anchors[un]))
            else:
                anchors[un] = "id{0:03d}".format(len(anchors) + 1)
                lines.append("      unit: &{0} !astropy.units.Unit {{unit: {1}}}".format(anchors[un], un))
            lines.append("      value: !astropy.table.SerializedColumn {{name: {0}}}".format(k))
        ds["data"] = (table, {})
        ds["data.__table_column_meta__"] = (np.array([x.encode() for x in lines]), {})
    return attrs, ds


def save_run(filename, sampler, compression=True, clobber=False):
    """Save the sampler chain, log-probabilities, blobs, data table, parameter labels and
    run info (analysis.py:366-471).  ``*.h5`` / ``*.hdf5``: the reference's HDF5 file,
    object for object (needs h5py; naima's ``read_run`` reads it).  Anything else: the same
    objects under the same names in a ``.npz`` (h5py is not installed on the target image)."""
    import os
    attrs, ds = run_layout(sampler)
    if filename.endswith((".h5", ".hdf5")):
        try:
            import h5py
        except ImportError:
            raise ImportError("writing %s needs h5py; use a .npz file name for the same layout "
                              "without it" % filename)
        if os.path.exists(filename) and not clobber:
            import warnings
            warnings.warn("Not writing file because file exists and clobber is False")
            return None
        with h5py.File(filename, "w") as f:
            g = f.create_group("mcmc")
            for name, (arr, dattrs) in ds.items():
                kw = {"compression": "gzip"} if compression and arr.ndim > 0 and arr.dtype.kind != "S" \
                    else {}
                d = g.create_dataset(name, data=arr, **kw)
                for k, v in dattrs.items():
                    d.attrs[k] = v
            for k, v in attrs.items():
                try:
                    g.attrs[k] = v
                except TypeError:
                    g.attrs[k] = str(v)
        return filename
    if not filename.endswith(".npz"):
        filename += ".npz"
    if os.path.exists(filename) and not clobber:
        raise OSError("{0} exists; pass clobber=True to overwrite".format(filename))
    out = {}
    dattrs = {}
    for name, (arr, da) in ds.items():
        out["mcmc/" + name] = arr
        if da:
            dattrs[name] = da
    meta = {"attrs": {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in attrs.items()},
            "dataset_attrs": dattrs}
    out["mcmc.attrs"] = np.array(json.dumps(meta, default=str))
    (np.savez_compressed if compression else np.savez)(filename, **out)
    return filename


class _Result(InfoCritMixin, PredictiveMixin, ReweightMixin):
    """what read_run returns: chain / log-prob / blobs with emcee's accessor names, and the
    sampler's get_pointwise_log_likelihood / waic / loo / get_posterior_predictive / ppc /
    reweight / influence"""

    def __init__(self, chain, log_prob, blobs, blob_units, data, labels, run_info, accf):
        self._chain, self._lp, self._blobs = chain, log_prob, blobs
        self.blob_units, self.data, self.labels, self.run_info = blob_units, data, labels, run_info
        self.acceptance_fraction = accf

    def get_chain(self, flat=False, discard=0, thin=1):
        c = self._chain[discard::thin]
        return c.reshape(-1, c.shape[-1]) if flat else c

    def get_log_prob(self, flat=False, discard=0, thin=1):
        c = self._lp[discard::thin]
        return c.reshape(-1) if flat else c

    def get_blobs(self, flat=False, discard=0, thin=1):
        out = []
        for b in self._blobs:
            a = b[discard::thin]
            out.append(a.reshape((-1,) + a.shape[2:]) if flat else a)
        return out

    def get_ess(self, kind="bulk", discard=0, thin=1):
        """``EnsembleSampler.get_ess`` of the saved chain"""
        from .posterior import _check_kind, ess
        _check_kind(kind)
        return ess(self.get_chain(discard=discard, thin=thin), kind)

    def get_summary(self, discard=0):
        """``EnsembleSampler.get_summary`` of the saved chain (its ensembles from ``run_info``)"""
        from .posterior import summary
        return summary(self.get_chain(discard=discard), int(self.run_info.get("ensembles", 1)),
                       labels=self.labels or None)

    @property
    def chain(self):
        return np.swapaxes(self._chain, 0, 1)

    @property
    def flatchain(self):
        return self.get_chain(flat=True)

    @property
    def lnprobability(self):
        return self._lp.T


def _table_from(table, meta_lines):
    """structured array + astropy column meta lines -> DataTable (units restored)"""
    units = {}
    for line in [x.decode() if isinstance(x, bytes) else str(x) for x in meta_lines]:
        line = line.strip()
        if line.startswith("- {name:") and "unit:" in line:
            body = line[3:-1]
            name = body.split("name:")[1].split(",")[0].strip()
            units[name] = body.split("unit:")[1].rsplit(", datatype", 1)[0].strip()
    data = DataTable()
    for name in table.dtype.names:
        col = np.asarray(table[name])
        data[name] = u.Quantity(col, u.Unit(units[name])) if name in units else col
    return data


def read_run(filename, modelfn=None):
    """Read a run saved by ``save_run`` (either container).  ``modelfn``, the run's model
    function, is attached to the result as ``modelfn`` (analysis.py:497-530) so that the plots
    can recompute the model on an ``e_range`` grid."""
    if filename.endswith((".h5", ".hdf5")):
        import h5py
        with h5py.File(filename, "r") as f:
            g = f["mcmc"]
            attrs = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in g.attrs.items()}
            ds = {k: (np.array(g[k]), dict(g[k].attrs)) for k in g.keys()}
    else:
        if not filename.endswith(".npz"):
            filename += ".npz"
        z = np.load(filename, allow_pickle=False)
        meta = json.loads(str(z["mcmc.attrs"]))
        attrs = meta["attrs"]
        ds = {k[len("mcmc/"):]: (z[k], meta["dataset_attrs"].get(k[len("mcmc/"):], {}))
              for k in z.files if k.startswith("mcmc/")}
    chain, log_prob = ds["chain"][0], ds["log_prob"][0]
    nsteps, nwalkers = chain.shape[:2]
    blobs, units, j = [], [], 0
    while "blob%d" % j in ds:
        arr, da = ds["blob%d" % j]
        blobs.append(arr.reshape((nsteps, nwalkers) + arr.shape[1:]))
        un = da.get("unit", "")
        un = un.decode() if isinstance(un, bytes) else un
        units.append(u.Unit(un) if un else None)
        j += 1
    data = _table_from(ds["data"][0], ds["data.__table_column_meta__"][0]) if "data" in ds else None
    labels, i = [], 0
    while "label%d" % i in attrs:
        labels.append(attrs["label%d" % i])
        i += 1
    run_info = {k: v for k, v in attrs.items()
                if not k.startswith("label") and k != "acceptance_fraction"}
    res = _Result(chain, log_prob, blobs, units, data, labels, run_info,
                  attrs.get("acceptance_fraction"))
    res.modelfn = modelfn
    return res


def find_ML(sampler, refine=False):
    """(max log-probability, its parameter vector): the most probable sample of the chain
    (the first return values of analysis-time ``find_ML`` in the reference, which
    ``save_results_table`` stores as ``MaxLogLikelihood`` / ``ML_pars``; no refit).
    ``refine=True``: the refitted point instead -- ``sampler.fit_ml(prior=True)``, simplex
    searches from the most probable samples under the sampler's own log-probability (on the
    GPU, ``naima_amd.optimize``), which is never worse than the best sample it starts from."""
    if refine:
        ml = sampler.fit_ml(prior=True)
        return float(ml.fun), ml.x
    lp = np.asarray(sampler.get_log_prob())
    chain = np.asarray(sampler.get_chain())
    idx = np.unravel_index(np.argmax(lp), lp.shape)
    return float(lp[idx]), chain[idx]


def save_diagnostic_plots(outname, sampler, modelidxs=None, pdf=False, sed=True, blob_labels=None,
                          last_step=False, dpi=100):
    """Diagnostic figures of a run (analysis.py:29-162 of the reference): the chain and posterior
    of every parameter (``<outname>_chain_<label>.png``, log prefixes stripped), the corner plot
    (``<outname>_corner.png``; the built-in figure when the corner package is not installed) and
    every model blob
    (``<outname>_model<i>.png``: a spectrum with 100 sample models, the ML model, data and
    residuals; a scalar as its distribution).  ``pdf=True``: all of them as the pages of
    ``<outname>_plots.pdf`` instead.  Collective on a sampler that spans several ranks."""
    import warnings

    from matplotlib import pyplot as plt

    from .plot import plot_blob, plot_chain, plot_corner
    old_interactive = plt.rcParams["interactive"]
    plt.rcParams["interactive"] = False
    outpdf = None
    if pdf:
        from matplotlib.backends.backend_pdf import PdfPages
        plt.rc("pdf", fonttype=42)
        outpdf = PdfPages("{0}_plots.pdf".format(outname))

    def save(f, png):
        if outpdf is not None:
            f.savefig(outpdf, format="pdf", dpi=dpi)
        else:
            f.savefig(png, dpi=dpi)
        f.clf()
        plt.close(f)

    try:
        for par, label in enumerate(sampler.labels):
            try:
                f = plot_chain(sampler, par, last_step=last_step)
                if "log(" in label or "log10(" in label:
                    label = label.split("(")[-1].split(")")[0]
                save(f, "{0}_chain_{1}.png".format(outname, label))
            except Exception as e:
                warnings.warn("plot_chain failed for parameter {0} ({1}): {2}".format(label, par, e))
        f = plot_corner(sampler)
        if f is not None:
            save(f, "{0}_corner.png".format(outname))
        if modelidxs is None:
            modelidxs = list(range(len(sampler.get_blobs() or [])))
        sed = [sed] * len(modelidxs) if isinstance(sed, bool) else list(sed)
        if blob_labels is None:
            blob_labels = []
        elif isinstance(blob_labels, str):
            blob_labels = [blob_labels]
        blob_labels = list(blob_labels) + ["Model output {0}".format(i)
                                           for i in modelidxs[len(blob_labels):]]
        for modelidx, plot_sed, label in zip(modelidxs, sed, blob_labels):
            try:
                f = plot_blob(sampler, blobidx=modelidx, label=label, sed=plot_sed, n_samples=100,
                              last_step=last_step)
                save(f, "{0}_model{1}.png".format(outname, modelidx))
            except Exception as e:
                warnings.warn("plot_blob failed for {0}: {1}".format(label, e))
    finally:
        if outpdf is not None:
            outpdf.close()
        plt.rcParams["interactive"] = old_interactive


def save_results_table(outname, sampler, convert_log=True, last_step=False, include_blobs=True,
                       overwrite=False, information_criteria=False, diagnostics=False,
                       goodness_of_fit=False, evidence=None, profile=False):
    """Write ``<outname>_results.ecsv``: median and 16th/84th-percentile distances of every
    parameter (plus the de-logged value for ``log10(x)`` / ``log(x)`` labels and every
    scalar blob), with the run information, the most probable parameters and the BIC as
    metadata (analysis.py:165-363 of the reference; ECSV written directly, astropy is not
    available).  ``information_criteria=True`` adds ``WAIC_elpd``, ``WAIC_p``, ``LOO_elpd``,
    ``LOO_p``, ``LOO_se`` and ``LOO_max_pareto_k`` of the whole chain's stored spectra (blob 0,
    ``naima_amd.infocrit``, computed on the GPU) to the metadata; without it the file is what it
    always was.  ``diagnostics=True`` adds ``ESS_bulk`` and ``ESS_tail`` per parameter and, for a
    run of several ensembles, ``Rhat_rank`` (``posterior.summary`` of the whole chain, ranked on
    the GPU).  ``goodness_of_fit=True`` adds ``PPC_p_chi2``, ``PPC_p_max``, ``PPC_p_runs`` and
    ``PPC_chi2_obs_mean`` of the posterior predictive check of the whole chain's stored spectra
    (blob 0, ``naima_amd.predictive.ppc`` with seed 0).  ``evidence`` adds ``logZ``, ``logZ_err``
    and ``logZ_forbidden_fraction``: a result of ``naima_amd.evidence.bridge_sampling``, or True
    for ``sampler.log_evidence()`` with its defaults (a sampler only: a read run has no
    log-probability function; and mind that module's docstring on proper priors and
    ``log_prior_norm``).  ``profile=True`` adds the maximum-likelihood refit ``ML_refit`` and
    ``ML_refit_pars`` (``sampler.fit_ml()``, flat prior) and the Delta lnL = 1/2 profile-likelihood
    interval of every parameter, ``<label>_profile_lo`` / ``_hi`` (``sampler.profile_likelihood``;
    null where the grid does not bracket it).  Returns the table as a dict of columns +
    ``meta``."""
    import os

    import yaml
    fname = "{0}_results.ecsv".format(outname)
    if os.path.exists(fname) and not overwrite:
        raise OSError("{0} exists; pass overwrite=True".format(fname))
    labels = list(sampler.labels)
    chain = np.asarray(sampler.get_chain())
    dists = chain[-1] if last_step else chain.reshape(-1, chain.shape[-1])
    quant = [16, 50, 84]
    rows = []

    def add(label, dist):
        lo, med, hi = np.percentile(dist, quant)
        rows.append((label, float(med), float(med - lo), float(hi - med)))

    for p, label in enumerate(labels):
        add(label, dists[:, p])
        if convert_log and ("log10(" in label or "log(" in label):
            nlabel = label.split("(")[-1].split(")")[0]
            add(nlabel, 10 ** dists[:, p] if label.split("(")[0] == "log10" else np.exp(dists[:, p]))
    meta = {"n_samples": int(dists.shape[0])}
    ML, MLp = find_ML(sampler)
    meta["ML_pars"] = [float(x) for x in MLp]
    meta["MaxLogLikelihood"] = ML
    ndata = len(sampler.data["energy"]) if getattr(sampler, "data", None) is not None else 0
    if ndata:
        meta["BIC"] = float(len(MLp) * np.log(ndata) - 2 * ML)
    if information_criteria:
        from .infocrit import loo, sampler_pointwise, waic
        L = sampler_pointwise(sampler)
        w, lo = waic(L), loo(L)
        meta["WAIC_elpd"], meta["WAIC_p"] = w["elpd_waic"], w["p_waic"]
        meta["LOO_elpd"], meta["LOO_p"], meta["LOO_se"] = lo["elpd_loo"], lo["p_loo"], lo["se"]
        meta["LOO_max_pareto_k"] = float(np.max(lo["pareto_k"]))
    if diagnostics:
        from .posterior import summary
        k = int(getattr(sampler, "run_info", {}).get("ensembles", getattr(sampler, "ensembles", 1)))
        sm = summary(chain, k)
        meta["ESS_bulk"] = [float(v) for v in sm["ess_bulk"]]
        meta["ESS_tail"] = [float(v) for v in sm["ess_tail"]]
        if k > 1:
            meta["Rhat_rank"] = [float(v) for v in sm["rhat_rank"]]
    if goodness_of_fit:
        from .infocrit import sampler_spectra
        from .predictive import ppc
        g = ppc(*sampler_spectra(sampler))
        meta["PPC_p_chi2"], meta["PPC_p_max"] = g["p_chi2"], g["p_max"]
        meta["PPC_p_runs"], meta["PPC_chi2_obs_mean"] = g["p_runs"], g["chi2_obs"]["mean"]
    if evidence is not None and evidence is not False:
        if evidence is True:
            if not hasattr(sampler, "log_evidence"):
                raise ValueError("evidence=True needs a sampler with a log-probability function; "
                                 "pass a result of naima_amd.evidence.bridge_sampling")
            evidence = sampler.log_evidence()
        try:
            meta["logZ"], meta["logZ_err"] = float(evidence["logz"]), float(evidence["logz_err"])
            meta["logZ_forbidden_fraction"] = float(evidence["forbidden_fraction"])
        except (TypeError, KeyError, IndexError):
            raise ValueError("evidence must be True or a result of evidence.bridge_sampling")
    if profile:
        if not hasattr(sampler, "profile_likelihood"):
            raise ValueError("profile=True needs a sampler with a log-probability function")
        ml = sampler.fit_ml()
        meta["ML_refit"], meta["ML_refit_pars"] = float(ml.fun), [float(x) for x in ml.x]
        for label, pr in zip(labels, sampler.profile_likelihood(list(range(len(labels))), ml=ml)):
            lo, hi = pr.interval(0.683)
            meta[label + "_profile_lo"] = None if np.isnan(lo) else float(lo)
            meta[label + "_profile_hi"] = None if np.isnan(hi) else float(hi)
    for k, v in dict(getattr(sampler, "run_info", {})).items():
        meta[k] = v.tolist() if isinstance(v, np.ndarray) else (v.item() if isinstance(
            v, np.generic) else v)
    if include_blobs:
        blobs = sampler.get_blobs() or []
        units = list(getattr(sampler, "blob_units", None) or [None] * len(blobs))
        for idx, b in enumerate(blobs):
            b = np.asarray(b)
            if b.ndim == 2:  # one scalar per walker and step
                add("blob{0}".format(idx), b[-1] if last_step else b.ravel())
                if units[idx] is not None:
                    meta["blob{0}_unit".format(idx)] = units[idx].name
    cols = [("label", "string", "Name of the parameter"),
            ("median", "float64", "Median of the posterior distribution function"),
            ("unc_lo", "float64", "Difference between the median and the 16th percentile of the "
                                  "pdf, ~1sigma lower uncertainty"),
            ("unc_hi", "float64", "Difference between the 84th percentile and the median of the "
                                  "pdf, ~1sigma upper uncertainty")]
    header = {"datatype": [dict(name=n, datatype=t, description=d) for n, t, d in cols],
              "meta": meta}
    with open(fname, "w") as f:
        f.write("# %ECSV 1.0\n# ---\n")
        for line in yaml.safe_dump(header, default_flow_style=None, sort_keys=False).splitlines():
            f.write("# " + line + "\n")
        f.write("label median unc_lo unc_hi\n")
        for label, med, lo, hi in rows:
            f.write('"{0}" {1!r} {2!r} {3!r}\n'.format(label, med, lo, hi))
    return {"label": [r[0] for r in rows], "median": np.array([r[1] for r in rows]),
            "unc_lo": np.array([r[2] for r in rows]), "unc_hi": np.array([r[3] for r in rows]),
            "meta": meta}
