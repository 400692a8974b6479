"""The cases of tests/golden/plan_shapes.json: which models at which ensemble sizes, how a case is
run for one step with the descriptor of every nh_half_step_create captured, and what of it is
compared.  test_plan_shape_host.py replays the recorded sizes through the planner (nh_hs_plan.h)
without a GPU; test_gpu_plan_shapes.py holds the library's plans and resident loops to the record.

A case's record: {"ncu", "knobs": {"run_rt"}, "plans": [{"in": sizes, "out": plan info}, ...],
"resident": resident_info or None}.  Numbers only: no pointer of a descriptor is kept; a component
of the likelihood is kept as (which table or the synchrotron component produces it, offset)."""
import ctypes as C
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_shapes.json")

PER_HALF_STEP = (8, 128, 256, 512, 2048)
T_KINDS = ("ic", "pion-lut", "pion-analytic", "bremsstrahlung")
NSTEPS = 3  # (the first step records the model's launches; the plan and the resident loop follow)


def case_ids():
    ids = ["%s/%d" % (w, n) for w in ("cfg1", "cfg2", "cfg3", "cfg5") for n in PER_HALF_STEP]
    ids.append("cfg4/256")
    import test_gpu_shapes as TS
    ids += ["S/" + c[0] for c in TS.S_CASES]
    ids += ["T/%s/rt%d" % (k, rt) for k in T_KINDS for rt in (1, 0)]
    return ids


def _problem(na, cid):
    """(model, prior, data, start positions, environment) of a case"""
    parts = cid.split("/")
    if parts[0].startswith("cfg"):
        from bench import build_problem
        model, p0, raw, data, prior, labels = build_problem(parts[0], na)
        nw = 2 * int(parts[1])
        pos = p0 + 0.01 * p0 * np.random.default_rng(3).normal(size=(nw, p0.size))
        return model, prior, data, pos, {}
    import test_gpu_shapes as TS
    from naima_amd.datatable import make_data
    if parts[0] == "S":
        case = [c for c in TS.S_CASES if c[0] == parts[1]][0]
        cname, sgrid, igrid, nw, m, E, beta, regime = case
        igrid = sgrid if igrid == "same" else (1e11, 1e15, 40)
        model, omodel = TS.syn_ic(na, sgrid, igrid, beta)
        prior, _ = TS.uniform([(20, 45), (-1, 4), (-2, 3), (-0.5, 3.5)])
        p0 = np.array([33.0, 2.3, 1.2 if beta == 1.0 else 0.0, 1.5])
        if cname == "below-tbot":
            p0 = np.array([31.0, 0.3, 2.3, 1.5])
        rng = np.random.default_rng(len(cname) * 7 + nw)
        true = TS._repr(omodel(p0, E)[0], E, "erg/(cm2 s)")
        raw = TS.make_raw(E, true, "erg/(cm2 s)", rng, rel=(0.05, 0.05), scatter=0.05, cl0=0.9,
                          dcl=0.0)
        pos = TS._spread(p0, nw, np.random.default_rng(31), [0.1, 0.05, 0.5, 1.5])
        return model, prior, make_data(raw), pos, {}
    kind, rt = parts[1], parts[2][2:]
    model, omodel, E, lut = TS._table_case(na, kind)
    prior, _ = TS.uniform([(20, 60), (1, 4), (-1, 3)])
    p0 = np.array([46.0 if kind.startswith("pion") else 33.0, 2.3, 1.0])
    true = TS._repr(omodel(p0)[0], E, "1/(cm2 s TeV)")
    raw = TS.make_raw(E, true, "1/(cm2 s TeV)", np.random.default_rng(41),
                      zero_below=1e-6 if lut else 1e-100)
    pos = TS._spread(p0, 16, np.random.default_rng(42), [0.05, 0.05, 0.1])
    return model, prior, make_data(raw), pos, {"NH_RUN_RT": rt}


def _download(ctx, ptr, n):
    from naima_amd import _lib
    host = np.empty(n)
    ctx.sync()
    _lib._chk(_lib._lib.nh_download(ctx.h, host.ctypes.data, ptr, host.nbytes))
    return host


def _sizes(ctx, d):
    """the sizes of an nh_hs_desc that the planner reads, and what the device facts it asks for are
    (per table the first row that holds a non-zero; the synchrotron grid's end points)"""
    grids = [dict(nG=d.grids[g].nG, unit_scale=d.grids[g].unit_scale) for g in range(d.ngrids)]
    tabs = []
    for t in range(d.ntab):
        tb = d.tab[t]
        nG, nK = d.grids[tb.grid].nG, tb.nK
        kd = _download(ctx, tb.KD, 2 * nG * nK).reshape(nG, nK, 2)[:nG - 1, :, 0]
        rows = np.flatnonzero((kd != 0.0).any(axis=1))
        tabs.append(dict(grid=tb.grid, nK=nK, ldo=tb.ldo, nonnegative=tb.nonnegative,
                         r0=int(rows[0]) if rows.size else nG - 1))
    syn = dict(grid=d.syn.grid)
    if d.syn.grid >= 0:
        s, gr = d.syn, d.grids[d.syn.grid]
        xg = _download(ctx, gr.xg, gr.nG)
        syn.update(nE=s.nE, n1=s.n1, ldo=s.ldo, ldo2=s.ldo2, two_outputs=int(bool(s.out2)),
                   bcol=s.bcol, x_first=float(xg[0]), x_last=float(xg[-1]), nG=gr.nG,
                   unit_scale=gr.unit_scale)
    comps = []
    for q in range(d.ncomp):  # (which table -- or -1: the synchrotron component -- and where in it)
        cp, src = d.comps[q], None
        for t in range(d.ntab):
            if cp.ptr >= d.tab[t].out and cp.ld == d.tab[t].ldo and src is None and \
                    (cp.ptr - d.tab[t].out) // 8 + d.nE <= d.tab[t].nK:
                src = dict(table=t, at=(cp.ptr - d.tab[t].out) // 8)
        if src is None and d.syn.grid >= 0 and cp.ptr >= d.syn.out and cp.ld == d.syn.ldo and \
                (cp.ptr - d.syn.out) // 8 + d.nE <= d.syn.nE:
            src = dict(table=-1, at=(cp.ptr - d.syn.out) // 8)
        comps.append(src or dict(table=-2, at=0))
    return dict(ns=d.ns, ndim=d.ndim, lo=d.lo, nloc=d.nloc, kind=d.kind, npacks=d.npacks,
                grids=grids, moms=[d.moms[m].grid for m in range(d.nmoms)], tabs=tabs, syn=syn,
                nE=d.nE, ncomp=d.ncomp, comps=comps, nblobs=d.nblobs,
                blobs=[dict(kind=d.blobs[b].kind, m=d.blobs[b].m, mom=d.blobs[b].mom)
                       for b in range(d.nblobs)],
                nterms=d.nterms, do_accept=d.do_accept, write_weights=d.write_weights,
                send_width=d.send_width, has_lp=int(bool(d.lp)))


def run_case(na, monkeypatch, cid):
    """NSTEPS steps of the device loop on the case's model -> the case's record"""
    from naima_amd import _lib, step_plan
    from naima_amd.sampler import EnsembleSampler
    model, prior, data, pos, env = _problem(na, cid)
    for k in ("NAIMA_AMD_RESIDENT", "NAIMA_AMD_MEGA", "NH_RUN_RT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = _lib.get_context()
    plans = []
    create = step_plan.StepPlan._create

    def recording(self, ctx_, d):
        h = create(self, ctx_, d)
        thr, blk, lds, spl, form = _lib._i(), _lib._i(), _lib._ll(), _lib._i(), _lib._i()
        _lib._chk(_lib._lib.nh_half_step_info(h, C.byref(thr), C.byref(blk), C.byref(lds)))
        _lib._chk(_lib._lib.nh_half_step_split(h, C.byref(spl)))
        _lib._chk(_lib._lib.nh_half_step_syn_form(h, C.byref(form)))
        plans.append({"in": _sizes(ctx_, d),
                      "out": dict(threads=thr.value, blocks=blk.value, lds_bytes=lds.value,
                                  split=spl.value, syn_form=form.value)})
        return h

    monkeypatch.setattr(step_plan.StepPlan, "_create", recording)
    nw, nd = pos.shape
    s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=5, naima_style=True,
                        store_blobs=True, device=True)
    s.run_mcmc(pos, NSTEPS)
    dev = s._dev
    info = getattr(dev, "resident_info", None)
    rec = dict(ncu=ctx.info()["compute_units"], knobs=dict(run_rt=int(env.get("NH_RUN_RT", 1))),
               plans=plans, resident=None if info is None else {k: int(v) for k, v in info.items()})
    if info is None:  # (the refusal is the expected output)
        rec["resident_reason"] = getattr(dev, "resident_reason", None)
    return rec


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
