"""What the device step loop records of ONE evaluation of the user's model, and replays.

The loop (device_sampler.DeviceLoop) first RECORDS what a model evaluation asks of the context
(parameter packs, the particle-weights launch, single-row reductions such as We, emission
launches, persistent output buffers, the names of all launches), then has nh_step_front -- or,
when ``can_be_one_launch`` admits the plan, ONE nh_half_step launch -- produce all of it right
after the proposal.  While a plan REPLAYS, a request of the model (Context.pack_rows,
weights_multi, moment, emit_tables, emit_synchrotron, plan_buffer) only checks that it is the
recorded one and returns its buffers.  The context holds the plan of the evaluation in progress
(Context._plan) and the likelihood's accept hook (Context._accept_hook) and asks them; the lists,
the cursors and the descriptors of the launches are kept here.
"""
import ctypes as C
import dataclasses
import os
import typing

import numpy as np

from . import _lib
from . import darray as D

KINDS = ("packs", "weights", "moments", "emit", "bufs")
_CHANGED = ("the model's launch sequence changed between evaluations (%s); "
            "run the sampler with use_graph=False")


class TabKey(typing.NamedTuple):
    """an nh_integrate_tables launch of the model (Context.emit_tables): device addresses + sizes"""
    kind: str  # "tab"
    w: int
    lw: int
    N: int
    nG: int
    lx: int
    Kt: int
    dlnKt: int
    nK: int
    scale: int
    nonneg: int


class SynKey(typing.NamedTuple):
    """an nh_synchrotron launch of the model (Context.emit_synchrotron)"""
    kind: str  # "syn"
    w: int
    lw: int
    B: int
    ldB: int
    N: int
    gd: int
    lx: int
    nG: int
    Ed: int
    nE: int


class _ByName:
    """read access by field name, ``plan["hs"]["split"]`` / ``plan.get("stage")``: how the plan was
    read while it was a dict, by scripts and tests that look at a loop's ``_plan``"""

    def __getitem__(self, name):
        try:
            return getattr(self, name)
        except AttributeError:
            raise KeyError(name) from None

    def get(self, name, default=None):
        return getattr(self, name, default)


@dataclasses.dataclass
class Emission:
    """a recorded emission launch; ``out``: the plan's own buffer for its spectrum (made at the
    first replay), ``keep``: the buffers the key's addresses point into"""
    kind: str
    key: tuple
    out: object
    N: int
    keep: tuple
    E_host: object = None


class Front(typing.NamedTuple):
    """what every launch of a fused loop starts from: the ensemble and the block of moves (device
    addresses), where the loop stands in that block (``pos``: the loop's OWN dict, which it keeps
    changing -- read at launch time), and the arguments of nh_step_front after the proposal's"""
    coords: int
    logp: int
    blk: int
    cursor: int
    pos: dict
    qT: int
    factors: int
    hist: int
    accepted: int
    naccepted: int
    sel: int
    ns: int
    ndim: int
    lo: int
    nloc: int
    packs: object
    npacks: int
    kind: int
    rows_ptr: int
    grids: object
    ngrids: int
    moments: object
    nmoments: int

    def step_front_args(self):
        return self[-8:]

    def launch_slice(self):
        """the slice a launch is told: baked in while a multi-step graph is captured, else the
        kernel reads the device cursor (-1)"""
        return self.pos["slice"] if self.pos["bake"] else -1


@dataclasses.dataclass
class OneLaunch(_ByName):
    """the created nh_half_step plan; ``keep`` and ``sorted`` hold the buffers it points into"""
    key: tuple
    handle: object
    keep: tuple
    threads: int
    blocks: int
    lds_bytes: int
    split: int
    tabs: list  # (what the resident loop sorts the columns of: Context.sorted_tables)
    sorted: list = dataclasses.field(default_factory=list)


@dataclasses.dataclass
class Stage:
    """a staged plan's first launch (StepPlan.stage_a)"""
    handle: object
    keep: tuple


@dataclasses.dataclass
class AcceptHook:
    """what the likelihood of a fused loop's evaluation is told (core.lnprobmodel): the walkers
    it is meant for, where the log-probabilities go, the accept that rides on its launch"""
    N: int
    total: object = None       # persistent result buffer (None: a fresh one per evaluation)
    mv: object = None          # nh_accept (None, sharded: the accept waits for the all-gather)
    used: bool = False
    blobs: object = None       # [(current array, width, history word)] the one launch may keep
    send_width: int = 0        # sharded: doubles per row { lnprob | blobs } of the all-gather
    total_rows: object = None  # ... and the send buffer of those rows
    rows_active: int = 0       # the row width the last launch wrote its results with
    blobs_in_kernel: bool = False

    def reset(self, total=None):
        """as made for a loop that is not one launch per half-step (its plan was turned down)"""
        self.__init__(self.N, total, self.mv)


class StepPlan(_ByName):
    def __init__(self):
        self.replaying = False  # (else: recording)
        for kind in KINDS:
            setattr(self, kind, [])  # [(key, value)]; emit: value is the Emission
        self.calls = []
        self.rewind()
        self.mega = self.staged = False
        self.prior_terms = self.front = self.hs = self.stage = None

    def rewind(self):
        """a new evaluation: every kind's next request is its first recorded one"""
        self.cursor = dict.fromkeys(KINDS, 0)

    def record(self, kind, key, value):
        if not self.replaying:
            getattr(self, kind).append((key, value))
        return value

    def record_emission(self, key, N, keep, E_host=None):
        key = (TabKey if key[0] == "tab" else SynKey)(*key)
        self.record("emit", key, Emission(key.kind, key, None, N, keep, E_host))

    def replayed(self, kind, key, label=None):
        """the next recorded (key, value) of this kind, whose key must begin with ``key``"""
        i, seq = self.cursor[kind], getattr(self, kind)
        if i >= len(seq) or seq[i][0][:len(key)] != key:
            raise _lib.NaimaHipError(_CHANGED % (label or kind))
        self.cursor[kind] = i + 1
        return seq[i]

    def emissions(self, kind=None):
        return [e for _, e in self.emit if kind is None or e.kind == kind]

    def destroy(self, ctx):
        for name in ("hs", "stage"):
            rec = getattr(self, name)
            if rec is not None and rec.handle is not None:
                _lib._lib.nh_half_step_destroy(ctx.h, rec.handle)
                rec.handle = None
                setattr(self, name, None)

    # -- admission --------------------------------------------------------------------------
    def can_be_one_launch(self, nloc):
        """every launch the recorded model evaluation made is one nh_half_step absorbs, and
        its working set fits in one workgroup's LDS (sets ``staged``)"""
        if os.environ.get("NAIMA_AMD_MEGA", "1") == "0":
            return False
        allowed = {"nh_pack_rows", "nh_particle_weights_multi", "nh_integrate_tables",
                   "nh_synchrotron", "nh_lnprob"}
        (_, _, _, grids), bufs = self.weights[0]
        nodes = [g[5] for g in grids]  # (e, x, ln e, lx, scale, nG)
        wptr = {wk.ptr: g for g, (wk, _) in enumerate(bufs)}
        moments, emit, syn = self.moments, self.emissions(), self.emissions("syn")
        ntab, nsyn = len(emit) - len(syn), len(syn)
        # A model that takes its synchrotron spectrum twice with launches of other kernels in
        # between -- the SSC seed of examples/CrabNebula_SynSSC.py:29-45: Synchrotron.flux at the
        # seed's energies, a linear combination, the seed integral (sixteen walkers per wave: not
        # a one-workgroup-per-walker job), Synchrotron.flux at the data's -- runs as TWO launches
        # of the half-step kernel around those (stage_a): ``staged``
        between = {"nh_lincomb", "nh_ic_seed_walkers_tab", "nh_ic_seed_walkers"}
        staged = nsyn == 2 and bool(set(self.calls) & between)
        if staged:
            if os.environ.get("NAIMA_AMD_STAGED", "1") == "0" or emit[0].kind != "syn" or \
                    syn[0].key[1:9] != syn[1].key[1:9] or \
                    any(e.E_host is None for e in syn) or moments:
                return False
            allowed = allowed | between
            nsyn = 1
        if not set(self.calls) <= allowed or not emit or ntab > 4 or nsyn > 1:
            return False
        if self.calls.count("nh_lnprob") != 1:
            return False
        # every integrate call is either a recorded single-row reduction or an emission table
        if self.calls.count("nh_integrate_tables") != ntab + len(moments) or \
                self.calls.count("nh_synchrotron") != (2 if staged else nsyn):
            return False
        lds = 88 + 3 * sum(nodes) + sum(2 * nodes[wptr[key[0]]] for key, _ in moments)
        items = nspec = 0
        for e in emit:
            k = e.key
            if e.N != nloc or k.w not in wptr:
                return False
            if e.kind == "tab":
                items += ((k.nK + 63) // 64) * ((k.nG - 1 + 31) // 32)
                nspec += k.nK
            elif not staged:
                lds += 3 * k.nG + 4 * k.nE + 1 + 32 * k.nE
                nspec += k.nE
        lds += min(items, 96) * 64 + nspec
        if staged:  # its other launch: one synchrotron component over both sets of energies
            nG, n1, nEa = syn[0].key.nG, syn[0].key.nE, syn[0].key.nE + syn[1].key.nE
            cd = max(1, min(32, (40 * 1024) // (8 * nEa)))
            lds = max(lds, 88 + 6 * nG + (5 + cd) * nEa + 8 * n1)
        if 8 * lds > 140 * 1024:
            return False
        self.staged = staged
        return True

    # -- the nh_half_step launches ----------------------------------------------------------
    def _desc_front(self, d):
        """the part of an nh_hs_desc every plan of a device loop shares: the ensemble, the block of
        moves, the parameter packs, the grids (returns {weights pointer: grid index})"""
        f = self.front
        for name in ("coords", "logp", "blk", "cursor", "qT", "factors"):
            setattr(d, name, getattr(f, name))
        d.ns, d.ndim, d.lo, d.nloc = f.ns, f.ndim, f.lo, f.nloc
        for q in range(f.npacks):
            d.packs[q] = f.packs[q]
        d.npacks, d.kind, d.params = f.npacks, f.kind, f.rows_ptr
        wgrid = {}
        for g in range(f.ngrids):
            d.grids[g] = f.grids[g]
            wgrid[f.grids[g].w] = g
        d.ngrids = f.ngrids
        return wgrid

    def _desc_syn(self, wgrid, k, nE, ldo, n1, E, out, out2=None, ldo2=0):
        """the synchrotron component of a launch; a field that is a column of the particle
        distribution's parameter rows is read from there"""
        at = k.B - self.front.rows_ptr
        in_rows = k.ldB == _lib.NH_PD_NPAR and 0 <= at < 8 * _lib.NH_PD_NPAR
        return D.nh_hs_syn(wgrid[k.w], nE, ldo, at // 8 if in_rows else -1, k.ldB, n1, E,
                           None if in_rows else k.B, out, out2, ldo2, 0)

    def _create(self, ctx, d):
        h = _lib._dp()
        _lib._chk(_lib._lib.nh_half_step_create(ctx.h, C.addressof(d), C.byref(h)))
        return h

    def stage_a(self, ctx, key, N, nE):
        """A model that asks for its synchrotron spectrum TWICE -- at the energies of a seed photon
        field it then builds from it, and at the data's (examples/CrabNebula_SynSSC.py:29-45) --
        with launches of other kernels in between (the SSC seed integral batches sixteen WALKERS
        per wave: nothing a one-workgroup-per-walker launch can absorb): the half-step is two
        nh_half_step launches around them.  Stage A, launched where the model asks for the first
        spectrum: proposal -> packs -> weights (written to HBM for the kernels in between) ->
        ONE synchrotron component over both sets of energies, no accept.  Stage C is the plan's
        own launch (half_step): proposal, packs and weights again (a few microseconds),
        the table reductions, the spectra of the launches in between and stage A's from HBM,
        likelihood, accept."""
        ent = self.replayed("emit", key, "synchrotron")[1]
        e1, e2 = self.emissions("syn")
        f = self.front
        if self.stage is None:
            n1, n2 = e1.key.nE, e2.key.nE
            base = ctx.empty((N * (n1 + n2),))
            e1.out = _lib.DeviceArray(ctx, base.ptr, (N, n1), np.float64, 0)
            e2.out = _lib.DeviceArray(ctx, base.ptr + 8 * N * n1, (N, n2), np.float64, 0)
            Ecat = ctx.array(np.concatenate([e1.E_host, e2.E_host]))
            d = D.nh_hs_desc()
            wgrid = self._desc_front(d)
            d.hist = None
            d.do_accept, d.write_weights = 0, 1
            d.nmoms, d.ntab = 0, 0
            d.syn = self._desc_syn(wgrid, e1.key, n1 + n2, n1, n1, Ecat.ptr, base.ptr,
                                   base.ptr + 8 * N * n1, n2)
            # (a launch has a likelihood: this one's is of the first spectrum against columns of
            # ones and zeros, into a buffer nobody reads)
            ones, zeros = ctx.array(np.ones(n1)), ctx.array(np.zeros(n1))
            izero = ctx.array(np.zeros(n1, dtype=np.int32), dtype=np.int32)
            half = ctx.array(np.full(n1, 0.5))
            dummy = ctx.empty((N,))
            d.comps[0] = D.nh_comp(base.ptr, n1, 1.0)
            d.ncomp, d.nE = 1, n1
            d.conv, d.flux, d.err_lo, d.err_hi = ones.ptr, zeros.ptr, ones.ptr, ones.ptr
            d.ul, d.cl, d.lp, d.nterms = izero.ptr, half.ptr, None, 0
            # the prior of the recorded evaluation: a proposal it forbids is integrated by nobody
            # (its synchrotron spectrum is written as zeros, the seed field made of it is empty and
            # the SSC kernel packs such walkers out of its groups: k_ssc_order) -- as the plan's
            # own launch does for it
            if self.prior_terms is not None:
                terms, d.nterms = self.prior_terms
                for q in range(d.nterms):
                    d.terms[q] = terms[q]
            d.model_out, d.total, d.nblobs, d.send_width = None, dummy.ptr, 0, 0
            h = self._create(ctx, d)
            self.stage = Stage(h, (base, Ecat, ones, zeros, izero, half, dummy))
            # the span clock: this launch opens the half-step's span, the plan's own closes it
            _lib._chk(_lib._lib.nh_half_step_span(h, 1, 0))
            ctx.call("nh_half_step_begin_block", h, f.pos["slice"], 0)
        if ent is e1:
            ctx.call("nh_half_step_launch", self.stage.handle, f.launch_slice())
        return ent.out

    def half_step(self, ctx, hook, comps, ncomp, nE, conv, dd, lpd, terms, nterms, total, blobs=()):
        """the plan's nh_half_step launch: everything the recorded model evaluation asked
        for plus the likelihood of ``comps`` (created on first use, then checked and reused)"""
        if self.cursor["emit"] != len(self.emit):
            raise _lib.NaimaHipError("the model's launch sequence changed between evaluations "
                                     "(fewer emission components); run with use_graph=False")
        key = (bytes(C.string_at(C.addressof(comps), C.sizeof(comps))), ncomp, nE, conv.ptr,
               lpd.ptr if lpd is not None else 0,
               bytes(C.string_at(C.addressof(terms), C.sizeof(terms))) if nterms else b"",
               total.ptr)
        f = self.front  # filled in by the device loop when it chose this mode
        if self.hs is not None:
            if self.hs.key != key:
                raise _lib.NaimaHipError("the model's likelihood inputs changed between "
                                         "evaluations; run the sampler with use_graph=False")
            ctx.call("nh_half_step_launch", self.hs.handle, f.launch_slice())
            return
        d = D.nh_hs_desc()
        wgrid = self._desc_front(d)
        d.hist, d.accepted, d.naccepted, d.sel = f.hist, f.accepted, f.naccepted, f.sel
        d.do_accept, d.write_weights = int(hook.mv is not None), 0
        for q in range(f.nmoments):
            d.moms[q] = f.moments[q]
        d.nmoms = f.nmoments
        d.syn.grid = -1
        tabs = []
        for ent in self.emissions():
            k = ent.key
            if ent.kind == "tab":
                def interleaved(k=k):
                    kd = ctx.empty((2 * k.nG * k.nK,))
                    # (a non-negative table carries its log-ratios in units of lx)
                    ctx.call("nh_table_interleave", k.Kt, k.dlnKt, k.lx if k.nonneg else None,
                             k.nG, k.nK, kd)
                    return kd

                kdkey = ("kd", k.Kt, k.dlnKt, k.nG * k.nK, bool(k.nonneg))
                kd = ctx.table(kdkey, interleaved)
                ctx._pinned.add(kdkey)  # the plan points into it
                d.tab[len(tabs)] = D.nh_hs_table(wgrid[k.w], k.nK, k.nK, k.nonneg, kd.ptr, None,
                                                 k.scale or None, ent.out.ptr)
                tabs.append((k.Kt, k.dlnKt, k.nG, k.nK, k.lx, bool(k.nonneg)))
            elif not self.staged:
                # (a staged plan: stage A's launch has produced it, the likelihood reads it from HBM)
                d.syn = self._desc_syn(wgrid, k, k.nE, k.nE, 0, k.Ed, ent.out.ptr)
        d.ntab = len(tabs)
        for q in range(ncomp):
            d.comps[q] = comps[q]
        d.ncomp, d.nE = ncomp, nE
        d.conv, d.flux, d.err_lo, d.err_hi = conv.ptr, dd.flux.ptr, dd.elo.ptr, dd.ehi.ptr
        d.ul, d.cl = dd.ul.ptr, dd.cl.ptr
        d.lp = lpd.ptr if lpd is not None else None
        for q in range(nterms):
            d.terms[q] = terms[q]
        d.nterms = nterms
        d.model_out, d.total = None, total.ptr
        self._desc_blobs(d, hook, comps, ncomp, nE, blobs)
        h = self._create(ctx, d)
        thr, blk, lds, spl = _lib._i(), _lib._i(), _lib._ll(), _lib._i()
        _lib._chk(_lib._lib.nh_half_step_info(h, C.byref(thr), C.byref(blk), C.byref(lds)))
        _lib._chk(_lib._lib.nh_half_step_split(h, C.byref(spl)))
        if self.staged:  # (the span clock: stage A's launch has opened this half-step's span)
            _lib._chk(_lib._lib.nh_half_step_span(h, 0, 1))
        self.hs = OneLaunch(key, h, (conv, lpd, total, dd), thr.value, blk.value, lds.value,
                            spl.value, tabs)
        # where the step loop stands in the current block of moves
        ctx.call("nh_half_step_begin_block", h, f.pos["slice"], f.pos["steps"])
        ctx.call("nh_half_step_launch", h, -1)

    def _desc_blobs(self, d, hook, comps, ncomp, nE, blobs):
        """blobs the launch keeps itself (the device loop says where: hook.blobs); anything
        it cannot express leaves them to the separate staging / scatter launches"""
        from . import units as u
        f = self.front
        hook.blobs_in_kernel = False
        blobs = [b for b in blobs if not isinstance(b, (float, int))]  # (lnprob's constant NaN)
        dest = hook.blobs
        if not (dest and (hook.mv is not None or hook.send_width) and len(dest) == len(blobs) <= 4):
            return
        model_terms = [(int(comps[q].ptr), int(comps[q].ld), float(comps[q].scale))
                       for q in range(ncomp)]
        mouts = [f.moments[q].out for q in range(f.nmoments)]
        ent = []
        for (cur, m, hist_word), b in zip(dest, blobs):
            v = b.value if isinstance(b, u.Quantity) else b
            if isinstance(v, D.DMat) and v.colfac is None and v.shape[1] == nE == m and \
                    [(int(t[1]), int(t[2]), float(t[3])) for t in v.terms] == model_terms:
                ent.append(D.nh_hs_blob(0, 0, m, 0, D.lazy_const(1.0), cur, hist_word))
            elif isinstance(v, D.DVec) and m == 1 and v.stride == 1 and v.ptr in mouts:
                ent.append(D.nh_hs_blob(1, mouts.index(v.ptr), 1, 0, v.lazy(), cur, hist_word))
            else:
                return
        for q, e in enumerate(ent):
            d.blobs[q] = e
        d.nblobs = len(ent)
        d.send_width = hook.send_width if hook.mv is None else 0
        hook.rows_active = d.send_width
        hook.blobs_in_kernel = True
