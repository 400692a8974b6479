"""The recorded step plan (naima_amd/step_plan.py) without a GPU and without the library: what a
model evaluation asks of the context is recorded and replayed, a changed sequence is refused,
which recorded plans may become ONE launch per half-step, and the accept hook's reset."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from naima_amd import _lib
from naima_amd.darray import nh_comp, nh_grid, nh_hs_desc, nh_lazy, nh_moment, nh_pack, nh_prior
from naima_amd.step_plan import AcceptHook, Front, StepPlan


class Buf:
    """stands in for a device array: all a plan reads of one is its address"""

    def __init__(self, ptr):
        self.ptr = ptr


class _Library:
    """stands in for the loaded library: every entry point succeeds; the descriptors that
    nh_half_step_create was given are kept"""

    def __init__(self):
        self.descs = []

    def nh_half_step_create(self, h, addr, out):
        self.descs.append(nh_hs_desc.from_buffer_copy(C.string_at(addr, C.sizeof(nh_hs_desc))))
        return 0

    def __getattr__(self, name):
        return lambda *args: 0


class _Context(_lib.Context):
    """a context's requests and launches with no device behind them"""

    def __init__(self):
        self.h = None
        self._plan = self._accept_hook = None
        self._in_eval = True
        self._deferred = []
        self._pinned = set()
        self.capturing = False
        self.made = 0

    def empty(self, shape, dtype=np.float64):
        self.made += 1
        return Buf(0x100000 * self.made)

    def array(self, host, dtype=np.float64):
        return self.empty(np.shape(host))

    def table(self, key, build):
        return build()


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _Library())
    return _Context()


def _cols(a):
    cols = (nh_lazy * 8)()
    cols[0].a = a
    return cols


ROWS, GRIDS = Buf(0x10), [tuple(Buf(0x20 + 8 * g + j) for j in range(4)) + (1.0, 50 + g)
                          for g in range(2)]
COLS = [_cols(1.0), _cols(2.0), _cols(3.0)]
# (the context's entry point, its arguments, the kind named when the sequence has changed)
W, LW, LX, KT, DKT, SC, GD, ED = (Buf(0x1000 + 8 * j) for j in range(8))
REQUESTS = [
    ("pack_rows", (COLS[0], 8, 64), "packs"),
    ("pack_rows", (COLS[1], 3, 64), "packs"),
    ("weights_multi", (1, ROWS, 64, GRIDS), "weights"),
    ("moment", (W, LW, 64, 50, LX, KT, DKT), "moments"),
    ("emit_tables", (W, LW, 64, 50, LX, KT, DKT, 40, SC, 1, False), "tables"),
    ("emit_tables", (W, LW, 64, 50, LX, DKT, KT, 30, None, 0, False), "tables"),
    ("emit_synchrotron", (W, LW, 0x18, 8, 64, GD, LX, 50, ED, 20), "synchrotron"),
    ("plan_buffer", (("seed-integral", "SSC", 64, 20), (64, 20)), "seed-integral"),
]
# the same request with one argument changed, by kind
CHANGED = {"packs": (COLS[2], 8, 64), "weights": (2, ROWS, 64, GRIDS),
           "moments": (W, LW, 64, 51, LX, KT, DKT),
           "tables": (W, LW, 64, 50, LX, KT, DKT, 41, SC, 1, False),
           "synchrotron": (W, LW, 0x18, 8, 64, GD, LX, 50, ED, 21),
           "seed-integral": (("seed-integral", "SSC", 64, 21), (64, 21))}


def _flat(x):
    """the objects a request returned, in order (emit_tables: (out, planes); weights: pairs)"""
    if isinstance(x, (list, tuple)):
        return [z for y in x for z in _flat(y)]
    return [x]


def _recorded(ctx):
    plan = ctx._plan = StepPlan()
    first = [getattr(ctx, name)(*args) for name, args, _ in REQUESTS]
    plan.replaying = plan.mega = True
    return plan, first


def test_a_recorded_sequence_is_replayed_with_its_own_buffers(ctx):
    plan, first = _recorded(ctx)
    assert [len(getattr(plan, k)) for k in ("packs", "weights", "moments", "emit", "bufs")] == \
        [2, 1, 1, 3, 1]
    assert plan.calls == ["nh_pack_rows", "nh_pack_rows", "nh_particle_weights_multi",
                          "nh_integrate_tables", "nh_integrate_tables", "nh_integrate_tables",
                          "nh_synchrotron"]
    tab, _, syn = plan.emissions()
    assert (tab.key.nG, tab.key.nK, tab.key.w, syn.key.nE, syn.key.B) == (50, 40, W.ptr, 20, 0x18)
    assert tab.keep == (W, LW, LX, KT, DKT, SC) and syn.keep == (W, LW, GD, LX, ED)
    made, calls, runs = ctx.made, list(plan.calls), []
    for _ in range(2):
        plan.rewind()
        runs.append([getattr(ctx, name)(*args) for name, args, _ in REQUESTS])
    for a, b in zip(_flat(runs[0]), _flat(runs[1])):
        assert a is b
    # packs, weights, the moment and the plan's buffer: the recorded evaluation's own; the
    # spectra of a one-launch plan: buffers of the plan, made once
    for k in (0, 1, 2, 3, 7):
        assert all(a is b for a, b in zip(_flat(runs[0][k]), _flat(first[k])))
    assert ctx.made == made + 3 and plan.calls == calls
    plan.rewind()
    grids, bufs = ctx.weights_replay(1, ROWS, 64)
    assert bufs is first[2] and [g[5] for g in grids] == [50, 51]


@pytest.mark.parametrize("k", range(len(REQUESTS)), ids=[r[0] + str(i) for i, r in enumerate(REQUESTS)])
@pytest.mark.parametrize("how", ["changed", "one-more"])
def test_a_changed_sequence_is_refused(ctx, k, how):
    plan, _ = _recorded(ctx)
    plan.rewind()
    if how == "one-more":
        for name, args, _ in REQUESTS:
            getattr(ctx, name)(*args)
    else:
        for name, args, _ in REQUESTS[:k]:
            getattr(ctx, name)(*args)
    name, args, kind = REQUESTS[k]
    with pytest.raises(_lib.NaimaHipError) as err:
        getattr(ctx, name)(*(CHANGED[kind] if how == "changed" else args))
    text = str(err.value)
    assert "launch sequence changed" in text and "(%s)" % kind in text and "use_graph=False" in text
    if name == "weights_multi":
        plan.cursor["weights"] = 0 if how == "changed" else 1
        with pytest.raises(_lib.NaimaHipError, match=r"launch sequence changed.*\(weights\).*use_graph=False"):
            ctx.weights_replay(*(CHANGED[kind] if how == "changed" else args)[:3])


def _front(weights, pos, rows_ptr=ROWS.ptr):
    """a Front over the recorded weights launch's grids, its first grid's weights at W"""
    gd = (nh_grid * 4)()
    for g, (wk, lwk) in enumerate(weights[0][1]):
        gd[g] = nh_grid(1, 2, W.ptr if g == 0 else wk.ptr, lwk.ptr, 1.0, 50 + g, 0, 3, 4)
    return Front(0xc0, 0xc1, 0xc2, 0xc3, pos, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 32, 3, 0, 64,
                 (nh_pack * 4)(), 2, 1, rows_ptr, gd, 2, (nh_moment * 4)(), 1)


def test_the_plans_launch_is_described_once_and_reads_the_loops_position(ctx):
    plan, _ = _recorded(ctx)
    pos = dict(slice=3, steps=7, bake=False)
    plan.front = _front(plan.weights, pos)
    hook = AcceptHook(64, mv=object(), total=Buf(0xd0))
    dd = types.SimpleNamespace(**{k: Buf(0xe0 + j) for j, k in enumerate(("flux", "elo", "ehi", "ul", "cl"))})
    comps, launches = (nh_comp * 8)(), []
    ctx.call = lambda name, *args: launches.append((name,) + args[1:])

    def evaluate():
        plan.rewind()
        for name, args, _ in REQUESTS:
            getattr(ctx, name)(*args)
        plan.half_step(ctx, hook, comps, 2, 20, Buf(0xf0), dd, None, None, 0, hook.total)

    evaluate()
    (d,) = _lib._lib.descs
    assert (d.coords, d.qT, d.hist, d.sel, d.ns, d.ndim, d.nloc) == (0xc0, 0xc4, 0xc6, 0xc9, 32, 3, 64)
    assert (d.npacks, d.kind, d.params, d.ngrids, d.nmoms, d.ntab, d.do_accept) == (2, 1, ROWS.ptr, 2, 1, 2, 1)
    tab, tab2, syn = plan.emissions()
    assert (d.tab[0].grid, d.tab[0].nK, d.tab[0].out, d.tab[1].nK, d.tab[1].scale) == \
        (0, 40, tab.out.ptr, 30, None)
    # (the field at 0x18: eight bytes into the parameter rows at ROWS, their column 1)
    assert (d.syn.grid, d.syn.nE, d.syn.bcol, d.syn.B, d.syn.out) == (0, 20, 1, None, syn.out.ptr)
    assert (plan.hs.tabs, plan.hs.keep[2]) == ([(KT.ptr, DKT.ptr, 50, 40, LX.ptr, True),
                                                (DKT.ptr, KT.ptr, 50, 30, LX.ptr, False)], hook.total)
    assert launches[-2:] == [("nh_half_step_begin_block", 3, 7), ("nh_half_step_launch", -1)]
    pos.update(slice=5, bake=True)  # (the loop, capturing a graph of several steps)
    evaluate()
    assert len(_lib._lib.descs) == 1 and launches[-1] == ("nh_half_step_launch", 5)
    plan.rewind()
    with pytest.raises(_lib.NaimaHipError, match="fewer emission components"):
        plan.half_step(ctx, hook, comps, 2, 20, Buf(0xf0), dd, None, None, 0, hook.total)
    plan.destroy(ctx)
    assert plan.hs is None


def test_a_staged_plans_first_launch(ctx):
    """one synchrotron component over both sets of energies, launched where the first spectrum is
    asked for; a field that is not a column of the parameter rows is read where it is"""
    plan = ctx._plan = StepPlan()
    k1 = ("syn", W.ptr, LW.ptr, 0x9000, 1, 64, GD.ptr, LX.ptr, 50, ED.ptr, 30)
    k2 = k1[:9] + (ED.ptr + 8, 20)
    plan.record("weights", (1, ROWS.ptr, 64, ()), [(W, LW), (KT, DKT)])
    plan.record_emission(k1, 64, keep=(), E_host=np.ones(30))
    plan.record_emission(k2, 64, keep=(), E_host=np.ones(20))
    plan.replaying = plan.mega = plan.staged = True
    plan.front = _front(plan.weights, dict(slice=4, steps=0, bake=False))
    plan.prior_terms = ((nh_prior * 16)(), 2)
    launches = []
    ctx.call = lambda name, *args: launches.append((name,) + args[1:])
    for _ in range(2):
        plan.rewind()
        a, b = plan.stage_a(ctx, k1, 64, 30), plan.stage_a(ctx, k2, 64, 20)
        assert (a.shape, b.shape, b.ptr - a.ptr) == ((64, 30), (64, 20), 8 * 64 * 30)
    (d,) = _lib._lib.descs
    assert (d.do_accept, d.write_weights, d.ntab, d.nmoms, d.nterms, d.ncomp, d.nE) == (0, 1, 0, 0, 2, 1, 30)
    assert (d.syn.nE, d.syn.n1, d.syn.bcol, d.syn.B, d.syn.out, d.syn.out2, d.syn.ldo2) == \
        (50, 30, -1, 0x9000, a.ptr, b.ptr, 20)
    assert launches == [("nh_half_step_begin_block", 4, 0), ("nh_half_step_launch", -1),
                        ("nh_half_step_launch", -1)]
    assert len(plan.stage.keep) == 7
    plan.destroy(ctx)
    assert plan.stage is None


# -- which recorded plans become one launch per half-step ------------------------------------
FRONT = ["nh_pack_rows", "nh_particle_weights_multi"]
SSC = FRONT + ["nh_synchrotron", "nh_lincomb", "nh_ic_seed_walkers_tab", "nh_synchrotron", "nh_lnprob"]
E_HOST = np.ones(3)


def _tab(nG, nK, grid=0, N=64):
    return ("tab", grid, N, nG, nK, None)


def _syn(nG, nE, grid=0, N=64, E_host=None, Ed=0):
    return ("syn", grid, N, nG, nE, E_host, Ed)


def raw_plan(nodes, emit, calls, moments=()):
    """the recorded lists of a plan whose weights launch is on grids of ``nodes`` nodes:
    (weights, moments, emissions as (kind, key, N, E_host), calls)"""
    grids = tuple((0x100 + g, 0x200 + g, 0x300 + g, 0x400 + g, 1.0, nG) for g, nG in enumerate(nodes))
    wp = [0x10000 * (g + 1) for g in range(len(nodes) + 1)]  # (the last: nobody's weights)
    weights = [((1, 0x5000, 64, grids), [(Buf(wp[g]), Buf(wp[g] + 8)) for g in range(len(nodes))])]
    moms = [((wp[g], wp[g] + 8, 64, nodes[g], 0x400 + g, 0x600, 0x608), Buf(0x700 + q))
            for q, g in enumerate(moments)]
    ems = []
    for e in emit:
        kind, g, N, nG, n = e[:5]
        if kind == "tab":
            key = ("tab", wp[g], wp[g] + 8, N, nG, 0x400 + g, 0x800, 0x808, n, 0x900, 1)
        else:
            key = ("syn", wp[g], wp[g] + 8, 0x5018, 8, N, 0xa00, 0x400 + g, nG, 0xb00 + e[6], n)
        ems.append((kind, key, N, e[5]))
    return weights, moms, ems, list(calls)


# (id, raw_plan's arguments, environment, nloc) -> (admitted, staged) as DeviceLoop._can_be_one_launch
# of commit c2c7510 answers for the same recorded lists (called unbound on
# types.SimpleNamespace(nloc=...) and a plan dict; "staged" is what it left in the dict)
ADMISSION = [
    ("one-table", ([100], [_tab(100, 40)], FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (True, False)),
    ("five-tables", ([100], [_tab(100, 40)] * 5, FRONT + ["nh_integrate_tables"] * 5 + ["nh_lnprob"]),
     {}, 64, (False, False)),
    ("syn-and-table", ([100], [_syn(100, 30), _tab(100, 40)],
                       FRONT + ["nh_synchrotron", "nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (True, False)),
    ("foreign-launch", ([100], [_tab(100, 40)],
                        FRONT + ["nh_integrate_tables", "nh_ebl_apply", "nh_lnprob"]), {}, 64,
     (False, False)),
    ("two-lnprob", ([100], [_tab(100, 40)], FRONT + ["nh_integrate_tables", "nh_lnprob", "nh_lnprob"]),
     {}, 64, (False, False)),
    ("other-N", ([100], [_tab(100, 40, N=32)], FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (False, False)),
    ("not-the-plans-weights", ([100], [_tab(100, 40, grid=1)],
                               FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64, (False, False)),
    ("mega-off", ([100], [_tab(100, 40)], FRONT + ["nh_integrate_tables", "nh_lnprob"]),
     {"NAIMA_AMD_MEGA": "0"}, 64, (False, False)),
    ("table-and-moment", ([100, 60], [_tab(100, 40)], FRONT + ["nh_integrate_tables"] * 2 + ["nh_lnprob"],
                          [1]), {}, 64, (True, False)),
    ("unrecorded-integrate", ([100], [_tab(100, 40)], FRONT + ["nh_integrate_tables"] * 2 + ["nh_lnprob"]),
     {}, 64, (False, False)),
    # 88 + 3 nG + 64 min(items, 96) + nK doubles of LDS against 140 KiB / 8 = 17920
    ("lds-17919", ([3800], [_tab(3800, 287)], FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (True, False)),
    ("lds-17920", ([3800], [_tab(3800, 288)], FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (True, False)),
    ("lds-17921", ([3800], [_tab(3800, 289)], FRONT + ["nh_integrate_tables", "nh_lnprob"]), {}, 64,
     (False, False)),
    ("two-syn-unstaged", ([100], [_syn(100, 30, E_host=E_HOST), _syn(100, 20, E_host=E_HOST, Ed=8)],
                          FRONT + ["nh_synchrotron", "nh_synchrotron", "nh_lnprob"]), {}, 64,
     (False, False)),
    ("staged", ([100], [_syn(100, 30, E_host=E_HOST), _syn(100, 20, E_host=E_HOST, Ed=8)], SSC), {}, 64,
     (True, True)),
    ("staged-with-table", ([100], [_syn(100, 30, E_host=E_HOST), _tab(100, 40),
                                   _syn(100, 20, E_host=E_HOST, Ed=8)],
                           SSC[:-1] + ["nh_integrate_tables", "nh_lnprob"]), {}, 64, (True, True)),
    ("staged-off", ([100], [_syn(100, 30, E_host=E_HOST), _syn(100, 20, E_host=E_HOST, Ed=8)], SSC),
     {"NAIMA_AMD_STAGED": "0"}, 64, (False, False)),
    ("staged-moment", ([100], [_syn(100, 30, E_host=E_HOST), _syn(100, 20, E_host=E_HOST, Ed=8)],
                       SSC[:-1] + ["nh_integrate_tables", "nh_lnprob"], [0]), {}, 64, (False, False)),
    ("staged-no-host-energies", ([100], [_syn(100, 30, E_host=E_HOST), _syn(100, 20, Ed=8)], SSC), {},
     64, (False, False)),
    ("staged-other-grid", ([100, 100], [_syn(100, 30, E_host=E_HOST),
                                        _syn(100, 20, grid=1, E_host=E_HOST, Ed=8)], SSC), {}, 64,
     (False, False)),
    ("staged-table-first", ([100], [_tab(100, 40), _syn(100, 30, E_host=E_HOST),
                                    _syn(100, 20, E_host=E_HOST, Ed=8)],
                            SSC[:-1] + ["nh_integrate_tables", "nh_lnprob"]), {}, 64, (False, False)),
    ("staged-lds", ([2000], [_syn(2000, 600, E_host=E_HOST), _syn(2000, 400, E_host=E_HOST, Ed=8)], SSC),
     {}, 64, (False, False)),
]


@pytest.mark.parametrize("case", ADMISSION, ids=[c[0] for c in ADMISSION])
def test_which_recorded_plans_become_one_launch(monkeypatch, case):
    """the verdicts and the ``staged`` flag are those of commit c2c7510's
    DeviceLoop._can_be_one_launch for the same recorded lists"""
    _, args, env, nloc, (admitted, staged) = case
    for name in ("NAIMA_AMD_MEGA", "NAIMA_AMD_STAGED"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    weights, moments, emissions, calls = raw_plan(*args)
    plan = StepPlan()
    plan.record("weights", *weights[0])
    for key, out in moments:
        plan.record("moments", key, out)
    for kind, key, N, E_host in emissions:
        plan.record_emission(key, N, keep=(), E_host=E_host)
    plan.calls = calls
    assert plan.can_be_one_launch(nloc) == admitted
    assert plan.staged == staged


def test_the_hook_of_a_plan_that_was_turned_down_is_a_fresh_one():
    for total, mv in ((None, object()), (Buf(8), None)):  # (one rank; sharded)
        hook = AcceptHook(64, total=total, mv=mv)
        fresh = dataclasses.replace(hook)
        # what the loop and the plan's launch fill in once the plan is one launch per half-step
        hook.used, hook.total, hook.blobs = True, Buf(16), [(0x10, 3, 0x20)]
        hook.send_width, hook.total_rows, hook.rows_active, hook.blobs_in_kernel = 4, Buf(24), 4, True
        assert hook != fresh
        hook.reset(total=total)
        assert hook == fresh
        assert [f.name for f in dataclasses.fields(hook)] == [
            "N", "total", "mv", "used", "blobs", "send_width", "total_rows", "rows_active",
            "blobs_in_kernel"]


def test_the_records_keep_the_recorded_tuples():
    """an emission's key is the tuple the context builds, with names: equal to it, and the staged
    plan's comparison of two synchrotron keys is a slice of it"""
    plan = StepPlan()
    key = ("syn", 1, 2, 3, 8, 64, 4, 5, 100, 6, 30)
    plan.record_emission(key, 64, keep=())
    plan.record_emission(key[:9] + (7, 20), 64, keep=())
    a, b = plan.emissions("syn")
    assert a.key == key and a.key[1:9] == b.key[1:9] and a.key != b.key
    assert (a.key.kind, a.key.B, a.key.ldB, a.key.nG, a.key.Ed, a.key.nE) == ("syn", 3, 8, 100, 6, 30)
    assert plan.cursor == dict(packs=0, weights=0, moments=0, emit=0, bufs=0)


def test_a_plan_can_still_be_read_by_field_name():
    """as while it was a dict: ``plan["hs"]["split"]``, ``plan.get("stage")``"""
    from naima_amd.step_plan import OneLaunch
    plan = StepPlan()
    assert plan["hs"] is None and plan.get("stage") is None and plan.get("staged") is False
    assert plan["calls"] is plan.calls and plan.get("no such field", 7) == 7
    plan.hs = OneLaunch((), object(), (), 256, 64, 1024, 2, tabs=[])
    assert (plan["hs"]["split"], plan["hs"]["threads"], plan["hs"].get("sorted")) == (2, 256, [])
    with pytest.raises(KeyError):
        plan["no such field"]
