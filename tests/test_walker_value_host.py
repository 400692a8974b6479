"""naima_amd/walker_value.py without a GPU or the library: the one classification of a
per-walker value (scalar, host array, device value), the one merge of walker counts and the one
"value -> nh_lazy + keep-alive" builder, on the stub context of test_lazy_host.

What is pinned are the answers every caller gave BEFORE there was one module -- the radiative
classes' ``_per_walker`` / ``_batch_of``, the EBL model's 1-D-only rule, pair absorption's
``None`` for "scalars everywhere" and its size-1-is-a-scalar rule -- and the bits their five
copies of the lazy builder handed to the kernels.  The ``nh_lazy`` fields and the uploaded bytes
below were taken by running those copies once on this stub (general launches, packed rows,
pair absorption and the cooling solve) and are written here as literals: a kernel argument that
changes in one bit changes a recorded step plan's key.
"""
import numpy as np
import pytest

import naima_amd.units as u
from naima_amd import models as M
from naima_amd import radiative as R
from naima_amd import walker_value as wv
from naima_amd.darray import DPars, DVec
from naima_amd.validator import validate_scalar_or_per_walker
from test_lazy_host import StubCtx


class Ctx(StubCtx):
    """the stub device, remembering what was uploaded"""

    def __init__(self):
        super().__init__()
        self.uploads = []

    def array(self, a):
        self.uploads.append(np.array(a, dtype=float))
        return super().array(a)


def dvec(ctx, n):
    x = np.linspace(0.5, 2.0, 2 * n).reshape(2, n)
    return DPars(ctx, StubCtx.array(ctx, x), 2, n)[0]


# the table of the issue: value -> (form, walkers, exactly one value per walker)
FORMS = {"scalar": (lambda c: 3.0, wv.SCALAR, 1, False),
         "one": (lambda c: np.ones(1), wv.HOST, 1, True),
         "host": (lambda c: np.ones(4), wv.HOST, 4, True),
         "2d": (lambda c: np.ones((2, 3)), wv.HOST, 2, False),
         "device": (lambda c: dvec(c, 4), wv.DEVICE, 4, True)}


@pytest.mark.parametrize("name", list(FORMS))
def test_classification_table(name):
    make, form, n, vector = FORMS[name]
    ctx = Ctx()
    for x in (make(ctx), make(ctx) * u.G):  # bare and as a Quantity
        assert wv.classify(x) == (form, n)
        assert wv.per_walker(x) is (form is not wv.SCALAR)
        assert wv.is_vector(x) is vector
        assert wv.counts([x]) == [n]
        assert wv.on_device([3.0, x]) is (form is wv.DEVICE)
        assert wv.is_batched([3.0, x]) is (form is not wv.SCALAR)
    q = make(ctx) * u.mG
    assert q.on_device is (form is wv.DEVICE)
    # pair absorption's and the cooling solve's value: a float, or a DVec with the unit folded
    if name == "2d":
        with pytest.raises(TypeError, match="non-empty 1-D array"):
            wv.resolve(ctx, q, "G", fold=True)
    else:
        v = wv.resolve(ctx, q, "G", fold=True)
        if n == 1:
            assert type(v) is float
        else:
            assert isinstance(v, DVec) and v.n == 4 and v.a == 1e-3


def _props(obj):
    return obj.batch_size, obj.is_batched, obj.on_device


# (batch_size, is_batched, on_device) per class and form, as before the module
PROPS = {
    "PowerLaw": {"scalar": (1, False, False), "one": (1, True, False), "host": (4, True, False),
                 "2d": (2, True, False), "device": (4, True, True)},
    "TableModel": {"scalar": (1, False, False), "one": (1, True, False),
                   "host": (4, True, False), "2d": (2, True, False), "device": (4, True, True)},
    # a batch of one in B or nh alone does not make the radiative model batched
    "Synchrotron": {"scalar": (1, False, False), "one": (1, False, False),
                    "host": (4, True, False), "2d": TypeError, "device": (4, True, True)},
    "PionDecayKelner06": {"scalar": (1, False, False), "one": (1, False, False),
                          "host": (4, True, False), "2d": (2, True, False),
                          "device": (4, True, True)},
}


def _build(cls, v):
    pd = M.PowerLaw(1.0 / u.eV, 1 * u.TeV, 2.0)
    if cls == "PowerLaw":
        return M.PowerLaw(v / u.eV, 1 * u.TeV, 2.0)
    if cls == "TableModel":
        return M.TableModel(np.logspace(0, 2, 8) * u.TeV, np.logspace(0, -4, 8) / u.eV,
                            amplitude=v)
    if cls == "Synchrotron":
        return R.Synchrotron(pd, B=v * u.G)
    return R.PionDecayKelner06(pd, nh=v / u.cm ** 3)


@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("cls", list(PROPS))
def test_public_properties(cls, name):
    v = FORMS[name][0](Ctx())
    want = PROPS[cls][name]
    if want is TypeError:
        with pytest.raises(TypeError, match="scalar or a 1-D batch"):
            _build(cls, v)
    else:
        assert _props(_build(cls, v)) == want


@pytest.mark.parametrize("name,want", [("scalar", (None, False)), ("one", (None, False)),
                                       ("host", (4, False)), ("2d", (None, False)),
                                       ("device", (4, True))])
def test_pair_absorption_properties(name, want):
    L = FORMS[name][0](Ctx()) * u.kpc
    pa = M.PairAbsorptionModel([["s", 30 * u.K, 1 * u.eV / u.cm ** 3]], L)
    assert (pa.batch_size, pa.on_device) == want


def test_ebl_takes_one_value_per_walker_only():
    assert M.EblAbsorptionModel(np.array([0.1, 0.2]))._batch
    assert M.EblAbsorptionModel(dvec(Ctx(), 4))._batch
    with pytest.raises(TypeError, match="redshift should be a scalar"):
        M.EblAbsorptionModel(np.full((2, 3), 0.1))


def test_merge_errors_keep_their_texts():
    three, four = np.ones(3), np.ones(4)
    with pytest.raises(ValueError, match=r"^inconsistent walker-batch sizes in PowerLaw: 3 vs 4$"):
        M.PowerLaw(three / u.eV, 1 * u.TeV, 2.0 * four).batch_size
    syn = R.Synchrotron(M.PowerLaw(three / u.eV, 1 * u.TeV, 2.0), B=four * u.G)
    with pytest.raises(ValueError, match=r"^inconsistent walker-batch sizes: 3 vs 4$"):
        syn.batch_size
    pa = M.PairAbsorptionModel([["s", 30 * u.K, four * u.eV / u.cm ** 3]], three * u.kpc)
    with pytest.raises(ValueError, match=r"^inconsistent walker-batch sizes: 3 vs 4$"):
        pa.batch_size
    with pytest.raises(ValueError,
                       match=r"^inconsistent walker-batch sizes in CooledElectrons: 3 vs 4$"):
        M.CooledElectrons(M.PowerLaw(1e36 / u.eV / u.s, 1 * u.TeV, 2.0), three * u.uG,
                          four * u.yr, seed_photon_fields=())
    assert wv.merge([1, 4, 1, 4]) == 4 and wv.merge([]) == 1 and wv.merge([1, 1]) == 1
    assert wv.merge([None, None], broadcast_one=False) is None
    # pair absorption's contract: a device value of one walker does not go with four
    with pytest.raises(ValueError, match="1 vs 4"):
        wv.merge([1, 4], broadcast_one=False)
    pa = M.PairAbsorptionModel([["s", 30 * u.K, four * u.eV / u.cm ** 3]],
                               dvec(Ctx(), 1) * u.kpc)
    with pytest.raises(ValueError, match="1 vs 4"):
        pa.batch_size


def test_a_device_value_of_the_wrong_length():
    ctx = Ctx()
    pd = M.PowerLaw(dvec(ctx, 4) / u.eV, 1 * u.TeV, 2.0)
    with pytest.raises(ValueError, match="parameter amplitude has 4 walkers, batch has 3"):
        pd.device_rows(ctx, 3)
    # the general launches leave the length to the kernel's caller
    z, keep = wv.lazy(ctx, dvec(ctx, 4) * u.GeV, N=3)
    assert keep.n == 4


def test_scalar_or_per_walker_validation():
    ctx = Ctx()
    for v in (np.ones(4), np.ones((2, 3)), dvec(ctx, 4)):  # only the physical type is checked
        assert validate_scalar_or_per_walker("nh", v / u.cm ** 3, "number density").unit
        with pytest.raises(TypeError, match="nh should be given in units of number density"):
            validate_scalar_or_per_walker("nh", v * u.G, "number density")
    with pytest.raises(ValueError, match="nh value is NaN or Inf"):  # a scalar: as the reference
        validate_scalar_or_per_walker("nh", np.nan / u.cm ** 3, "number density")
    with pytest.raises(ValueError, match="nh value is NaN or Inf"):
        R.PionDecay(M.PowerLaw(1.0 / u.eV, 1 * u.TeV, 2.0), nh=np.inf / u.cm ** 3)


# ---- the lazy builder: (ptr != 0, stride, a, b, c, tf) and the uploaded doubles per policy ----
def fields(z):
    return (bool(z.base), z.stride, z.a, z.b, z.c, z.tf)


def doubles(hexes):
    return [np.frombuffer(bytes.fromhex(h), dtype=float) for h in hexes]


PLAIN = (True, 1, 1.0, 1.0, 0.0, 0)
HOST3 = np.array([1.5, 2.5, 4.0])
AS_GIVEN = "000000000000f83f00000000000004400000000000001040"  # 1.5, 2.5, 4.0

# policy -> form -> (nh_lazy fields, uploads); N = 3, the device value is a plain DVec
POLICIES = {
    # the general launches and the packed rows: mG -> G on the host, broadcast, plain lazy
    "host-convert": (dict(unit="G"), u.mG, {
        "scalar": ((False, 0, 0.0025, 0.0, 0.0, 0), []),
        "one": (PLAIN, ["7b14ae47e17a643f" * 3]),  # 2.5 * 0.001, three times
        "host": (PLAIN, ["fa7e6abc7493583f7b14ae47e17a643ffca9f1d24d62703f"]),
        "device": ((True, 1, 0.001, 1.0, 0.0, 0), [])}),
    # Eemin / Eemax / Epmin / Epmax: in their own unit (the erg or GeV factor travels beside)
    "own-unit": (dict(unit=None), u.GeV, {
        "scalar": ((False, 0, 2.5, 0.0, 0.0, 0), []),
        "one": (PLAIN, ["0000000000000440" * 3]),
        "host": (PLAIN, [AS_GIVEN]),
        "device": (PLAIN, [])}),
    # pair absorption and the cooling solve: uploaded as given, uG -> G folded into ``a``;
    # a size-1 array is a float
    "fold": (dict(unit="G", fold=True), u.uG, {
        "scalar": ((False, 0, 2.4999999999999998e-06, 0.0, 0.0, 0), []),
        "one": ((False, 0, 2.4999999999999998e-06, 0.0, 0.0, 0), []),
        "host": ((True, 1, 1e-06, 1.0, 0.0, 0), [AS_GIVEN]),
        "device": ((True, 1, 1e-06, 1.0, 0.0, 0), [])}),
}


@pytest.mark.parametrize("form", ["scalar", "one", "host", "device"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_lazy_builder_bits(policy, form):
    kw, unit, want = POLICIES[policy]
    ctx = Ctx()
    dev = dvec(ctx, 3)
    x = {"scalar": 2.5, "one": np.array([2.5]), "host": HOST3, "device": dev}[form] * unit
    z, keep = wv.lazy(ctx, x, N=3, **kw)
    f, ups = want[form]
    assert fields(z) == f
    assert len(ctx.uploads) == len(ups)
    for got, ref in zip(ctx.uploads, doubles(ups)):
        assert got.tobytes() == ref.tobytes()
    if f[0]:  # a pointer: the buffer is kept alive, and it is the one uploaded (or the DVec's)
        assert keep.ptr == z.base
        assert keep.ptr == (dev.ptr if form == "device" else ctx.bufs[-1].ptr)
    else:
        assert keep is None and z.base is None


def test_lazy_builder_in_the_packed_rows_and_pair_absorption_units():
    # kpc -> cm and eV/cm3 -> erg/cm3 as pair absorption folds them
    ctx = Ctx()
    assert wv.resolve(ctx, 2.5 * u.kpc, "cm", fold=True) == 7.714193953728418e+21
    v = wv.resolve(ctx, HOST3 * u.kpc, "cm", fold=True)
    assert (v.a, v.b, v.c, v.tf, v.n) == (3.0856775814913673e+21, 1.0, 0.0, 0, 3)
    v = wv.resolve(ctx, HOST3 * u.eV / u.cm ** 3, "erg/cm3", fold=True)
    assert (v.a, v.b, v.c, v.tf, v.n) == (1.602176634e-12, 1.0, 0.0, 0, 3)
    # the amplitude column of the packed rows: 1/TeV -> 1/eV on the host
    ctx = Ctx()
    cols = []
    ctx.pack_rows = lambda c, ncols, N: cols.extend(fields(c[j]) for j in range(ncols))
    M.PowerLaw(np.array([1.0, 2.0, 3.0]) / u.TeV, 1 * u.TeV, 2.0).device_rows(
        ctx, 3, amplitude_to=u.Unit("1/eV"))
    assert cols == [PLAIN, (False, 0, 1e12, 0.0, 0.0, 0), (False, 0, 2.0, 0.0, 0.0, 0),
                    (False, 0, 0.0, 0.0, 0.0, 0), (False, 0, 1.0, 0.0, 0.0, 0)] \
        + [(False, 0, 0.0, 0.0, 0.0, 0)] * 3
    assert [a.tobytes() for a in ctx.uploads] == [
        r.tobytes() for r in doubles(["11ea2d819997713d11ea2d819997813d1adfc44166638a3d"])]
