"""naima_amd.plot on the host: imports without matplotlib, naima's rank and sample-count rules,
the seeded draws, find_ML / _process_blob against the reference (tests/golden/bands.npz, made by
gen_golden_bands.py) and the argument errors that come before any device work."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FU = "1/(cm2 s eV)"


def bands():
    return np.load(os.path.join(ROOT, "tests", "golden", "bands.npz"))


class Stub:
    """a sampler as naima_amd stores one: dense blob histories + blob_units"""

    def __init__(self, z, name, modelfn=None):
        from naima_amd import units as u
        self._chain, self._lp = z[name + "__chain"], z[name + "__log_prob"]
        self._blobs = [z[name + "__blob0"], z[name + "__blob1"]]
        self.blob_units = [u.Unit(FU), u.Unit("erg")]
        m = z[name + "__energy_TeV"].size
        self.data = {"energy": u.Quantity(z[name + "__energy_TeV"], "TeV"),
                     "flux": u.Quantity(np.ones(m), FU)}
        self.labels = ["log10(norm)", "alpha", "beta"]
        self.acceptance_fraction = np.full(self._chain.shape[1], 0.3)
        if modelfn is not None:
            self.modelfn = modelfn

    def get_chain(self, flat=False):
        return self._chain.reshape(-1, self._chain.shape[-1]) if flat else self._chain

    def get_log_prob(self, flat=False):
        return self._lp.reshape(-1) if flat else self._lp

    def get_blobs(self):
        return list(self._blobs)


def test_plot_module_imports_without_matplotlib():
    code = ("import sys; import naima_amd, naima_amd.plot as P; "
            "from naima_amd.plot import _calc_CI, _calc_ML, find_ML, _read_or_calc_samples; "
            "assert 'matplotlib' not in sys.modules, 'matplotlib imported'; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_exports():
    import naima_amd as na
    for name in ("plot_chain", "plot_fit", "plot_data", "plot_blob", "plot_corner",
                 "save_diagnostic_plots"):
        assert callable(getattr(na, name)), name
    from naima_amd import plot
    assert plot.__all__ == ["plot_chain", "plot_fit", "plot_data", "plot_blob", "plot_corner"]
    # the analysis-time find_ML keeps its 2-tuple
    z = bands()
    ML, MLp = na.find_ML(Stub(z, "logn"))
    assert np.ndim(MLp) == 1


def test_rank_rule_is_scipys():
    from scipy import stats

    from naima_amd.plot import _band_ranks, _min_samples
    for M in (2, 7, 101, 320, 512 * 1000, 2 ** 21):
        for confs in ([3, 1], [3, 1, 0.5], [2], [1.5, 4]):
            want = []
            for c in confs:
                want += [int(stats.norm.cdf(-c) * (M - 1)), int(stats.norm.cdf(c) * (M - 1))]
            assert _band_ranks(M, confs) == want
    assert _min_samples([3, 1]) == 100
    assert _min_samples([1]) == int(1 / stats.norm.cdf(-1) + 1) == 7
    assert _min_samples([2, 1]) == 44


def test_seeded_draws_are_the_global_stream():
    from naima_amd.plot import _draw
    z = bands()
    s = Stub(z, "logn")
    flat = s.get_chain(flat=True)
    for seed, n in ((0, 5), (12345, 100), (7, 4096)):
        np.random.seed(seed)
        want = flat[np.random.randint(len(flat), size=n)]
        assert np.array_equal(_draw(s, n, False, seed), want)
    np.random.seed(3)
    want = s.get_chain()[-1][np.random.randint(s.get_chain().shape[1], size=9)]
    assert np.array_equal(_draw(s, 9, True, 3), want)


@pytest.mark.parametrize("name", ["logn", "edge"])
def test_process_blob_and_find_ML_match_the_reference(name):
    from naima_amd import plot as P
    z = bands()
    s = Stub(z, name)
    S, W, m = z[name + "__blob0"].shape
    for last in (0, 1):
        tag = "%s__last%d" % (name, last)
        mx, model = P._process_blob(s, 0, last_step=bool(last))
        assert np.array_equal(mx.to("TeV").value, z[tag + "__pb0_x"])
        want = z[name + "__blob0"][-1] if last else z[name + "__blob0"].reshape(-1, m)
        assert np.array_equal(model.to(FU).value, want, equal_nan=True)
        mx, model = P._process_blob(s, 1, last_step=bool(last))
        assert mx is None
        assert np.array_equal(model.to("erg").value, z[tag + "__pb1"])
    for fn in (P.find_ML, P._calc_ML):
        ML, MLp, MLerr, (mx, my) = fn(s, 0)
        assert ML == z[name + "__ML"]
        assert np.array_equal(MLp, z[name + "__MLp"])
        assert np.array_equal(np.array(MLerr), z[name + "__MLerr"])
        assert np.array_equal(mx.to("TeV").value, z[name + "__ML_x"])
        assert np.array_equal(my.to(FU).value, z[name + "__ML_model"], equal_nan=True)


def test_malformed_blobs_and_e_range_raise():
    from naima_amd import plot as P
    from naima_amd import units as u
    z = bands()
    s = Stub(z, "logn")
    s._blobs.append(np.zeros(z["logn__blob0"].shape[:2] + (3,)))  # 3 values, 9 energies
    s.blob_units.append(None)
    for fn in (lambda: P._process_blob(s, 2), lambda: P.find_ML(s, 2),
               lambda: P._process_blob(s, 5)):
        with pytest.raises(TypeError, match="Model . has wrong blob format"):
            fn()
    # e_range without a model function says why
    with pytest.raises(ValueError, match="modelfn"):
        P._calc_CI(s, 0, e_range=[1 * u.GeV, 10 * u.TeV])
    s.modelfn = lambda p, d: None
    with pytest.raises(TypeError):  # not an energy
        P._calc_CI(s, 0, e_range=[1 * u.cm, 10 * u.cm])
    with pytest.raises(ValueError):  # three numbers
        P._read_or_calc_samples(s, 0, e_range=u.Quantity([1.0, 2.0, 3.0], "TeV"))
    with pytest.raises(ValueError):
        P._calc_ML(s, 0, e_range=u.Quantity([0.0, 2.0], "TeV"))


def test_read_run_attaches_the_model_function(tmp_path):
    from naima_amd import plot as P
    from naima_amd import units as u
    from naima_amd.analysis import read_run, save_run
    z = bands()
    s = Stub(z, "logn")
    s.data = None  # (no data table: the saved run has chain, log-prob and blobs)
    fn = save_run(str(tmp_path / "run.npz"), s)

    def model(p, d):
        return d["energy"]

    r = read_run(fn, modelfn=model)
    assert r.modelfn is model
    r = read_run(fn)
    assert r.modelfn is None
    with pytest.raises(ValueError, match="read_run"):
        P._calc_CI(r, 0, e_range=[1 * u.GeV, 10 * u.TeV])


def test_select_kernels_hold_no_scratch():
    """nh_column_select's kernels keep everything in registers and LDS: no scratch in their
    resource reports, no scratch instruction in their bodies"""
    import re
    src = os.path.join(ROOT, "naima_amd", "csrc", "nh_select.hip")
    base = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
            "-mllvm", "-amdgpu-kernarg-preload-count=16"]
    out = subprocess.run(base + ["-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull],
                         capture_output=True, text=True).stderr
    blocks = re.split(r"remark: Function Name: ", out)[1:]
    sizes = {b.split()[0]: int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
             for b in blocks}
    mine = {k: v for k, v in sizes.items() if "k_sel_" in k}
    assert len(mine) == 4, sizes
    assert all(v == 0 for v in mine.values()), mine
    asm = subprocess.run(base + ["--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True).stdout
    bodies = re.findall(r"^(_Z\S*k_sel_\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    assert len(bodies) == 4
    for name, body in bodies:
        assert "scratch_" not in body, "%s touches scratch memory" % name
