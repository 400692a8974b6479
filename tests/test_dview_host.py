"""The typed device views without a GPU (naima_amd.dview): tuple parsing, view arithmetic and its
bounds on a stand-in buffer, and that a typed view is never reinterpreted."""
import subprocess
import sys

import numpy as np
import pytest

from test_rank_host import no_device  # noqa: F401  (the fixture)

from naima_amd import dview as V

PTR0 = 0x7f0000001000


class Buf:
    """what a view needs of a device array: an address, a size and a context"""

    def __init__(self, nbytes, ptr=PTR0):
        self.ptr, self.nbytes, self.ctx = ptr, nbytes, object()


def chain_783(logp=False):
    c = V.as_chain((Buf(7 * 24 * 8), 7, 8, 3))
    if logp:
        c = V.as_chain(c, logp=V.matrix_on(Buf(7 * 8 * 8, PTR0 + 0x10000), 7, 8))
    return c


def test_import_creates_no_gpu_context():
    code = ("import naima_amd.dview as V, naima_amd._lib as L; "
            "assert L._lib is None and not L._default, 'GPU touched'; "
            "assert V.DeviceMatrix and V.DeviceChain and V.as_matrix and V.as_chain; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_matrix_tuple_parsing(no_device):
    buf = Buf(9 * 5 * 8)
    m = V.as_matrix((buf, 9, 3, 5))
    assert (m.M, m.ncol, m.ld, m.row0, m.ptr, m.nbytes) == (9, 3, 5, 0, PTR0, 9 * 5 * 8)
    assert m.owner is buf and m.ctx is buf.ctx
    assert V.matrix_shape((buf, 9, 3, 5)) == (9, 3) and V.matrix_shape(m) == (9, 3)
    assert V.as_matrix(m) is m
    for bad in ((Buf(9 * 5 * 8 - 8), 9, 3, 5),   # eight bytes short
                (buf, 9, 6, 5),                  # ld < ncol
                (buf, 0, 3, 5), (buf, -1, 3, 5),  # M < 1
                (buf, 9, 0, 5)):
        for fn in (V.as_matrix, V.matrix_shape):
            with pytest.raises(ValueError, match="does not fit its buffer"):
                fn(bad)


def test_chain_tuple_parsing(no_device):
    buf = Buf(7 * 24 * 8)
    assert V.chain_dims((buf, 7, 8, 3)) == (7, 8, 3)
    c = V.as_chain((buf, 7, 8, 3))
    assert c.shape == (7, 8, 3) and c.ptr == PTR0 and c.owner is buf and c.logp is None
    for bad in ((Buf(7 * 24 * 8 - 8), 7, 8, 3), (buf, 7, 0, 3), (buf, 7, -8, -3), (buf, 7, 8, 0),
                (buf, -1, 8, 3)):
        for fn in (V.chain_dims, V.as_chain):
            with pytest.raises(ValueError, match="does not fit its buffer"):
                fn(bad)
    for bad in ((buf, 7, 8), (np.zeros(3), 7, 8, 3)):
        with pytest.raises(ValueError, match="a device chain is"):
            V.chain_dims(bad)
    with pytest.raises(ValueError, match="needed at least"):
        V.chain_dims((buf, 7, 8, 3), 6, 2)
    with pytest.raises(ValueError, match="behind discard"):
        V.as_chain((buf, 7, 8, 3), 7)
    with pytest.raises(ValueError, match="negative"):
        V.chain_dims((buf, 7, 8, 3), -1)


def test_host_shapes_are_checked_without_a_device(no_device):
    assert V.matrix_shape(np.zeros(6)) == (6, 1) and V.matrix_shape(np.zeros((6, 2))) == (6, 2)
    assert V.matrix_shape(np.zeros((6, 2)), pointwise=True) == (6, 2)
    with pytest.raises(ValueError, match="a pointwise matrix must be 2-D"):
        V.matrix_shape(np.zeros(6), pointwise=True)
    with pytest.raises(ValueError, match=r"samples must be \(M,\) or \(M, ncol\)"):
        V.matrix_shape(np.zeros((2, 3, 4)))
    for x in (np.zeros((0, 3)), np.zeros((3, 0))):
        for pw in (False, True):
            with pytest.raises(ValueError, match="no samples"):
                V.matrix_shape(x, pw)
    assert V.chain_dims(np.zeros((7, 8, 3)), 2, 5) == (7, 8, 3)
    with pytest.raises(ValueError, match=r"a chain must be \(rows, nwalkers, ndim\)"):
        V.chain_dims(np.zeros((7, 8)))
    with pytest.raises(ValueError, match="no walkers or no parameters"):
        V.chain_dims(np.zeros((7, 0, 3)))
    with pytest.raises(ValueError, match="needed at least"):
        V.chain_dims(np.zeros((7, 8, 3)), 2, 6)
    # a host array is uploaded by as_matrix / as_chain, after the checks
    for fn, x in ((V.as_matrix, np.zeros((6, 2))), (V.as_chain, np.zeros((7, 8, 3)))):
        with pytest.raises(AssertionError, match="device work"):
            fn(x)


def test_chain_view_arithmetic(no_device):
    c = chain_783()
    b = c.behind(2)
    assert b.nrows == 5 and b.shape == (5, 8, 3) and b.S == 40
    assert b.pooled() == (PTR0, 2, 5, 24, 3, 8, 3)
    f = b.flat()
    assert (f.M, f.ncol, f.ld, f.ptr) == (40, 3, 3, PTR0 + 8 * 2 * 24)
    assert f.pooled() == (PTR0, 16, 40, 3, 0, 1, 3)
    a, want = c.rows(2, 5).rows(1, 3), c.rows(3, 5)
    assert a.pooled() == want.pooled() == (PTR0, 3, 2, 24, 3, 8, 3)
    assert a.ptr == want.ptr == PTR0 + 8 * 3 * 24 and a.shape == want.shape == (2, 8, 3)
    assert V.as_chain(c, 2).pooled() == b.pooled()
    assert V.as_chain(b, 1).pooled() == c.behind(3).pooled()
    assert V.chain_dims(b) == (5, 8, 3)


def test_logp_follows_the_chain(no_device):
    c = chain_783(logp=True)
    lp0 = c.logp.ptr
    assert (c.logp.M, c.logp.ncol, c.logp.ld) == (7, 8, 8)
    for view, row0, n in ((c.behind(2), 2, 5), (c.rows(2, 5).rows(1, 3), 3, 2),
                          (V.as_chain(c, 4), 4, 3)):
        assert view.m.row0 == row0 and view.nrows == n
        assert (view.logp.row0, view.logp.M, view.logp.ld) == (row0, n, 8)
        assert view.logp.ptr == lp0 + 8 * row0 * 8
    with pytest.raises(ValueError, match=r"log-probabilities are not \(7, 8\)"):
        V.as_chain(chain_783(), logp=V.matrix_on(Buf(6 * 8 * 8), 6, 8))
    with pytest.raises(ValueError, match="does not fit its buffer"):
        V.matrix_on(Buf(7 * 8 * 8 - 8), 7, 8)


def test_bounds(no_device):
    c = chain_783(logp=True)
    for a, b in ((-1, 2), (3, 2), (0, 8)):
        with pytest.raises(ValueError):
            c.rows(a, b)
        with pytest.raises(ValueError):
            c.m.rows(a, b)
        with pytest.raises(ValueError):
            c.flat().rows(a * 8, b * 8)
    with pytest.raises(ValueError):
        c.behind(8)
    with pytest.raises(ValueError):
        c.behind(2).rows(0, 6)  # (inside the buffer, outside the view)
    m = V.as_matrix((Buf(9 * 5 * 8), 9, 3, 5))
    assert m.pooled() == (PTR0, 0, 9, 5, 0, 1, 3)
    assert m.rows(2, 9).pooled() == (PTR0, 2, 7, 5, 0, 1, 3) and m.rows(2, 9).ptr == PTR0 + 8 * 10
    # a view that claims more than its buffer holds is refused where it is made
    with pytest.raises(ValueError, match="does not fit its buffer"):
        V.DeviceMatrix(m.ctx, PTR0, 9, 3, 5, m.owner, 1, m.nbytes)


def test_get_reads_nothing_behind_the_last_value(monkeypatch):
    """``rows(2, 9)`` of a (9, 3) matrix stored with ld 5 in a buffer that ends with the last
    row's third value: the download starts at row 2 and stops there"""
    from naima_amd import _lib
    buf = Buf((8 * 5 + 3) * 8)
    buf.ctx = type("Ctx", (), {"h": 1})()
    m = V.DeviceMatrix(buf.ctx, buf.ptr, 9, 3, 5, buf)   # (size unknown to the view: no check)
    reads = []

    class Lib:
        @staticmethod
        def nh_download(h, dst, src, nbytes):
            reads.append((src, nbytes))
            return 0
    monkeypatch.setattr(_lib, "_lib", Lib)
    monkeypatch.setattr(_lib, "_chk", lambda rc: None)
    out = m.rows(2, 9).get()
    assert out.shape == (7, 3)
    (src, nbytes), = reads
    assert src == PTR0 + 8 * 2 * 5 and src + nbytes == buf.ptr + buf.nbytes


def test_typed_views_are_never_reinterpreted(no_device):
    """each reaches the branch of its own type, told by the argument error that branch raises"""
    from naima_amd import posterior as P
    m = V.as_matrix((Buf(24 * 4 * 8), 24, 4, 4))       # as a chain tuple this would be (24, 4, 4)
    c = V.as_chain((Buf(24 * 4 * 8), 6, 4, 4))         # as a matrix tuple this would be 6 x 4, ld 4
    with pytest.raises(ValueError, match="no samples behind discard = 24"):
        P.rank_normalize(m, ensembles=2, discard=24)
    with pytest.raises(ValueError, match="no samples behind discard = 24"):
        P.covariance(m, discard=24)
    with pytest.raises(ValueError, match="0 rows behind discard = 6: 1 needed at least"):
        P.rank_columns(c, discard=6)
    with pytest.raises(ValueError, match="do not split"):
        P.rank_normalize(c, ensembles=3)
    # and a matrix does not ask whether its columns split into ensembles
    with pytest.raises(ValueError, match="no samples behind discard = 30"):
        P.rank_normalize(m, ensembles=3, discard=30)
    # the legacy tuple keeps its two readings
    t = (Buf(24 * 4 * 8), 6, 4, 4)
    with pytest.raises(ValueError, match="no samples behind discard = 6"):
        P.rank_columns(t, discard=6)
    with pytest.raises(ValueError, match="0 rows behind discard = 6: 1 needed at least"):
        P.rank_normalize(t, discard=6)
    with pytest.raises(ValueError, match=r"samples must be \(M,\) or \(M, ncol\)"):
        P.histogram(c, range=(0, 1))
