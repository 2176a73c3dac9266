"""CPU: the numpy statement of CosmoBox.bispectrum (tests/bk_numpy.py) against the explicit sum over mode pairs and against
plane-wave triangles whose bispectrum is known in closed form, and the host helpers of the call (edges, triple order, the
finishing step)."""
import itertools

import numpy as np
import pytest

from fastbox_amd import hostgeom
from tests import bk_numpy as bk


def _plane_waves(N, modes):
    x = np.indices((N, N, N)).astype(np.float64)
    return sum(np.cos(2. * np.pi * (m[0] * x[0] + m[1] * x[1] + m[2] * x[2]) / N) for m in modes)


@pytest.mark.parametrize("N,L", [(8, (100., 100., 100.)), (12, (100., 130., 170.))])
def test_statement_equals_brute_force(N, L):
    """Edges reach past the Nyquist shell of every axis, so triangles that close only modulo N are exercised."""
    d = np.random.RandomState(N).standard_normal((N, N, N))
    edges = np.linspace(0., 1.0001 * np.pi * N / min(L), 5)
    r = bk.bispectrum(d, L, edges)
    sums, cnt = bk.bispectrum_brute(d, L, edges)
    assert np.array_equal(r["ntri"], cnt) and cnt.max() > 0
    aliased = bk.bispectrum(d, L, np.linspace(0., (2. / 3.) * np.pi * N / max(L), 5))["ntri"].sum()
    assert cnt.sum() > aliased                          # (more triangles than the alias-free edges admit)
    dev = np.max(np.abs(r["sums"] - sums)) / np.max(np.abs(sums))
    print("N=%d: max |d sum III| / max |sum III| = %.2e; max |sum UUU / N^3 - ntri| = %.2e"
          % (N, dev, np.max(np.abs(r["usums"] / N ** 3 - cnt))))
    assert dev <= 1e-13


def _triangle(modes, triple):
    N, L = 16, 100.
    kf = 2. * np.pi / L
    edges = (np.arange(9) + 0.5) * kf
    r = bk.bispectrum(_plane_waves(N, modes), L, edges)
    t = int(np.nonzero((r["triples"] == triple).all(axis=1))[0][0])
    return r, t, L ** 3


def test_triangle_in_distinct_shells():
    ms = [(2, 1, 0), (-1, 3, 2), (-1, -4, -2)]
    r, t, V = _triangle(ms, (1, 3, 4))
    assert r["ntri"][t] == 4008
    assert abs(r["B"][t] / (V * V / (4. * 4008.)) - 1.) < 1e-13
    rest = np.delete(r["B"], t)
    assert np.nanmax(np.abs(rest)) < 1e-13 * r["B"][t]


def test_triangle_in_one_shell():
    ms = [(2, 2, 1), (-2, -1, 2), (0, -1, -3)]
    r, t, V = _triangle(ms, (2, 2, 2))
    assert r["ntri"][t] == 1200
    assert abs(r["B"][t] / (1.5 * V * V / 1200.) - 1.) < 1e-13
    rest = np.delete(r["B"], t)
    assert np.nanmax(np.abs(rest)) < 1e-13 * r["B"][t]


def test_triple_order():
    for nb in (1, 2, 5, 32):
        tri = hostgeom.bispectrum_triples(nb)
        assert tri.shape == (nb * (nb + 1) * (nb + 2) // 6, 3)
        assert [tuple(t) for t in tri] == list(itertools.combinations_with_replacement(range(nb), 3))
        assert np.array_equal(tri, bk.triples(nb))
    for bad in (0, 33, 2.5, True):
        with pytest.raises(ValueError):
            hostgeom.bispectrum_triples(bad)


def test_edges():
    L, N = (100., 200., 400.), 32
    e = hostgeom.bispectrum_edges(L, N)
    assert np.array_equal(e, np.linspace(0., (2. / 3.) * np.pi * N / 400., 17))
    assert np.array_equal(hostgeom.bispectrum_edges(L, N, dk=0.05, kmin=0.1, kmax=0.4), np.arange(0.1, 0.425, 0.05))
    assert np.array_equal(hostgeom.bispectrum_edges(L, N, kmin=0.1, kmax=0.4), np.linspace(0.1, 0.4, 17))
    kb = [0.1, 0.2, 0.4, np.inf]
    assert np.array_equal(hostgeom.bispectrum_edges(L, N, kbins=kb), np.array(kb))
    assert hostgeom.bispectrum_edges(L, N, kbins=np.linspace(0., 1., 33)).size == 33


@pytest.mark.parametrize("kw", [
    dict(kbins=[0.1, 0.2], dk=0.1),                    # both
    dict(kbins=[0.2, 0.1]), dict(kbins=[0.1, 0.1, 0.2]),   # not increasing
    dict(kbins=[-0.1, 0.2]), dict(kbins=[0.1, np.nan]), dict(kbins=[0.1, np.inf, np.inf]),
    dict(kbins=[0.1]), dict(kbins=np.linspace(0., 1., 34)), dict(kbins=np.zeros((2, 2))),   # shell count, shape
    dict(dk=0.), dict(dk=-1.), dict(dk=1e-9), dict(dk=0.001, kmax=1.),   # dk: sign, too many shells
    dict(kmin=1., kmax=0.5),
])
def test_edge_errors(kw):
    with pytest.raises(ValueError):
        hostgeom.bispectrum_edges((100., 100., 100.), 32, **kw)


def test_finish():
    """The finishing step on the statement's own raw sums gives the statement's k, B, Q and NaN pattern."""
    N, L = 16, (100., 120., 150.)
    d = np.random.RandomState(3).standard_normal((N, N, N))
    edges = np.array([0., 0.05, 0.3, 0.31, 0.5, 0.9])           # an empty shell (0, 0.05) and a narrow one
    r = bk.bispectrum(d, L, edges)
    nb = edges.size - 1
    D = np.fft.fftn(d)
    b, kk = bk.shell_map(N, L, edges)
    raw = np.concatenate([r["sums"], r["nmodes"], [kk[b == q].sum() for q in range(nb)],
                          [np.sum(np.abs(D[b == q]) ** 2) for q in range(nb)]])
    ntri = hostgeom.bispectrum_ntri(np.concatenate([r["usums"], np.zeros(3 * nb)]), nb, N)
    assert np.array_equal(ntri, r["ntri"])
    k, B, Q, nt = hostgeom.finish_bispectrum(raw, ntri, nb, L, N)
    assert k.shape == (35, 3) and B.shape == Q.shape == nt.shape == (35,)
    for a in (k, B, Q, nt):
        assert a.dtype == np.float64 and a.flags.writeable
    empty = r["ntri"] == 0
    assert empty.any() and not empty.all()
    assert np.array_equal(np.isnan(B), empty) and np.array_equal(np.isnan(Q), empty)
    assert np.array_equal(np.isnan(k), np.isnan(r["k"])) and np.all(np.isnan(k[empty]))
    assert np.allclose(B[~empty], r["B"][~empty], rtol=1e-14, atol=0)
    assert np.allclose(Q[~empty], r["Q"][~empty], rtol=1e-12, atol=0)
    assert np.allclose(k[~empty], r["k"][~empty], rtol=1e-14, atol=0)
