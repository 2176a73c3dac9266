"""CPU: the numpy statement of the correlation function (tests/corrfn_numpy.py) -- its FFT form against a brute-force sum
over all cell pairs, the line of sight pinned by plane waves -- and the argument handling of
CosmoBox.correlation_function that needs no GPU."""
import ctypes

import numpy as np
import pytest

from tests import corrfn_numpy as cf
from fastbox_amd import hostgeom

BOXES = [(100., 100., 100.), (1e2, 2e2, 1e3)]


def _fields(N, seed):
    rng = np.random.RandomState(seed)
    d1 = rng.standard_normal((N, N, N)) + 0.3
    d2 = 0.5 * d1 + rng.standard_normal((N, N, N)) - 1.
    return d1, d2


@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("L", BOXES)
@pytest.mark.parametrize("cross", [False, True])
def test_fft_form_equals_brute_force(N, L, cross):
    d1, d2 = _fields(N, 3 + N)
    d2 = d2 if cross else None
    xa, xb = cf.xi_fft(d1, d2), cf.xi_brute(d1, d2)
    scale = abs(xb[0, 0, 0])
    assert np.max(np.abs(xa - xb)) <= 1e-13 * scale
    h = min(L) / N
    # edges on separations (dr = the cell size) and a ragged set
    for edges in (np.arange(0., 0.5 * min(L) + 0.5 * h, h), np.array([0., 0.7 * h, 2.5 * h, 3 * h, 0.5 * max(L)])):
        ra, xia, na = cf.bin_xi(xa, L, edges, poles=(0, 2, 4))
        rb, xib, nb = cf.bin_xi(xb, L, edges, poles=(0, 2, 4))
        assert np.array_equal(na, nb) and np.array_equal(ra, rb, equal_nan=True)
        m = na > 0
        assert np.max(np.abs(xia[:, m] - xib[:, m])) <= 1e-12 * scale
        assert np.all(np.isnan(xia[:, ~m])) and np.all(np.isnan(ra[~m]))


def test_edges_on_separations_fall_in_the_upper_bin():
    # L = 1000, N = 500, dr = 2: (2, 0, 0) has |s| = 2.0 exactly and belongs to [2, 4)
    (ix, sx), _, _ = cf.separation_axes(500, (1e3,) * 3)
    assert sx[1] == 2.0
    edges = np.arange(0., 10.5, 2.)
    assert np.digitize([np.sqrt((sx[1] * sx[1] + 0.) + 0.)], edges)[0] - 1 == 1


@pytest.mark.parametrize("L", BOXES)
def test_npairs_cover_the_grid(L):
    N = 16
    d = _fields(N, 5)[0]
    r, x, n = cf.bin_xi(cf.xi_fft(d), L, np.array([0., 1e-9, 0.1 * min(L), 1e9]), poles=(0,))
    assert n.sum() == N ** 3 and n[0] == 1
    # zero lag = the variance; the sum over every separation vanishes (the k = 0 mode is removed)
    assert abs(x[0, 0] - np.var(d)) <= 1e-13 * np.var(d)
    total = np.sum(x[0] * n)
    assert abs(total) <= 1e-12 * np.var(d) * N ** 3


def test_plane_wave_pins_the_line_of_sight():
    N, L = 32, 100.
    q = np.arange(N)
    wave = np.cos(2 * np.pi * 3 * q * (L / N) / L)
    dz = np.broadcast_to(wave[None, None, :], (N, N, N)).copy()
    dx = np.broadcast_to(wave[:, None, None], (N, N, N)).copy()
    xz = cf.xi_fft(dz)
    m = cf.signed_index(N)
    expect = 0.5 * np.cos(2 * np.pi * 3 * m / N)
    assert np.max(np.abs(xz - expect[None, None, :])) < 1e-14
    edges = np.arange(0., 0.5 * L + 1e-9, L / N)
    rz, pz, nz = cf.bin_xi(xz, (L,) * 3, edges, poles=(0, 2))
    rx, px, nx = cf.bin_xi(cf.xi_fft(dx), (L,) * 3, edges, poles=(0, 2))
    assert np.max(np.abs(pz[1, 1:])) > 0.05                     # a wave along z has a quadrupole
    # bins without s = 0: L2(mu_x) + L2(mu_y) + L2(mu_z) = 0 and the y <-> z symmetry give -1/2 of it along x
    assert np.allclose(px[1, 1:], -0.5 * pz[1, 1:], rtol=0, atol=1e-13)
    assert np.allclose(px[0], pz[0], rtol=0, atol=1e-13)


def test_separation_edges_defaults_and_validation():
    L, N = (1e3, 1e3, 1e3), 500
    e = hostgeom.separation_edges(L, N)
    assert e[0] == 0 and np.isclose(e[1], 2.) and np.isclose(e[-1], 500.) and e.size == 251
    e = hostgeom.separation_edges(L, N, dr=2., rmin=20., rmax=200.)   # the notebooks' bins
    assert e[0] == 20. and e[-1] == 200. and e.size == 91
    e = hostgeom.separation_edges((1e2, 2e2, 1e3), 16)
    assert np.isclose(e[1], 100. / 16) and np.isclose(e[-1], 50.)
    assert hostgeom.separation_edges(L, 1024).size == 513            # the default edges fit up to 2048^3
    assert hostgeom.separation_edges(L, 2048).size == 1025
    for bad in ([0., 2., 2., 4.], [0., 4., 2.], [-1., 2.], [1.], np.zeros((2, 2)), np.arange(1100.)):
        with pytest.raises(ValueError):
            hostgeom.separation_edges(L, N, rbins=bad)
    with pytest.raises(ValueError):
        hostgeom.separation_edges(L, N, dr=0.)
    assert hostgeom.check_poles(None) == (0,) and hostgeom.check_poles([4, 0]) == (4, 0)
    for bad in ([1], [0, 3], [2.5], []):
        with pytest.raises(ValueError):
            hostgeom.check_poles(bad)


def test_finish_correlation_record():
    nb = 3
    raw = np.array([0., 2., 4.,   0., 3., 10.,   0., 1., 2.,   0., 0.5, -1.])
    r, xi, n = hostgeom.finish_correlation(raw, nb, (0, 2))
    assert np.isnan(r[0]) and np.all(np.isnan(xi[:, 0]))
    assert np.allclose(r[1:], [1.5, 2.5]) and np.allclose(xi[0, 1:], [0.5, 0.5]) and np.allclose(xi[1, 1:], [1.25, -1.25])
    assert np.array_equal(n, [0., 2., 4.])


def test_library_exports_the_correlation_entries():
    from fastbox_amd import _lib
    lib = _lib.load()
    assert lib.fb_version() >= 101
    e = (ctypes.c_double * 3)(0., 1., 2.)
    out = (ctypes.c_double * 16)()
    # a NULL plan is refused without touching a device (the checks of edges, nbins and lmax themselves need a plan:
    # tests/test_correlation_gpu.py::test_c_entries_refuse_bad_arguments)
    assert lib.fb_bin_separation(None, None, e, 2, 0, out, None) == -1
    assert lib.fb_correlation_function(None, None, None, None, None, None, e, 2, 0, out, None) == -1
    assert lib.fb_cross_power_half(None, None, None, None, 1.0, None) == -1
