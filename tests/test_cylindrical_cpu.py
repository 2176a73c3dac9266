"""CPU: the numpy statement of the cylindrical power spectrum and the multi-frequency angular power spectrum
(tests/cyl_numpy.py) against sum rules, plane waves and the identity that ties the two estimators together; and the host
helpers of fastbox_amd.hostgeom (edges, finishing, collapse) that CosmoBox.cylindrical_power_spectrum and
.angular_power_spectrum use."""
import numpy as np
import pytest

from fastbox_amd import hostgeom
from tests import cyl_numpy as cn


def _field(N, seed=0):
    return np.random.RandomState(seed).normal(size=(N, N, N)) + 0.3


ALL_PERP = np.array([0., np.inf])
ALL_PAR = np.array([-1., np.inf])


@pytest.mark.parametrize("N,L", [(8, (10., 10., 10.)), (12, (10., 20., 35.))])
def test_half_spectrum_form_equals_full_grid_form(N, L):
    d1, d2 = _field(N, 1), _field(N, 2)
    pe = np.array([0., 0.7, 1.5, 2.9, np.inf])
    qe = np.array([-0.1, 0.3, 0.9, 2.0])
    a, b = cn.cyl_sums(d1, d2, L, pe, qe), cn.cyl_sums_brute(d1, d2, L, pe, qe)
    assert np.array_equal(a["modes"], b["modes"])
    for key in ("sum_kperp", "sum_kpar", "sum_p"):
        assert np.allclose(a[key], b[key], rtol=1e-12, atol=1e-12 * np.max(np.abs(b[key])))


@pytest.mark.parametrize("N,L", [(8, (10., 10., 10.)), (12, (10., 20., 35.))])
def test_parseval_cylindrical(N, L):
    d = _field(N, 3)
    s = cn.cyl_sums(d, None, L, np.linspace(0., 40., 9), np.linspace(-1., 40., 7))
    assert s["modes"].sum() == N ** 3 - 1
    V = L[0] * L[1] * L[2]
    want = (V / float(N) ** 6) * (N ** 3 * np.sum(d * d) - np.sum(d) ** 2)
    assert abs(s["sum_p"].sum() - want) <= 1e-12 * abs(want)
    one = cn.cyl_sums(d, None, L, ALL_PERP, ALL_PAR)
    assert one["modes"][0, 0] == N ** 3 - 1 and abs(one["sum_p"][0, 0] - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("N,L", [(8, (10., 10., 10.)), (12, (10., 20., 35.))])
def test_parseval_angular(N, L):
    d = _field(N, 4)
    k, cl, modes = cn.angular_power_spectrum(d, None, L, np.linspace(0., 40., 9))
    assert modes.sum() == N * N - 1
    got = np.nansum(modes[:, None] * np.einsum("bii->bi", cl), axis=0)
    want = (L[0] * L[1] / float(N) ** 4) * (N * N * np.sum(d * d, axis=(0, 1)) - np.sum(d, axis=(0, 1)) ** 2)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(cl[modes > 0], np.transpose(cl[modes > 0], (0, 2, 1)))


def test_plane_wave_lands_in_its_cell_and_bin():
    N, L = 16, (100., 100., 100.)
    kf = 2. * np.pi / 100.
    x = np.arange(N)
    mx, my, mz = 3, -2, 5
    d = np.cos(2. * np.pi * (mx * x[:, None, None] + my * x[None, :, None] + mz * x[None, None, :]) / N)
    pe = np.arange(0., 9.) * kf                       # sqrt(13) = 3.6: k_perp bin 3
    qe = (np.arange(N // 2 + 2) - 0.5) * kf
    s = cn.cyl_sums(d, None, L, pe, qe)
    p = s["sum_p"]
    assert p[3, 5] > 0 and np.all(np.abs(np.delete(p.ravel(), 3 * (N // 2 + 1) + 5)) <= 1e-20 * p[3, 5])
    # the two modes +-m hold all of sum d^2: (V / N^6) N^3 sum d^2
    assert abs(p[3, 5] - (1e6 / float(N) ** 6) * N ** 3 * np.sum(d * d)) <= 1e-12 * p[3, 5]
    k, cl, modes = cn.angular_power_spectrum(d, None, L, pe)
    assert modes[0] == 0 and np.all(np.isnan(cl[0]))                  # [0, kf) holds m_perp = 0 alone, which is excluded
    power = np.array([np.max(np.abs(c)) for c in cl[1:]])
    assert power[2] > 0 and np.all(np.delete(power, 2) <= 1e-20 * power[2])
    # a plane wave along z alone has m_perp = 0: it is in no bin
    dz = np.cos(2. * np.pi * mz * x[None, None, :] / N) * np.ones((N, N, 1))
    assert np.nanmax(np.abs(cn.angular_power_spectrum(dz, None, L, pe)[1])) <= 1e-20


@pytest.mark.parametrize("N,L", [(8, (10., 10., 10.)), (12, (10., 20., 35.))])
def test_identity_between_the_two_estimators(N, L):
    """P(b, m) = (Lz / N^2) sum C_b(nu, nu') cos(2 pi m (nu - nu') / N) for the same k_perp edges with edges[0] > 0 and one
    k_par bin per |m_z|; modes(b, m) = modes_b (1 if m in {0, N/2} else 2)."""
    d = _field(N, 5)
    pe = np.array([0.2, 0.9, 1.7, 2.6, 4.0])
    qe = (np.arange(N // 2 + 2) - 0.5) * (2. * np.pi / L[2])
    kperp, kpar, power, modes = cn.cylindrical_power_spectrum(d, None, L, pe, qe)
    k, cl, mb = cn.angular_power_spectrum(d, None, L, pe)
    mult = np.where((np.arange(N // 2 + 1) == 0) | (np.arange(N // 2 + 1) == N // 2), 1, 2)
    assert np.array_equal(modes, mb[:, None] * mult[None, :])
    m = mb > 0
    rhs = cn.power_from_maps(cl[m], L[2])
    assert np.max(np.abs(rhs - power[m])) <= 1e-12 * np.max(np.abs(power[m]))
    assert np.allclose(kperp[m], np.repeat(k[m][:, None], N // 2 + 1, axis=1), rtol=1e-14, atol=0)


def test_white_noise_channel_correlation_bound():
    """Independent channels: the off-diagonal correlation coefficients of C_b scatter with 1 / sqrt(modes_b); the bound
    5 / sqrt(modes_b) the GPU test puts on NoiseModel cubes holds for numpy white noise of the same shape."""
    N, L = 64, (1e3, 1e3, 1e3)
    d = np.random.RandomState(11).normal(size=(N, N, N))
    pe = hostgeom.maps_edges(L, N)
    k, cl, modes = cn.angular_power_spectrum(d, None, L, pe)
    sel = modes >= 100
    assert sel.sum() >= 10
    off = ~np.eye(N, dtype=bool)
    for b in np.nonzero(sel)[0]:
        dg = np.sqrt(np.diag(cl[b]))
        r = cl[b] / (dg[:, None] * dg[None, :])
        assert np.max(np.abs(r[off])) <= 5. / np.sqrt(modes[b])
        assert abs(np.mean(r[off])) <= 5. / np.sqrt(modes[b]) / np.sqrt(N)


# ---- hostgeom ---------------------------------------------------------------------------------------------------------------
def test_default_edges():
    L, N = (100., 200., 400.), 16
    pe, qe = hostgeom.cyl_edges(L, N)
    dk = 2. * np.pi / 100.
    assert np.array_equal(pe, np.arange(0., np.pi * N / 200. + 0.5 * dk, dk))
    assert np.array_equal(qe, (np.arange(N // 2 + 2) - 0.5) * (2. * np.pi / 400.)) and qe.size == N // 2 + 2
    me = hostgeom.maps_edges(L, N)
    assert np.array_equal(me, np.arange(0.5 * dk, np.pi * N / 200. + 0.5 * dk, dk))
    pe2, _ = hostgeom.cyl_edges(L, N, dk_perp=0.05, kperp_min=0.01, kperp_max=0.3)
    assert np.array_equal(pe2, np.arange(0.01, 0.3 + 0.025, 0.05))
    given = hostgeom.cyl_edges(L, N, kperp_bins=[0., 1., np.inf], kpar_bins=[0., 2., np.inf])
    assert np.array_equal(given[0], [0., 1., np.inf]) and np.array_equal(given[1], [0., 2., np.inf])
    # the defaults of a 2048^3 cube fit the limits: 1024 and 1025 bins
    pe3, qe3 = hostgeom.cyl_edges((1e3, 1e3, 1e3), 2048)
    assert pe3.size - 1 <= hostgeom.CYL_MAX_PERP and qe3.size - 1 == hostgeom.CYL_MAX_PAR


def test_edge_validation_errors():
    L, N = (100., 100., 100.), 16
    bad = [dict(kperp_bins=[0., 0.5, 0.3]), dict(kperp_bins=[-0.1, 0.5]), dict(kperp_bins=[0.1]),
           dict(kperp_bins=[0., np.inf, np.inf]), dict(kperp_bins=[0., np.nan, 1.]), dict(dk_perp=0.), dict(dk_perp=-1.),
           dict(kperp_bins=np.linspace(0., 1., 1026)), dict(kpar_bins=[0., 0.5, 0.5]), dict(kpar_bins=[0.]),
           dict(kpar_bins=[0., np.nan]), dict(kpar_bins=np.linspace(0., 1., 1027)), dict(kperp_bins=np.zeros((2, 2)))]
    for kw in bad:
        with pytest.raises(ValueError):
            hostgeom.cyl_edges(L, N, **kw)
    for kw in bad[:7] + [dict(kperp_bins=np.linspace(0., 1., 258))]:
        with pytest.raises(ValueError):
            hostgeom.maps_edges(L, N, **kw)
    with pytest.raises(ValueError):
        hostgeom.maps_edges(L, 2048)
    assert hostgeom.cyl_edges(L, N, kperp_bins=np.linspace(0., 1., 1025))[0].size == 1025
    assert hostgeom.cyl_edges(L, N, kpar_bins=np.linspace(-1., 1., 1026))[1].size == 1026
    assert hostgeom.maps_edges(L, N, kperp_bins=np.linspace(0., 1., 257)).size == 257
    with pytest.raises(ValueError) as e1:
        hostgeom.cyl_edges(L, N, kperp_bins=[0.5, 0.3])
    with pytest.raises(ValueError) as e2:
        hostgeom.power_edges(L, N, kbins=[0.5, 0.3])
    assert str(e1.value) == str(e2.value)


def test_finish_cyl_and_finish_maps():
    nperp, npar = 2, 3
    modes = np.array([4., 0., 2., 1., 8., 0.])
    raw = np.concatenate([modes, modes * 0.5, modes * 0.25, modes * 3.])
    kperp, kpar, power, m = hostgeom.finish_cyl(raw, nperp, npar)
    assert m.shape == (2, 3) and np.array_equal(m.ravel(), modes)
    e = modes.reshape(2, 3) == 0
    for a, v in ((kperp, 0.5), (kpar, 0.25), (power, 3.)):
        assert a.dtype == np.float64 and a.flags.writeable and np.array_equal(np.isnan(a), e) and np.all(a[~e] == v)
    k, mm = hostgeom.finish_maps(np.array([3., 0., 5., 1.5, 0., 10.]), 3)
    assert mm.dtype == np.int64 and np.array_equal(mm, [3, 0, 5])
    assert k[0] == 0.5 and np.isnan(k[1]) and k[2] == 2.


def test_collapse_maps_on_a_toeplitz_matrix():
    N = 7
    f = np.array([5., 3., 2., 1., 0.5, 0.25, 0.125])
    i = np.arange(N)
    toe = f[np.abs(i[:, None] - i[None, :])]
    cl = np.stack([toe, 2. * toe])
    out = hostgeom.collapse_maps(cl)
    assert out.shape == (2, N) and np.allclose(out[0], f, rtol=1e-15) and np.allclose(out[1], 2. * f, rtol=1e-15)
    rs = np.random.RandomState(0).normal(size=(3, N, N))
    assert np.allclose(hostgeom.collapse_maps(rs), cn.collapse(rs), rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        hostgeom.collapse_maps(np.zeros((3, 4)))


def test_library_declares_the_entries():
    from fastbox_amd import _lib
    for name in ("fb_bin_power_cyl", "fb_power_spectrum_cyl", "fb_transverse_gram", "fb_transverse_gram_work_bytes",
                 "fb_angular_power"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.fb_version() >= 102
    assert lib.fb_transverse_gram_work_bytes(None, 4, 0) == 0
