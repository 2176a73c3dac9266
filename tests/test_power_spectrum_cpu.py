"""CPU: the numpy restatement of CosmoBox.power_spectrum (tests/pk_numpy.py) against a brute-force sum over the full FFT grid
and plane-wave known answers, and the host helpers (default edges, mu edges, argument checks, the finishing step)."""
import numpy as np
import pytest

from fastbox_amd import hostgeom
from tests import pk_numpy as pk


def _field(N, seed, cross=False):
    rs = np.random.RandomState(seed)
    d1 = rs.standard_normal((N, N, N))
    return d1, (0.5 * d1 + rs.standard_normal((N, N, N)) if cross else None)


@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("L", [(100., 100., 100.), (100., 200., 50.)])
@pytest.mark.parametrize("cross", [False, True])
def test_restatement_equals_full_grid_brute_force(N, L, cross):
    d1, d2 = _field(N, 3 + N, cross)
    kf = 2. * np.pi / min(L)
    # edges on the lattice (|k| = kf exactly on an edge, axis-aligned modes) and beyond the corner: every mode is binned
    kedges = np.append(np.arange(0., 0.5 * N * 2. * np.pi / min(L) * 1.8, kf), 1e9)
    a = pk.power_sums(d1, d2, L, kedges, Nmu=4, lmax=4)
    b = pk.power_sums_brute(d1, d2, L, kedges, Nmu=4, lmax=4)
    assert np.array_equal(a["modes"], b["modes"])
    assert a["modes"].sum() == N ** 3 - 1                                     # every mode but k = 0
    np.testing.assert_allclose(a["sum_k"], b["sum_k"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(a["sum_mu"], b["sum_mu"], rtol=1e-13, atol=1e-13)
    scale = np.max(np.abs(b["sum_p"]))
    for l in (0, 2, 4):
        assert np.max(np.abs(a["sum_pl"][l] - b["sum_pl"][l])) <= 1e-12 * scale
    # mu = 1 (the k_z axis) lands in the last mu bin: k_x = k_y = 0, m_z = 1 is the first-shell pair on the z axis
    kb = int(np.digitize(2. * np.pi / L[2], kedges) - 1)
    assert b["modes"][kb, -1] >= 2


def test_total_power_is_parseval():
    N, L = 16, (100., 100., 100.)
    d1, _ = _field(N, 5)
    s = pk.power_sums(d1, None, L, [0., 1e9], Nmu=1)
    V = L[0] * L[1] * L[2]
    # sum over all modes but k = 0 of V |D|^2 / N^6 = V (sum d^2 - N^3 mean^2) / N^3
    expect = V * (np.sum(d1 * d1) - N ** 3 * d1.mean() ** 2) / N ** 3
    assert abs(s["sum_p"][0, 0] / expect - 1.) < 1e-12


@pytest.mark.parametrize("axis", [0, 2])
def test_plane_wave_multipoles(axis):
    N, L = 32, 200.
    x = np.arange(N)
    wave = np.cos(2. * np.pi * 3 * x / N)
    shape = [1, 1, 1]
    shape[axis] = N
    d = np.broadcast_to(wave.reshape(shape), (N, N, N)).copy()
    kf = 2. * np.pi / L
    kedges = np.arange(0., 0.5 * N * kf + 0.5 * kf, kf) + 0.5 * kf       # edges between the shells
    kedges = np.concatenate([[0.], kedges])
    k, p, m = pk.power_spectrum(d, None, (L, L, L), kedges, poles=[0, 2, 4])
    b = int(np.digitize(3 * kf, kedges) - 1)
    assert np.nanargmax(np.abs(p[0])) == b
    p0, p2, p4 = p[:, b]
    others = np.delete(p[0], b)
    assert np.nanmax(np.abs(others)) <= 1e-20 * p0                       # all the power is in one mode pair
    if axis == 2:                                                        # along the line of sight: mu = 1
        assert abs(p2 / p0 - 5.) < 1e-12 and abs(p4 / p0 - 9.) < 1e-12
    else:                                                                # across it: mu = 0
        assert abs(p2 / p0 + 2.5) < 1e-12 and abs(p4 / p0 - 27. / 8.) < 1e-12
    # the 2-d form puts it all in one mu bin: the last for mu = 1, the first for mu = 0
    k2, mu2, p2d, m2 = pk.power_spectrum(d, None, (L, L, L), kedges, mode="2d", Nmu=5)
    c = 4 if axis == 2 else 0
    assert p2d[b, c] == pytest.approx(p0 * m[b] / m2[b, c], rel=1e-12)
    assert np.nanmax(np.abs(np.delete(p2d[b], c))) <= 1e-20 * p0


@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 1024, 2048])
def test_default_edges(N):
    L = (1e3, 1e3, 1e3)
    e = hostgeom.power_edges(L, N)
    kf = 2. * np.pi / 1e3
    assert e.size - 1 == N // 2 <= hostgeom.PK_MAX_K
    assert e[0] == 0. and np.allclose(np.diff(e), kf, rtol=1e-12)
    assert abs(e[-1] - np.pi * N / 1e3) < 1e-9 * e[-1]                  # up to Nyquist
    assert np.array_equal(e, np.arange(0., np.pi * N / 1e3 + 0.5 * kf, kf))
    # the 2-d default fits the kernel's LDS rows at every size
    hostgeom.check_power_layout(e.size - 1, 5, 0)
    hostgeom.check_power_layout(e.size - 1, 1, 4)


def test_default_edges_cuboid():
    e = hostgeom.power_edges((100., 200., 400.), 64)
    dk = 2. * np.pi / 100.
    assert e[1] == dk and e[-1] <= np.pi * 64 / 400. + 0.5 * dk
    assert np.array_equal(e, np.arange(0., np.pi * 64 / 400. + 0.5 * dk, dk))


def test_mu_edges_match_the_library_formula():
    """fb_bin_power_kmu builds linspace(0, 1, nmu + 1) as q * (1 / nmu) + 0 with the last edge 1: the same doubles."""
    for nmu in range(1, hostgeom.PK_MAX_MU + 1):
        lib = np.arange(nmu + 1) * (1.0 / nmu) + 0.0
        lib[-1] = 1.0
        assert np.array_equal(hostgeom.mu_edges(nmu), lib), nmu


@pytest.mark.parametrize("kw", [dict(kbins=[0.1, 0.05, 0.2]), dict(kbins=[0., 0.1, 0.1]), dict(kbins=[-0.1, 0.1]),
                                dict(kbins=[0.1]), dict(kbins=np.arange(1026.)), dict(kbins=[0., np.nan, 1.]),
                                dict(dk=0.), dict(dk=-1.), dict(kmin=-1.)])
def test_bad_edges(kw):
    with pytest.raises(ValueError):
        hostgeom.power_edges((1e3, 1e3, 1e3), 64, **kw)


def test_last_edge_may_be_infinite():
    e = hostgeom.power_edges((1e3,) * 3, 64, kbins=[0., 0.1, np.inf])
    assert e.size == 3


@pytest.mark.parametrize("nmu", [0, -1, 129, 2.5, "5", None, True])
def test_bad_nmu(nmu):
    with pytest.raises(ValueError):
        hostgeom.mu_edges(nmu)


@pytest.mark.parametrize("poles", [[1], [0, 3], [6], [], [0.5]])
def test_bad_poles(poles):
    with pytest.raises(ValueError):
        hostgeom.check_poles(poles)


def test_layout_limits():
    hostgeom.check_power_layout(1024, 5, 0)
    hostgeom.check_power_layout(1024, 1, 4)
    hostgeom.check_power_layout(40, 128, 0)
    for nk, nmu, lmax in [(1024, 6, 0), (1024, 5, 2), (41, 128, 0)]:
        with pytest.raises(ValueError):
            hostgeom.check_power_layout(nk, nmu, lmax)


def test_finish_power_record():
    nk, nmu = 3, 2
    nc = nk * nmu
    modes = np.array([2., 0., 4., 6., 8., 10.])
    raw = np.concatenate([modes, 3. * modes, 0.5 * modes, 7. * modes])
    k, mu, p, m = hostgeom.finish_power(raw, nk, nmu)
    assert k.shape == (nk, nmu) and np.isnan(k[0, 1]) and np.isnan(p[0, 1]) and np.isnan(mu[0, 1])
    assert np.all(k[m > 0] == 3.) and np.all(mu[m > 0] == 0.5) and np.all(p[m > 0] == 7.)
    # 1-d with poles: (2l + 1) sum P L_l / modes
    m1 = np.array([2., 0., 4.])
    raw1 = np.concatenate([m1, m1, 0. * m1, 5. * m1, 1. * m1, -1. * m1])
    k, mu, p, m = hostgeom.finish_power(raw1, 3, 1, (0, 2, 4))
    assert p.shape == (3, 3) and np.all(np.isnan(p[:, 1]))
    assert np.allclose(p[:, [0, 2]], [[5., 5.], [5., 5.], [-9., -9.]])
    assert nc == 6
