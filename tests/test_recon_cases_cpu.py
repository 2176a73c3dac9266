"""CPU: the numpy statement of reconstruction and mesh readout (tests/recon_numpy.py) and the host model of the random positions
(fastbox_amd.rng.recon_uniforms) held to what is known without them -- closed-form plane waves, the defining equation checked
spectrally, the windows' partition of unity and the adjointness of readout and paint, a chi^2 of the uniforms -- and the
physical check: reconstruction raises the correlation with the linear field in every |k| bin.  tests/test_recon_gpu.py then
holds the device to the statement."""
import functools

import numpy as np
import pytest

from fastbox_amd import rng as fb_rng
from tests import halos_numpy as hn
from tests import recon_cases as rc
from tests import recon_numpy as rn

GEOMS = rc.geometries()
GEOM_IDS = ["N%d-%s" % (N, "x".join("%g" % a for a in L)) for N, L in GEOMS]


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("wave", sorted(rc.WAVES))
@pytest.mark.parametrize("beta", (0., rc.PARAMS["beta"]))
def test_plane_wave_displacement_is_the_closed_form(N, L, wave, beta):
    """Psi of A cos(k0.x) is -A k0 sin(k0.x) exp(-k0^2 R^2 / 2) / (b (k0^2 + beta k0z^2)) to rounding (the sign: recon_cases
    plane_wave_psi), along x, along z -- where beta matters -- and oblique, in cubic and cuboid boxes."""
    R, b = rc.PARAMS["R"], rc.PARAMS["b"]
    delta, k0 = rc.plane_wave(N, L, rc.WAVES[wave])
    got = rn.displacement(delta, L, R, b, beta)
    want = rc.plane_wave_psi(N, L, rc.WAVES[wave], R, b, beta)
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    if wave == "along z":                                   # beta changes the answer there, and only there
        other = rn.displacement(delta, L, R, b, 0. if beta else 0.4)
        assert np.max(np.abs(other - got)) > 1e-2 * np.max(np.abs(got))
    if wave == "along x":
        np.testing.assert_allclose(rn.displacement(delta, L, R, b, 0.7), got, rtol=0, atol=1e-15)


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_displacement_solves_the_defining_equation(N, L):
    """div Psi + beta d_z Psi_z = -delta_smoothed / b, spectrally, on every mode off the Nyquist planes (where the first
    derivative is dropped by convention) and k = 0."""
    R, b, beta = rc.PARAMS["R"], rc.PARAMS["b"], rc.PARAMS["beta"]
    delta = rc.random_field(N)
    psi = rn.displacement(delta, L, R, b, beta)
    m, k = rn.kvec(N, L)
    K = [k[0].reshape(N, 1, 1), k[1].reshape(1, N, 1), k[2].reshape(1, 1, N)]
    M = [m.reshape(N, 1, 1), m.reshape(1, N, 1), m.reshape(1, 1, N)]
    pk = [np.fft.fftn(p) for p in psi]
    lhs = 1j * (K[0] * pk[0] + K[1] * pk[1] + K[2] * pk[2]) + beta * 1j * K[2] * pk[2]
    kk = K[0] ** 2 + K[1] ** 2 + K[2] ** 2
    rhs = -np.fft.fftn(delta) * np.exp(-0.5 * kk * R * R) / b
    inner = (M[0] != -(N // 2)) & (M[1] != -(N // 2)) & (M[2] != -(N // 2)) & (kk > 0.)
    assert np.max(np.abs((lhs - rhs)[inner])) <= 1e-12 * np.max(np.abs(rhs))
    for a in range(3):                                      # component a vanishes on its own Nyquist plane, and all at k = 0
        assert np.max(np.abs(pk[a][tuple(slice(None) if c != a else N // 2 for c in range(3))])) <= 1e-12 * np.max(np.abs(pk[a]))
        assert abs(pk[a][0, 0, 0]) <= 1e-12 * np.max(np.abs(pk[a]))
    curl_z = K[0] * pk[1] - K[1] * pk[0]                    # irrotational
    assert np.max(np.abs(curl_z[inner])) <= 1e-12 * np.max(np.abs(K[0] * pk[1]))


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_single_nyquist_mode_moves_nothing_along_its_axis(axis):
    N, L = GEOMS[1]
    spec, _ = rc.nyquist_mode_spectrum(N, axis)
    psi = rn.displacement_k(spec, L, 3., 1., 0.3)
    assert np.all(psi[axis] == 0.)
    assert all(np.max(np.abs(psi[c])) > 0. for c in range(3) if c != axis)


@pytest.mark.parametrize("N,L", GEOMS[:2], ids=GEOM_IDS[:2])
@pytest.mark.parametrize("window", rc.WINDOWS)
def test_windows(N, L, window):
    """Readout on nodes returns the node values exactly (NGP and CIC; TSC reads its (1/8, 3/4, 1/8) stencil, exact for dyadic
    fields); a constant reads as the constant; the readout is the adjoint of the paint."""
    F = rc.readout_fields(N)
    pos, idx = rc.node_positions(N, L)
    got = rn.readout(F, pos, L, window)
    for c in range(3):
        want = F[c][idx[:, 0], idx[:, 1], idx[:, 2]] if window != "tsc" else rc.tsc_node_stencil(F[c], idx)
        np.testing.assert_array_equal(got[:, c], want)
    cloud = rc.readout_positions(N, L)["wave tail"] + 0.123
    const = np.full((1, N, N, N), 2.75)
    assert np.max(np.abs(rn.readout(const, cloud, L, window) - 2.75)) <= 8 * 2. ** -53 * 2.75
    w = np.random.RandomState(2).normal(size=cloud.shape[0])
    lhs = np.sum(w * rn.readout(F[:1], cloud, L, window)[:, 0])
    rhs = np.sum(F[0] * hn.paint(cloud, N, L, window, weights=w))
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(w)) * np.max(np.abs(F[0]))


@pytest.mark.parametrize("N,L", GEOMS[:2], ids=GEOM_IDS[:2])
def test_shift_wraps_and_moves_along_z_twice(N, L):
    """Psi = 0 returns the wrapped positions bit for bit; a constant Psi moves every particle by scale Psi, and by
    (scale + scale_z) Psi_z along z."""
    pos = rc.readout_positions(N, L)["seam"]
    got = rn.shift(np.zeros((3, N, N, N)), pos, L, "cic", 1., 0.5)
    np.testing.assert_array_equal(got, rn.wrap(pos, L))
    assert np.all((got >= 0.) & (got < np.asarray(L)))
    cell = np.asarray(L) / N
    psi = np.ones((3, N, N, N)) * (0.25 * cell).reshape(3, 1, 1, 1)
    got = rn.shift(psi, pos, L, "tsc", 2., 1.)
    np.testing.assert_array_equal(got, rn.wrap(pos - 0.25 * cell * np.array([2., 2., 3.]), L))


def test_recon_uniforms_model():
    """In [0, L), reproducible, independent of how the points are split into calls, and uniform: chi^2 of the occupancy of
    8^3 cells within 5 sigma; the three coordinates come from different words."""
    L = (32., 48., 80.)
    n = 1 << 16
    u = fb_rng.recon_uniforms(n, L, 9, 2)
    assert u.shape == (n, 3) and u.dtype == np.float64
    assert np.all(u >= 0.) and np.all(u < np.asarray(L))
    np.testing.assert_array_equal(fb_rng.recon_uniforms(n, L, 9, 2), u)
    np.testing.assert_array_equal(fb_rng.recon_uniforms(100, L, 9, 2, first=1000), u[1000:1100])
    assert not np.array_equal(fb_rng.recon_uniforms(16, L, 9, 3), u[:16])
    assert not np.array_equal(fb_rng.recon_uniforms(16, L, 10, 2), u[:16])
    cells = np.floor(u / np.asarray(L) * 8).astype(np.int64)
    occ = np.bincount((cells[:, 0] * 8 + cells[:, 1]) * 8 + cells[:, 2], minlength=512)
    chi2 = np.sum((occ - n / 512.) ** 2 / (n / 512.))
    assert abs(chi2 - 511.) < 5. * np.sqrt(2. * 511.)
    f = u / np.asarray(L)
    assert np.max(np.abs(np.corrcoef(f.T) - np.eye(3))) < 5. / np.sqrt(n)


@functools.lru_cache(maxsize=None)
def _physical(f, randoms):
    c = rc.physical_case(f)
    N, L = c["N"], c["L"]
    R = rn.grid_positions(N, L) if randoms == "grid" else rn.uniform_positions(4 * N ** 3, L, 3)
    out = rn.reconstruct(c["data"], R, N, L, c["R"], 1., f)
    before = rn.cross_correlation(rn.density_contrast(c["data"], N, L), c["delta_lin"], L)
    after = rn.cross_correlation(out["delta_rec"], c["delta_lin"], L)
    return c, out, before, after


@pytest.mark.parametrize("f", (0., 0.5))
@pytest.mark.parametrize("randoms", ("grid", "drawn"))
def test_reconstruction_raises_the_correlation_with_the_linear_field(f, randoms):
    """32^3 lattice, Zel'dovich rms of one cell per axis, R = 1.5 cells, b = 1: r(k) with the linear field is higher after
    reconstruction in every one of the 8 bins up to the Nyquist frequency, in real space and, with f = 0.5 and the matching
    displacement, in redshift space; the data end up nearer their lattice sites."""
    c, out, before, after = _physical(f, randoms)
    print("f = %g, %s randoms: r(k) before %s after %s" % (f, randoms, np.round(before, 3), np.round(after, 3)))
    assert np.all(after > before)
    assert before[0] > 0.9 and after[0] > 0.98 and after[3] > before[3] + 0.3
    d0, d1 = rc.lattice_rms(c["data"], c["lattice"], c["L"]), rc.lattice_rms(out["data"], c["lattice"], c["L"])
    print("rms distance from the lattice sites: %.3f -> %.3f cells" % (d0 / 2., d1 / 2.))
    assert d1 < 0.5 * d0


def test_iso_differs_from_sym_in_the_randoms_only():
    c = rc.physical_case(0.5)
    N, L = c["N"], c["L"]
    R = rn.grid_positions(N, L)
    sym = rn.reconstruct(c["data"], R, N, L, c["R"], 1., 0.5, "sym")
    iso = rn.reconstruct(c["data"], R, N, L, c["R"], 1., 0.5, "iso")
    np.testing.assert_array_equal(sym["data"], iso["data"])
    assert not np.array_equal(sym["randoms"], iso["randoms"])
    np.testing.assert_array_equal(sym["randoms"][:, :2], iso["randoms"][:, :2])
