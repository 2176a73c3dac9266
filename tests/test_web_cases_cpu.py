"""CPU: the numpy statement of the cosmic-web classification (tests/web_numpy.py) on the constructed cases of tests/web_cases.py
-- closed-form plane waves, the trace identity, the Nyquist rules, the shear of a linear velocity, matrices with known
eigenvalues -- and the host helpers of fastbox_amd/web.py.  tests/test_web_gpu.py then holds the device to the statement."""
import numpy as np
import pytest

from fastbox_amd import web
from tests import web_cases as wc
from tests import web_numpy as wn

GEOMS = wc.geometries()
GEOM_IDS = ["N%d-%s" % (N, "x".join("%g" % a for a in L)) for N, L in GEOMS]


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_plane_waves_have_the_closed_form(N, L):
    """T_ij = khat_i khat_j exp(-k0^2 R^2 / 2) delta, eigenvalues (s delta, 0, 0) sorted, trace = the smoothed field."""
    for name, mode in sorted(wc.WAVES.items()):
        for R in wc.SMOOTHINGS:
            want, delta, s = wc.plane_wave_tidal(N, L, mode, R)
            got = wn.tidal_tensor(delta, L, R)
            assert np.max(np.abs(got - want)) <= 1e-14, (name, R)
            np.testing.assert_allclose(got[0] + got[1] + got[2], s * delta, rtol=0, atol=1e-14)
            lam = wn.eigenvalues(got)
            sd = s * delta
            exact = np.array([np.maximum(sd, 0.), np.zeros_like(sd), np.minimum(sd, 0.)])
            assert np.max(np.abs(lam - exact)) <= 1e-14
            assert np.all(lam[0] >= lam[1]) and np.all(lam[1] >= lam[2])
            cls = wn.classify(lam, 0.3 * s * wc.AMPLITUDE)
            np.testing.assert_array_equal(cls, (sd > 0.3 * s * wc.AMPLITUDE).astype(np.uint8))


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_trace_is_the_smoothed_field_minus_its_mean_and_the_full_transform_is_real(N, L):
    delta = wc.random_field(N) + 0.7
    for R in wc.SMOOTHINGS:
        T = wn.tidal_tensor(delta, L, R)
        m, k = wn.kvec(N, L)
        k2 = k[0].reshape(N, 1, 1) ** 2 + k[1].reshape(1, N, 1) ** 2 + k[2].reshape(1, 1, N) ** 2
        dk = np.fft.fftn(delta) * np.exp(-0.5 * k2 * R * R)
        dk[0, 0, 0] = 0.
        np.testing.assert_allclose(T[0] + T[1] + T[2], np.fft.ifftn(dk).real, rtol=0, atol=1e-13)
        full = wn.tidal_tensor_full(delta, L, R)
        assert np.max(np.abs(full.imag)) <= 1e-15 * np.max(np.abs(full.real))
        np.testing.assert_allclose(full.real, T, rtol=0, atol=1e-13)


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_nyquist_rules(N, L):
    for axis in range(3):
        spec, _ = wc.nyquist_mode_spectrum(N, axis)
        T = wn.tidal_tensor_k(spec, L, 1.5)
        for q, (i, j) in enumerate(wn.PAIRS):
            if i == j:
                assert np.max(np.abs(T[q])) > 0.
            elif axis in (i, j):
                assert np.all(T[q] == 0.)
    spec = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    spec[0, 0, 0] = 5.
    assert np.all(wn.tidal_tensor_k(spec, L, 0.) == 0.)


@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_shear_of_the_linear_velocity_is_the_tidal_tensor(N, L):
    """Sigma_ij = (f H a / H0) T_ij for v = i fac k delta / k^2 of a field without power on the Nyquist planes."""
    dk = wn.rfftn(wc.random_field(N))
    h = N // 2
    dk[h, :, :] = 0.
    dk[:, h, :] = 0.
    dk[:, :, h] = 0.
    fac, H0 = 37.5, 70.
    for R in wc.SMOOTHINGS:
        S = wn.shear_tensor_k(wn.linear_velocity_k(dk, L, fac), L, R, H0)
        T = wn.tidal_tensor_k(dk, L, R)
        np.testing.assert_allclose(S, (fac / H0) * T, rtol=0, atol=1e-13 * np.max(np.abs(T)))
    # a velocity that is no gradient: the statement is the symmetrised gradient, by finite differences of the closed form
    v = wc.rotational_velocity(N, L)
    S = wn.shear_tensor(v, L, 0., H0)
    ky, kz, kx = 2 * np.pi * 2 / L[1], 2 * np.pi * 3 / L[2], 2 * np.pi / L[0]
    x, y, z = [np.arange(N).reshape([N if a == c else 1 for a in range(3)]) * (L[c] / N) for c in range(3)]
    one = np.ones((N, N, N))
    dxy = 40. * ky * np.cos(ky * y) - 10. * kx * np.sin(kx * x)              # d_y v_x + d_x v_y
    dxz = -30. * kx * np.cos(kx * x)                                         # d_z v_x + d_x v_z
    dyz = 25. * kz * np.cos(kz * z)                                          # d_z v_y + d_y v_z
    for q, want in ((3, dxy), (4, dxz), (5, dyz)):
        np.testing.assert_allclose(S[q], -(want * one) / (2. * H0), rtol=0, atol=1e-12)
    for q in range(3):
        assert np.max(np.abs(S[q])) <= 1e-12


def test_exact_matrices_and_classes():
    comp, lam = wc.exact_cube(16)
    got = wn.eigenvalues(comp)
    assert np.all(np.abs(got - lam) <= wn.eigen_bound(comp))
    np.testing.assert_array_equal(wn.classify(got, wc.INT_THRESHOLD), np.sum(lam > wc.INT_THRESHOLD, axis=0))
    bad, vox = wc.poisoned(comp)
    lb = wn.eigenvalues(bad)
    cls = wn.classify(lb, wc.INT_THRESHOLD)
    assert np.all(np.isnan(lb.reshape(3, -1)[:, vox])) and np.all(cls.ravel()[vox] == wn.NAN_CLASS)
    cnt, n_nan = wn.counts(cls)
    assert n_nan == vox.size == 7 and cnt.sum() + n_nan == 16 ** 3


def test_host_helpers():
    assert [web.class_index(k) for k in web.CLASS_NAMES] == [0, 1, 2, 3] and web.class_index(2) == 2
    for bad in ("wall", 4, -1, 1.5, True):
        with pytest.raises(ValueError):
            web.class_index(bad)
    assert web.field_bytes(16, "f32") == (16 ** 3 * 4, 16 * 17 * 16 * 8)
    assert web.field_bytes(512, "f64") == (512 ** 3 * 8, 512 * 513 * 272 * 16)
    real, half = web.field_bytes(64, "f32")
    assert web.web_device_bytes(64, "f32", stage="tensor") == 7 * half + 6 * real
    assert web.web_device_bytes(64, "f32", from_spectrum=True, stage="tensor") == 6 * half + 6 * real
    assert web.web_device_bytes(64, "f32", kind="shear", stage="tensor") == 9 * half + 6 * real
    assert web.web_device_bytes(64, "f32", eigenvalues=True, stage="classify") == 3 * real + 64 ** 3 + (1 << 20)
    assert web.web_device_bytes(64, "f32") >= web.web_device_bytes(64, "f32", stage="tensor")
    with pytest.raises(ValueError):
        web.web_device_bytes(64, "f16")
    with pytest.raises(ValueError):
        web.web_device_bytes(64, "f32", kind="density")
    t, scalar = web._check_thresholds(0.25)
    assert scalar and t.shape == (1,) and t[0] == 0.25
    t, scalar = web._check_thresholds([0., 0.5])
    assert not scalar and t.shape == (2,)
    for bad in ([0.5, 0.], [0., 0.], [np.nan], [np.inf], np.zeros((2, 2)), np.arange(17.), []):
        with pytest.raises(ValueError, match="threshold"):
            web._check_thresholds(bad)
    for bad in (-1., np.nan, np.inf):
        with pytest.raises(ValueError, match="smoothing"):
            web._check_smoothing(bad)
