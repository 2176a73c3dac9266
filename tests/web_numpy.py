"""numpy statement of the cosmic-web classification (fastbox_amd/web.py; fb_web.hip): the tidal tensor of
a density (T-web, Hahn et al. 2007, Forero-Romero et al. 2009), the shear tensor of a velocity (V-web, Hoffman et al. 2012),
their eigenvalues and the void / sheet / filament / knot classes.  np.fft and np.linalg.eigvalsh, fp64 throughout unless a
stage is given ``dtype``, the type the device stores its fields in: the transforms then run in it (scipy.fft keeps float32)
and all other arithmetic stays fp64, as on the device.

Fourier convention as numpy: f(x) = sum f(k) exp(+i k.x), k_a = 2 pi m_a / L_a, m_a the signed FFT index (N/2 -> -N/2).
Components are in the order xx, yy, zz, xy, xz, yz.  tests/test_web_cases_cpu.py validates this file on its own."""
import numpy as np
import scipy.fft

from tests.recon_numpy import kvec, rfftn, stored          # noqa: F401  (re-exported for the tests)

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
NAMES = ("xx", "yy", "zz", "xy", "xz", "yz")
CLASS_NAMES = ("void", "sheet", "filament", "knot")
NAN_CLASS = 255


def _grids(N, L, full):
    """(K, M, k2, window argument) broadcast over the full (N, N, N) or the half (N, N, N/2 + 1) spectrum."""
    m, k = kvec(N, L)
    nz = N if full else N // 2 + 1
    K = [k[0].reshape(N, 1, 1), k[1].reshape(1, N, 1), k[2][:nz].reshape(1, 1, nz)]
    M = [m.reshape(N, 1, 1), m.reshape(1, N, 1), m[:nz].reshape(1, 1, nz)]
    return K, M, (K[0] * K[0] + K[1] * K[1]) + K[2] * K[2]


def tidal_multipliers(N, L, R, full=False):
    """The six real multipliers k_i k_j exp(-k^2 R^2 / 2) / k^2: zero at k = 0; for i != j zero wherever m_i = -N/2 or
    m_j = -N/2 (an odd power of a Nyquist component); the diagonal keeps its Nyquist planes."""
    K, M, k2 = _grids(N, L, full)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.exp(-0.5 * (k2 * (R * R))) / k2
    w[0, 0, 0] = 0.
    out = []
    for i, j in PAIRS:
        r = (K[i] * K[j]) * w
        if i != j:
            r = np.where((M[i] == -(N // 2)) | (M[j] == -(N // 2)), 0., r)
        out.append(r)
    return out


def _c2r(spec, N, dtype):
    if np.dtype(dtype) == np.float64:
        return np.fft.irfftn(spec, s=(N, N, N), axes=(0, 1, 2))
    return scipy.fft.irfftn(spec.astype(np.complex64), s=(N, N, N), axes=(0, 1, 2)).astype(np.float64)


def tidal_tensor_k(dk_half, L, R=0., dtype=np.float64):
    """T (6, N, N, N) from the half spectrum delta(k) (N, N, N/2 + 1): the 1/N^3 inverse transforms of
    k_i k_j / k^2 exp(-k^2 R^2 / 2) delta(k)."""
    N = dk_half.shape[0]
    dk = dk_half.astype(np.complex128)
    return np.array([_c2r(r * dk, N, dtype) for r in tidal_multipliers(N, L, R)])


def tidal_tensor(delta, L, R=0., dtype=np.float64):
    """T (6, N, N, N) of a real field."""
    return tidal_tensor_k(rfftn(stored(delta, dtype), dtype), L, R, dtype)


def tidal_tensor_full(delta, L, R=0.):
    """The same through ifftn of the full spectrum, complex (6, N, N, N): with the Nyquist rules its imaginary part is rounding."""
    N = delta.shape[0]
    dk = np.fft.fftn(np.asarray(delta, dtype=np.float64))
    return np.array([np.fft.ifftn(r * dk) for r in tidal_multipliers(N, L, R, full=True)])


def shear_tensor_k(vk_half, L, R=0., H0=100., dtype=np.float64):
    """Sigma (6, N, N, N) from the three half spectra v_a(k): the inverse transforms of
    -(i / 2 H0) (k_i v_j + k_j v_i) exp(-k^2 R^2 / 2), the term k_i v_j zero where m_i = -N/2."""
    N = vk_half[0].shape[0]
    K, M, k2 = _grids(N, L, False)
    g = np.exp(-0.5 * (k2 * (R * R))) / (2. * H0)
    Kz = [np.where(M[a] == -(N // 2), 0., K[a]) for a in range(3)]
    v = [np.asarray(vk_half[a]).astype(np.complex128) for a in range(3)]
    return np.array([_c2r(-1j * (Kz[i] * v[j] + Kz[j] * v[i]) * g, N, dtype) for i, j in PAIRS])


def shear_tensor(vel, L, R=0., H0=100., dtype=np.float64):
    """Sigma (6, N, N, N) of three real velocity cubes (km/s; H0 in km/s/Mpc)."""
    return shear_tensor_k([rfftn(stored(v, dtype), dtype) for v in vel], L, R, H0, dtype)


def linear_velocity_k(dk_half, L, fac):
    """v_a(k) = i fac k_a delta(k) / k^2, zero at k = 0 and on the plane m_a = -N/2: ``realise_velocity`` with fac = f H a."""
    N = dk_half.shape[0]
    K, M, k2 = _grids(N, L, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = fac / k2
    w[0, 0, 0] = 0.
    return [np.where(M[a] == -(N // 2), 0., 1j * (K[a] * w) * dk_half) for a in range(3)]


def matrices(comp):
    """(..., 3, 3) symmetric matrices from components (6, ...)."""
    c = np.asarray(comp, dtype=np.float64)
    out = np.empty(c.shape[1:] + (3, 3))
    for q, (i, j) in enumerate(PAIRS):
        out[..., i, j] = c[q]
        out[..., j, i] = c[q]
    return out


def eigenvalues(comp):
    """(3, ...) lambda_1 >= lambda_2 >= lambda_3 per voxel; three NaN where a component is not finite."""
    A = matrices(comp)
    bad = ~np.all(np.isfinite(A), axis=(-2, -1))
    A[bad] = 0.
    lam = np.linalg.eigvalsh(A)[..., ::-1]
    lam[bad] = np.nan
    return np.moveaxis(lam, -1, 0)


def classify(lam, threshold):
    """uint8 classes: the number of eigenvalues > threshold (0 void, 1 sheet, 2 filament, 3 knot); 255 where lam is NaN."""
    lam = np.asarray(lam)
    cls = np.sum(lam > threshold, axis=0).astype(np.uint8)
    cls[np.isnan(lam[0])] = NAN_CLASS
    return cls


def counts(cls):
    """(counts[4], n_nan) of a class cube."""
    b = np.bincount(np.asarray(cls).ravel(), minlength=256)
    return b[:4].astype(np.int64), int(b[NAN_CLASS])


def eigen_bound(comp, dtype=np.float64):
    """Per voxel: 1024 * 2^-53 * ||A||_F, the backward-stability bound the device solver is held to."""
    A = matrices(comp)
    return 1024. * 2. ** -53 * np.sqrt(np.sum(A * A, axis=(-2, -1)))
