"""Constructed inputs for the cosmic-web kernels (fb_web.hip), numpy only: plane waves whose tidal tensor is known in closed
form, a seeded random field, single modes on the Nyquist planes, a non-potential velocity, and symmetric 3 x 3 matrices whose
eigenvalues are known exactly -- diagonal ones in every order, the same turned by the exact 3-4-5 rotation about each axis,
equal eigenvalues, rank one, zero, and scalings by 1e+-6.  tests/test_web_cases_cpu.py holds the numpy statement
(tests/web_numpy.py) to these cases; tests/test_web_gpu.py runs them on the device."""
import itertools

import numpy as np

from tests import recon_cases as rc
from tests import web_numpy as wn

geometries = rc.geometries
WAVES = rc.WAVES                                 # none on a Nyquist plane
plane_wave = rc.plane_wave
random_field = rc.random_field
nyquist_mode_spectrum = rc.nyquist_mode_spectrum
AMPLITUDE = 0.25
SMOOTHINGS = (0., 3.)
EIGEN_N = (16, 18, 30)                           # 30^3 = 27000 voxels: a tail in the last wave and the last workgroup
INT_THRESHOLD = 0.5


def plane_wave_tidal(N, L, mode, R, A=AMPLITUDE):
    """(T (6, N, N, N), delta, s) of plane_wave in closed form: T_ij = khat_i khat_j s delta with s = exp(-k0^2 R^2 / 2)."""
    delta, k0 = plane_wave(N, L, mode, A)
    k2 = float(np.dot(k0, k0))
    s = np.exp(-0.5 * k2 * R * R)
    return np.array([(k0[i] * k0[j] / k2) * s * delta for i, j in wn.PAIRS]), delta, s


def rotational_velocity(N, L):
    """Three real cubes that are no gradient: v = (A sin(k_y y), B sin(k_z z) + C cos(k_x x), D sin(k_x x)), km/s."""
    x, y, z = rc._coords(N, L)
    kx, ky, kz = 2 * np.pi / L[0], 2 * np.pi * 2 / L[1], 2 * np.pi * 3 / L[2]
    one = np.ones((N, N, N))
    return [40. * np.sin(ky * y) * one, (25. * np.sin(kz * z) + 10. * np.cos(kx * x)) * one, -30. * np.sin(kx * x) * one]


def _rot345(axis):
    """5 times the rotation by atan(4/3) about an axis: integer entries."""
    a, b = [c for c in range(3) if c != axis]
    R = np.zeros((3, 3))
    R[axis, axis] = 5.
    R[a, a], R[a, b], R[b, a], R[b, b] = 3., -4., 4., 3.
    return R


def exact_matrices():
    """[(A (3, 3), eigenvalues descending)] with integer (or exactly scaled integer) entries and eigenvalues."""
    out = []
    diags = sorted(set(itertools.permutations((3., 1., -2.))) | set(itertools.permutations((2., 2., -1.)))
                   | set(itertools.permutations((0., 1., 4.))))
    for d in diags:
        out.append((np.diag(d), sorted(d, reverse=True)))
        for axis in range(3):                                   # R D R^T with D = 25 d: (5 R) d (5 R)^T in integers
            R5 = _rot345(axis)
            out.append((R5 @ np.diag(d) @ R5.T, sorted((25. * v for v in d), reverse=True)))
    out.append((np.diag((1., 1., 1.)), [1., 1., 1.]))
    out.append((np.diag((2., 1., 1.)), [2., 1., 1.]))
    v = np.array([1., 2., -2.])
    out.append((np.outer(v, v), [9., 0., 0.]))                  # rank one
    out.append((-np.outer(v, v), [0., 0., -9.]))
    out.append((np.ones((3, 3)), [3., 0., 0.]))
    out.append((np.zeros((3, 3)), [0., 0., 0.]))
    base = list(out)
    for A, lam in base[:12] + base[-6:]:
        for s in (1e6, 1e-6):
            out.append((A * s, [x * s for x in lam]))
    return out


def exact_cube(N):
    """(comp (6, N, N, N), lam (3, N, N, N)): voxel v of the flattened cube holds matrix v mod the number of matrices."""
    mats = exact_matrices()
    idx = np.arange(N ** 3) % len(mats)
    A = np.array([m for m, _ in mats])[idx]
    lam = np.array([l for _, l in mats])[idx]
    comp = np.array([A[:, i, j] for i, j in wn.PAIRS]).reshape(6, N, N, N)
    return comp, lam.T.reshape(3, N, N, N).copy()


def poisoned(comp, seed=8):
    """(comp with a few NaN and +-inf components, the flat indices of the voxels hit): 7 voxels, one component each -- and one
    voxel with two."""
    rs = np.random.RandomState(seed)
    out = np.array(comp, dtype=np.float64)
    nv = out[0].size
    vox = rs.choice(nv, 7, replace=False)
    vox[0], vox[1] = 0, nv - 1                                  # the first and the last voxel among them
    flat = out.reshape(6, -1)
    for n, v in enumerate(vox):
        flat[n % 6, v] = (np.nan, np.inf, -np.inf)[n % 3]
    flat[5, vox[2]] = np.nan
    return out, np.sort(vox)
