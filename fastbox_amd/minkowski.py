"""
Minkowski functionals of excursion sets on the device: the morphological statistics of a field beside the moment statistics
(P(k), xi(r), the bispectrum).  For each threshold t the excursion set {field >= t} of the periodic box is a union of closed
voxels; its volume, surface, integrated mean curvature and Euler characteristic follow from the numbers of cells, faces, edges
and vertices of its cell complex (Schmalzing & Buchert 1997), which are integers and are counted exactly in one pass over the
cube.  Definition, conventions and limits: DESIGN.md section 4; numpy statement: tests/minkowski_numpy.py; kernel:
csrc/fb_minkowski.hip.

    mf = box.minkowski_functionals(nu=np.linspace(-3, 3, 25))          # MinkowskiFunctionals of box.delta_x
    mf.v0, mf.v1, mf.v2, mf.v3, mf.genus                                # per threshold
    s0, s1 = minkowski.spectral_moments(box, box.delta_x)
    minkowski.gaussian_minkowski(mf.nu, s0, s1)                         # what a Gaussian field of that spectrum gives
    ch = minkowski.minkowski_functionals(cube, nu=[-1., 0., 1.], per_channel=True)       # every channel as a 2-D map

The pure numpy functions (``minkowski_from_counts``, ``minkowski_from_counts_2d``, ``gaussian_minkowski``) need no GPU.
"""
import ctypes
import functools

import numpy as np

from . import _lib
from .device import DeviceArray, REAL

NT_MAX = 256
DEFAULT_NU = np.linspace(-3., 3., 25)
SPECTRAL_BINS = 1024                     # of spectral_moments: the most power_spectrum takes


# ---------------------------------------------------------------------- host arithmetic on the counts
def _sides(L, dim):
    L = np.asarray(L, dtype=np.float64)
    if L.ndim == 0:
        return tuple(float(L) for _ in range(dim))
    if L.shape != (dim,):
        raise ValueError("L: a box side or %d of them" % dim)
    return tuple(float(s) for s in L)


def minkowski_from_counts(n3, n2, n1, n0, N, L):
    """(V0, V1, V2, V3) per threshold from the counts of the cell complex of an excursion set in a periodic N^3 box of sides
    ``L`` (one number or (Lx, Ly, Lz)): n3 cells (nt,), n2 faces by normal (3, nt), n1 edges by direction (3, nt), n0 vertices
    (nt,).  With a_d = L_d / N, A_d the area of a face normal to d and V the box volume:

        V0 = n3 / N^3                                                    volume fraction
        V1 = (2 / 9V) sum_d (n2[d] - n3) A_d                             surface / (6 V): 2/3 of the lattice's
        V2 = (2 / 9V) sum_d (n1[d] - n2[e] - n2[f] + n3) a_d             integrated mean curvature density
        V3 = (n0 - sum n1 + sum n2 - n3) / V                             Euler characteristic density

    the Crofton estimates of Schmalzing & Buchert (1997), kept per orientation."""
    n3, n0 = np.asarray(n3, dtype=np.float64), np.asarray(n0, dtype=np.float64)
    n2, n1 = np.asarray(n2, dtype=np.float64), np.asarray(n1, dtype=np.float64)
    Ls = _sides(L, 3)
    a = [s / float(N) for s in Ls]
    V = Ls[0] * Ls[1] * Ls[2]
    v1 = np.zeros_like(n3)
    v2 = np.zeros_like(n3)
    for d in range(3):
        e, f = (d + 1) % 3, (d + 2) % 3
        v1 = v1 + (n2[d] - n3) * (a[e] * a[f])
        v2 = v2 + (n1[d] - n2[e] - n2[f] + n3) * a[d]
    chi = n0 - n1.sum(axis=0) + n2.sum(axis=0) - n3
    return n3 / float(N) ** 3, 2. * v1 / (9. * V), 2. * v2 / (9. * V), chi / V


def minkowski_from_counts_2d(n2, n1, n0, N, L):
    """(v0, v1, v2) per threshold of a periodic N^2 map of sides ``L`` (one number or (Lx, Ly)): n2 pixels (..., nt), n1 edges by
    direction (2, ..., nt), n0 vertices (..., nt).  With A = Lx Ly:

        v0 = n2 / N^2;  v1 = pi P / (16 A), P = sum_d 2 (n1[d] - n2) a_d the lattice perimeter;  v2 = (n0 - sum n1 + n2) / A

    (pi / 4 is the Crofton factor between the perimeter of a lattice body and that of the smooth body it samples)."""
    n2, n0 = np.asarray(n2, dtype=np.float64), np.asarray(n0, dtype=np.float64)
    n1 = np.asarray(n1, dtype=np.float64)
    Ls = _sides(L, 2)
    A = Ls[0] * Ls[1]
    P = sum(2. * (n1[d] - n2) * (Ls[d] / float(N)) for d in range(2))
    return n2 / float(N) ** 2, np.pi * P / (16. * A), (n0 - n1.sum(axis=0) + n2) / A


def gaussian_minkowski(nu, sigma0, sigma1, dim=3):
    """The expectations for a Gaussian random field (Tomita 1986) at nu = (t - mean) / sigma0, with sigma1^2 = <|grad|^2>.
    dim=3: (V0, V1, V2, V3) with lambda = sigma1 / (sigma0 sqrt(6 pi)); dim=2: (v0, v1, v2) with tau = sigma1^2 / (2 sigma0^2)."""
    from scipy.special import erfc
    nu = np.asarray(nu, dtype=np.float64)
    g = np.exp(-0.5 * nu * nu)
    v0 = 0.5 * erfc(nu / np.sqrt(2.))
    if dim == 3:
        lam = sigma1 / (sigma0 * np.sqrt(6. * np.pi))
        r = 1. / np.sqrt(2. * np.pi)
        return v0, (2. / 3.) * lam * r * g, (2. / 3.) * lam ** 2 * r * nu * g, lam ** 3 * r * (nu * nu - 1.) * g
    if dim == 2:
        tau = sigma1 ** 2 / (2. * sigma0 ** 2)
        return v0, np.sqrt(tau) / 8. * g, tau * nu * g / (2. * np.pi) ** 1.5
    raise ValueError("dim must be 2 or 3")


def spectral_moments(box, delta_x=None):
    """(sigma0, sigma1) of a real field of ``box`` from ``box.power_spectrum(mode='1d')``: sigma_j^2 = sum_b modes_b k_b^(2j)
    P_b / V over 1024 bins of equal width in k^2 up to the corner of the grid (every mode but k = 0, each counted once on the
    full grid; P = V |D|^2 / N^6, so j = 0 is Parseval's sum for the variance about the mean).  k_b is the mean |k| of a bin, so
    sigma1^2 carries at most the bin width k_corner^2 / 1024 as an error in k^2 -- and none on a cubic box of N <= 36, where the
    modes of a bin share one |k|: for a single plane wave sigma1 / sigma0 = |k| there."""
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    N = int(box.N)
    kmax = np.pi * N * np.sqrt(sum(1. / s ** 2 for s in L))            # |k| of the corner mode (N/2, N/2, N/2)
    edges = np.sqrt(np.linspace(0., kmax ** 2 * (1. + 1e-9), SPECTRAL_BINS + 1))
    k, power, modes = box.power_spectrum(delta_x, kbins=edges)
    ok = modes > 0
    V = L[0] * L[1] * L[2]
    s0 = np.sum(modes[ok] * power[ok]) / V
    s1 = np.sum(modes[ok] * k[ok] ** 2 * power[ok]) / V
    return float(np.sqrt(s0)), float(np.sqrt(s1))


# ---------------------------------------------------------------------- the result
class MinkowskiFunctionals(object):
    """The result of ``minkowski_functionals``.  ``thresholds`` (field units) and ``nu`` (or None), ``mean`` and ``sigma`` of the
    field (population standard deviation; with ``thresholds=`` they are not needed for the counts and are formed from the cube,
    which the result keeps for that, when first read), ``N``, ``L``, ``per_channel``.

    3-D: int64 counts ``n3`` (nt,), ``n2`` (3, nt) faces by normal, ``n1`` (3, nt) edges by direction, ``n0`` (nt,), ``euler``
    = n0 - sum n1 + sum n2 - n3, ``n_nan`` (voxels that are NaN: below every threshold); ``v0`` .. ``v3`` per threshold and
    ``genus`` = -euler / 2.

    Per channel (the last axis; every z-slice a periodic 2-D map): ``n2`` (N, nt) pixels, ``n1`` (2, N, nt) edges by direction,
    ``n0`` (N, nt), ``euler`` = n0 - sum n1 + n2, ``n_nan`` (N,); ``v0``, ``v1``, ``v2`` (N, nt); ``thresholds`` (nt,) or (N, nt),
    ``mean`` and ``sigma`` (N,)."""

    def __init__(self, moments=None, **kw):
        self.__dict__.update(kw)
        self._moments = moments              # (mean, sigma), or the call that forms them from the cube on first use

    def _moment(self, i):
        if callable(self._moments):
            self._moments = self._moments()
        return self._moments[i]

    mean = property(lambda self: self._moment(0))
    sigma = property(lambda self: self._moment(1))

    def __repr__(self):
        return "MinkowskiFunctionals(%s, N = %d, %d thresholds)" % ("per channel" if self.per_channel else "3-D", self.N,
                                                                    self.thresholds.shape[-1])


# ---------------------------------------------------------------------- arguments
def _field(field, box):
    """The real device cube and its engine; every check precedes the upload of a host array."""
    if isinstance(field, DeviceArray):
        if box is not None and field.engine is not box.engine:
            raise ValueError("field: a field of this box")
        if field.kind != REAL or field._as_complex:
            raise TypeError("field: a real field, not a complex one or a spectrum (take .real of a filtered field)")
        return field, field.engine
    if box is None:
        raise TypeError("field: a host array needs `box=` (the CosmoBox whose grid it lives on)")
    h = np.asarray(field)
    if np.iscomplexobj(h):
        raise TypeError("field: a real field, not a complex one")
    N = int(box.N)
    if h.shape != (N, N, N):
        raise ValueError("field: expected an array of shape %s, got %s" % ((N, N, N), h.shape))
    return box.engine.upload(h, REAL), box.engine


def _check_thresholds(t, N, per_channel):
    t = np.array(t, dtype=np.float64, order='C')            # a copy: the result keeps it
    if t.ndim == 0:
        t = t.reshape(1)
    if not (t.ndim == 1 or (per_channel and t.ndim == 2 and t.shape[0] == N)):
        raise ValueError("thresholds: shape (nt,)%s" % (", or (N, nt) with a row per channel" if per_channel else ""))
    if not 1 <= t.shape[-1] <= NT_MAX:
        raise ValueError("thresholds: between 1 and %d of them" % NT_MAX)
    if not np.all(np.isfinite(t)):
        raise ValueError("thresholds must be finite")
    if np.any(np.diff(t, axis=-1) <= 0.):
        raise ValueError("thresholds must be strictly ascending")
    return t


def _check_nu(nu):
    nu = np.array(nu, dtype=np.float64, order='C')
    if nu.ndim == 0:
        nu = nu.reshape(1)
    if nu.ndim != 1 or not 1 <= nu.size <= NT_MAX:
        raise ValueError("nu: between 1 and %d values, shape (nt,)" % NT_MAX)
    if not np.all(np.isfinite(nu)) or np.any(np.diff(nu) <= 0.):
        raise ValueError("nu must be finite and strictly ascending")
    return nu


def field_moments(cube, per_channel=False):
    """(mean, sigma) of a real device cube, sigma the population standard deviation: two ``sum_real`` reductions for the box, or
    per channel (arrays of N) fb_channel_means and fb_channel_moments about those means."""
    eng, N = cube.engine, cube.engine.N
    if not per_channel:
        n = float(N) ** 3
        mean = eng.sum_real(cube) / n
        var = eng.sum_real(cube, squared=True) / n - mean * mean
        return mean, float(np.sqrt(max(var, 0.)))
    mean_dev = eng._alloc_bytes(N * 8)
    mom_dev = eng._alloc_bytes(2 * N * 8)
    _lib.call("fb_channel_means", eng._plan, cube.ptr, mean_dev.ptr, eng.stream)
    _lib.call("fb_channel_moments", eng._plan, cube.ptr, mean_dev.ptr, mom_dev.ptr, eng.stream)
    mean, mom = eng.download_raw(mean_dev, N), eng.download_raw(mom_dev, (2, N))
    npix = float(N) ** 2
    d = mom[0] / npix                               # what rounding left of the mean
    return mean + d, np.sqrt(np.maximum(mom[1] / npix - d * d, 0.))


def _counts(eng, cube, thresholds, mode):
    N, nt = eng.N, thresholds.shape[-1]
    out = np.zeros((8, nt) if mode == 0 else (4, N, nt), dtype=np.uint64)
    nan = np.zeros(1 if mode == 0 else N, dtype=np.uint64)
    P_u64 = ctypes.POINTER(ctypes.c_uint64)
    _lib.call("fb_minkowski_counts", eng._plan, cube.ptr, thresholds.ctypes.data_as(_lib.P_double), nt, mode,
              out.ctypes.data_as(P_u64), nan.ctypes.data_as(P_u64), eng.stream)
    return out.astype(np.int64), nan.astype(np.int64)


def minkowski_functionals(field, thresholds=None, nu=None, per_channel=False, box=None):
    """The Minkowski functionals of the excursion sets {field >= t} of a periodic box, or with ``per_channel`` of every
    frequency channel (z-slice) as a periodic 2-D map; a ``MinkowskiFunctionals``.

    ``field``: a real DeviceArray, or a host (N, N, N) array together with ``box=``.  ``thresholds``: field units, strictly
    ascending, 1 to 256 of them, shape (nt,) -- or (N, nt) with ``per_channel``, a row per channel.  ``nu``: thresholds mean +
    nu sigma, with the mean and the population sigma of the cube, or of each channel (ValueError for a channel with sigma = 0).
    Neither: nu = np.linspace(-3, 3, 25); both: ValueError.  With ``thresholds=`` the call is one pass over the cube; ``nu=``
    adds the moment reductions (two more reads).  The comparison is field >= t in fp64 on the stored value; a NaN
    voxel is below every threshold (counted in ``n_nan``), +inf above every one.  Bad arguments raise before any device work."""
    if thresholds is not None and nu is not None:
        raise ValueError("give thresholds or nu, not both")
    per_channel = bool(per_channel)
    if isinstance(field, DeviceArray):
        N = field.engine.N
    elif box is not None:
        N = int(box.N)
    else:
        raise TypeError("field: a host array needs `box=` (the CosmoBox whose grid it lives on)")
    if thresholds is not None:
        thresholds = _check_thresholds(thresholds, N, per_channel)
    else:
        nu = _check_nu(DEFAULT_NU if nu is None else nu)
    cube, eng = _field(field, box)
    moments = functools.partial(field_moments, cube, per_channel)      # thresholds=: formed only if the result is asked
    if nu is not None:
        moments = mean, sigma = field_moments(cube, per_channel)
        if not np.all(np.isfinite(mean)) or not np.all(np.isfinite(sigma)):
            raise ValueError("nu: the field's mean and sigma are not finite (NaN or inf voxels): give thresholds")
        if np.any(sigma == 0.):
            raise ValueError("nu: %s has sigma = 0" % ("a channel" if per_channel else "the field"))
        thresholds = (mean[:, None] + nu[None, :] * sigma[:, None]) if per_channel else mean + nu * sigma
        thresholds = _check_thresholds(thresholds, N, per_channel)
    mode = 0 if not per_channel else (1 if thresholds.ndim == 1 else 2)
    cnt, nan = _counts(eng, cube, thresholds, mode)
    L = eng.L
    common = dict(thresholds=thresholds, nu=nu, moments=moments, N=N, L=L, per_channel=per_channel)
    if not per_channel:
        n3, n2, n1, n0 = cnt[0], cnt[1:4], cnt[4:7], cnt[7]
        euler = n0 - n1.sum(axis=0) + n2.sum(axis=0) - n3
        v0, v1, v2, v3 = minkowski_from_counts(n3, n2, n1, n0, N, L)
        return MinkowskiFunctionals(n3=n3, n2=n2, n1=n1, n0=n0, euler=euler, n_nan=int(nan[0]), v0=v0, v1=v1, v2=v2, v3=v3,
                                    genus=-0.5 * euler, **common)
    n2, n1, n0 = cnt[0], cnt[1:3], cnt[3]
    euler = n0 - n1.sum(axis=0) + n2
    v0, v1, v2 = minkowski_from_counts_2d(n2, n1, n0, N, L[:2])
    return MinkowskiFunctionals(n2=n2, n1=n1, n0=n0, euler=euler, n_nan=nan, v0=v0, v1=v1, v2=v2, genus=-0.5 * euler, **common)
