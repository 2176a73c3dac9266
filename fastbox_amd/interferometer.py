"""An interferometer on top of a box: uv coverage per frequency channel, dirty cubes, the point-spread function and
visibility noise, on the device.  Definitions, conventions and what is out of scope: DESIGN.md section 4.

A baseline of fixed length b samples u = b nu / c: it walks outward through the transverse Fourier plane as the frequency
changes, so a (k_perp) cell is sampled in some channels and not in others.  ``Interferometer.observe`` applies exactly that
sampling to a cube -- per channel ``ifft2(fft2(A T) f(S)) N^2 / w`` -- which is what throws smooth-spectrum foreground power
up to k_par ~ k_perp (the wedge) in ``cylindrical_power_spectrum`` of the result.

The pure-numpy helpers at the top (array layouts, baselines, rotation synthesis, the channel tables, collapsing of redundant
samples) need no GPU.  The sky is flat, the whole box sits at one distance, and a sample lands on the nearest cell of the
transform's own (u, v) grid: there is no gridding kernel and no w-term.
"""
import ctypes

import numpy as np

from . import _lib
from . import box as _box
from .device import DeviceBuffer, FULL, REAL
from .sky import _Maps

_ccl = _box._ccl

C_LIGHT = 299792458.                # m / s
WEIGHTINGS = {"natural": 0, "uniform": 1}
_MODE_SQRT = 2
_COUNT_MAX = 2 ** 31 - 1


# ---- host helpers (numpy only) ------------------------------------------------------------------------------------------------
def baselines_from_antennas(xy):
    """All pairs i < j of antenna positions (n, 2) or ENU (n, 3), in metres: x_j - x_i, shape (n (n - 1) / 2, 2 or 3), in the
    order of ``np.triu_indices(n, 1)``."""
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] not in (2, 3):
        raise ValueError("antenna positions: an (n, 2) or (n, 3) array")
    i, j = np.triu_indices(xy.shape[0], 1)
    return xy[j] - xy[i]


def hex_array(n_side, spacing):
    """Antenna positions (3 n_side^2 - 3 n_side + 1, 2) of a filled hexagon with n_side antennas along each side, nearest
    neighbours `spacing` metres apart, centred on the origin (n_side = 11: 331 antennas)."""
    n = int(n_side)
    if n < 1:
        raise ValueError("hex_array: n_side >= 1")
    rows = []
    for r in range(-(n - 1), n):
        cnt = 2 * n - 1 - abs(r)
        x = (np.arange(cnt) - 0.5 * (cnt - 1)) * spacing
        rows.append(np.stack([x, np.full(cnt, r * spacing * np.sqrt(3.) / 2.)], axis=1))
    return np.concatenate(rows)


def grid_array(nx, ny, spacing):
    """Antenna positions (nx ny, 2) of a rectangular grid, `spacing` metres (a number, or (East, North)), centred on the origin."""
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1:
        raise ValueError("grid_array: nx, ny >= 1")
    sx, sy = (spacing, spacing) if np.isscalar(spacing) else spacing
    x = (np.arange(nx) - 0.5 * (nx - 1)) * sx
    y = (np.arange(ny) - 0.5 * (ny - 1)) * sy
    return np.stack([np.repeat(x, ny), np.tile(y, nx)], axis=1)


def rotation_synthesis(baselines_enu, latitude, declination, hour_angles):
    """Projected baselines (u, v) in metres, shape (nbl nt, 2) -- baseline-major, hour angles in the order given -- of
    baselines (nbl, 3) East, North, Up (or (nbl, 2): Up = 0) at `latitude`, towards `declination`, at `hour_angles`; all
    angles in radians.  The standard equatorial formulas:

        X = -N sin(lat) + U cos(lat),   Y = E,   Z = N cos(lat) + U sin(lat)
        u =  X sin(H) + Y cos(H)
        v = -X sin(dec) cos(H) + Y sin(dec) sin(H) + Z cos(dec)
    """
    b = np.asarray(baselines_enu, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] not in (2, 3):
        raise ValueError("baselines: an (n, 2) or (n, 3) array")
    E, N = b[:, 0], b[:, 1]
    U = b[:, 2] if b.shape[1] == 3 else np.zeros(b.shape[0])
    lat, dec = float(latitude), float(declination)
    H = np.atleast_1d(np.asarray(hour_angles, dtype=np.float64))[None, :]
    X = (-N * np.sin(lat) + U * np.cos(lat))[:, None]
    Y = E[:, None]
    Z = (N * np.cos(lat) + U * np.sin(lat))[:, None]
    u = X * np.sin(H) + Y * np.cos(H)
    v = -X * np.sin(dec) * np.cos(H) + Y * np.sin(dec) * np.sin(H) + Z * np.cos(dec)
    return np.stack([u.ravel(), v.ravel()], axis=1)


def uv_cell(box, redshift=None):
    """(du, dv): the (u, v) cell of the per-channel N-point transform in wavelengths, du = r / Lx and dv = r / Ly with
    r = comoving_angular_distance(cosmo, 1 / (1 + redshift)) (``redshift`` defaults to the box's)."""
    z = box.redshift if redshift is None else redshift
    r = _ccl.comoving_angular_distance(box.cosmo, 1. / (1. + z))
    if not r > 0.:
        raise ValueError("the box needs a redshift > 0: at distance 0 it subtends no angle")
    return r / box.Lx, r / box.Ly


def channel_scales(box, redshift=None):
    """(sx, sy), fp64 (N,): cells per metre of baseline in every channel, nu_c 1e6 / c / du with nu_c = box.freq_array()[c] in
    MHz, formed in exactly this order (the count rule multiplies a baseline component by them and rounds)."""
    du, dv = uv_cell(box, redshift)
    nu = np.asarray(box.freq_array(redshift=redshift), dtype=np.float64)
    return np.ascontiguousarray(nu * 1e6 / C_LIGHT / du), np.ascontiguousarray(nu * 1e6 / C_LIGHT / dv)


def collapse_samples(samples, multiplicity=None):
    """(unique rows, int32 multiplicities) of an (ns, 2) sample array: ``np.unique`` on the exact fp64 pairs; multiplicities
    the samples already carry are summed over equal rows.  A redundant array then sends one weighted add per distinct
    baseline instead of hammering one cell with thousands."""
    s = _as_samples(samples)
    if s.shape[0] == 0:
        return s, np.zeros(0, dtype=np.int32)
    uniq, inv = np.unique(s, axis=0, return_inverse=True)
    mult = np.bincount(np.ravel(inv), weights=multiplicity, minlength=uniq.shape[0])      # (exact: the sums stay below 2^31)
    return np.ascontiguousarray(uniq), mult.astype(np.int32)


def _as_samples(samples):
    s = np.ascontiguousarray(samples, dtype=np.float64)
    if s.size == 0:
        return s.reshape(0, 2)
    if s.ndim != 2 or s.shape[1] != 2:
        raise ValueError("uv samples: an (ns, 2) array")
    return s


# ---- results ----------------------------------------------------------------------------------------------------------------------
class DeviceCounts(DeviceBuffer):
    """The int32 (N, N, N) coverage cube in device memory; ``host()`` copies it out."""

    def __init__(self, engine, buf):
        DeviceBuffer.__init__(self, engine, buf, (engine.N,) * 3, np.int32)


class UVCoverage(object):
    """counts: DeviceCounts S[u][v][c]; tot, ncell: int64 (N,) sum and number of sampled cells per channel; empty_channels:
    the channels with tot = 0; du, dv: the (u, v) cell in wavelengths; n_samples: the samples counted, multiplicities included."""

    def __init__(self, counts, tot, ncell, du, dv, n_samples):
        self.counts, self.tot, self.ncell = counts, tot, ncell
        self.empty_channels = np.flatnonzero(tot == 0)
        self.du, self.dv, self.n_samples = du, dv, n_samples


class Observation(object):
    """dirty: the dirty cube (noise included when sigma was given); noise: the noise cube on its own, or None; psf: the
    point-spread function, or None; coverage: the UVCoverage; weighting."""

    def __init__(self, dirty, noise, psf, coverage, weighting):
        self.dirty, self.noise, self.psf, self.coverage, self.weighting = dirty, noise, psf, coverage, weighting


# ---- the instrument ---------------------------------------------------------------------------------------------------------------
class Interferometer(object):

    def __init__(self, box, antennas=None, baselines=None, latitude=None, declination=None, hour_angles=None, redshift=None,
                 multiplicity=None):
        """box: a CosmoBox of even N.  Give ``antennas`` ((n, 2) or ENU (n, 3) positions in metres: all pairs are taken) or
        ``baselines`` ((nbl, 2) or (nbl, 3)) directly.  With ``latitude``, ``declination`` and ``hour_angles`` (radians) the
        baselines are projected by ``rotation_synthesis``; with none of them their (East, North) components are the samples
        (a snapshot at the zenith).  ``multiplicity``: integer copies of each baseline (default 1).  ``redshift``: where
        the angular scale and the channel frequencies are taken (default: the box's).  ValueError for samples that are not
        finite or whose doubled multiplicities exceed the int32 counts; no device work happens here."""
        if box.N % 2:
            raise ValueError("Interferometer: the box needs an even N")
        if (antennas is None) == (baselines is None):
            raise ValueError("Interferometer: give antennas or baselines (one of them)")
        self.box, self.redshift = box, redshift
        bl = baselines_from_antennas(antennas) if antennas is not None else np.asarray(baselines, dtype=np.float64)
        if bl.size == 0:
            bl = bl.reshape(0, 2)
        if bl.ndim != 2 or bl.shape[1] not in (2, 3):
            raise ValueError("baselines: an (n, 2) or (n, 3) array")
        synth = (latitude, declination, hour_angles)
        if any(a is not None for a in synth):
            if any(a is None for a in synth):
                raise ValueError("rotation synthesis needs latitude, declination and hour_angles together")
            nt = np.atleast_1d(np.asarray(hour_angles)).size
            samples = rotation_synthesis(bl, latitude, declination, hour_angles)
        else:
            nt = 1
            samples = np.ascontiguousarray(bl[:, :2])
        if multiplicity is None:
            mult = np.ones(samples.shape[0], dtype=np.int64)
        else:
            mult = np.asarray(multiplicity)
            if mult.shape != (bl.shape[0],) or not np.issubdtype(mult.dtype, np.integer) or (mult < 1).any():
                raise ValueError("multiplicity: one integer >= 1 per baseline")
            mult = np.repeat(mult.astype(np.int64), nt)
        if not np.isfinite(samples).all():
            raise ValueError("uv samples must be finite")
        if 2 * int(mult.sum()) > _COUNT_MAX:
            raise ValueError("2 x the number of samples (multiplicities included) must not exceed 2^31 - 1: the counts are int32")
        self._samples, self._mult = samples, mult
        self._coverage = None

    def uv_samples(self):
        """The projected baselines (ns, 2) in metres, fp64, before redundant ones are collapsed."""
        return self._samples

    def _collapsed(self):
        """Distinct samples and their int32 multiplicities: what goes to the device."""
        return collapse_samples(self._samples, self._mult)

    def uv_coverage(self):
        """The UVCoverage of this instrument on the box's grid (computed once, kept on the object)."""
        if self._coverage is not None:
            return self._coverage
        eng = self.box.engine
        N = eng.N
        eng.need_memory(4 * N ** 3 + eng.nbytes[FULL], "uv_coverage: a %d^3 box takes" % self.box.N)
        samples, mult = self._collapsed()
        sx, sy = channel_scales(self.box, self.redshift)
        du, dv = uv_cell(self.box, self.redshift)
        ns = samples.shape[0]
        s_dev = eng.upload_raw(samples) if ns else None
        m_dev = eng.upload_raw(mult) if ns else None
        sx_dev, sy_dev = eng.upload_raw(sx), eng.upload_raw(sy)
        counts = DeviceCounts(eng, eng._alloc_bytes(4 * N ** 3))
        sums_dev = eng._alloc_bytes(16 * N)
        _lib.call("fb_uv_coverage", eng._plan, s_dev.ptr if ns else None, m_dev.ptr if ns else None, ns, sx_dev.ptr, sy_dev.ptr,
                  counts.ptr, 0, eng.stream)
        _lib.call("fb_uv_channel_sums", eng._plan, counts.ptr, sums_dev.ptr, eng.stream)
        sums = eng.download_raw(sums_dev, (2, N), np.int64)
        self._coverage = UVCoverage(counts, sums[0].copy(), sums[1].copy(), du, dv, int(self._mult.sum()))
        return self._coverage

    # -- the sampling operator ----------------------------------------------------------------------------------------------
    def _apply(self, real, mode, scale):
        """Re ifft2(fft2(real) f(S) scale[c]) per channel; `real` is not modified."""
        eng = self.box.engine
        cov = self.uv_coverage()
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        scale_dev = eng.upload_raw(scale)
        full = eng.empty(FULL)
        out = eng.empty(REAL)
        _lib.call("fb_real_to_complex", eng._plan, real.ptr, full.ptr, eng.stream)
        _lib.call("fb_fft_transverse", eng._plan, full.ptr, -1, eng.stream)
        _lib.call("fb_uv_weight", eng._plan, full.ptr, cov.counts.ptr, int(mode), scale_dev.ptr, eng.stream)
        _lib.call("fb_fft_transverse", eng._plan, full.ptr, +1, eng.stream)
        _lib.call("fb_complex_to_real", eng._plan, full.ptr, out.ptr, eng.stream)
        eng.sync()                           # `scale` must outlive the copy
        return out

    def _normaliser(self, weighting):
        """N^2 / w[c] (0 in an empty channel): fb_fft_transverse(+1) divides by N^2 like np.fft.ifft2."""
        cov = self.uv_coverage()
        w = (cov.tot if weighting == "natural" else cov.ncell).astype(np.float64)
        scale = np.zeros(self.box.N)
        np.divide(float(self.box.N) ** 2, w, out=scale, where=w > 0)
        return scale

    def _zeros(self):
        """A real cube of zeros (fb_uv_coverage without samples clears 4 N^3 bytes)."""
        eng = self.box.engine
        out = eng.empty(REAL)
        tab = eng.upload_raw(np.zeros(eng.N))
        for off in range(0, eng.nbytes[REAL], 4 * eng.N ** 3):
            _lib.call("fb_uv_coverage", eng._plan, None, None, 0, tab.ptr, tab.ptr, out.ptr + off, 0, eng.stream)
        eng.sync()
        return out

    @staticmethod
    def _check_weighting(weighting):
        if weighting not in WEIGHTINGS:
            raise ValueError("weighting must be 'natural' or 'uniform'")

    def _check_sigma(self, sigma, weighting):
        s = np.asarray(sigma, dtype=np.float64)
        if s.shape not in ((), (self.box.N,)) or not np.isfinite(s).all() or (s < 0).any():
            raise ValueError("sigma: a non-negative number, or one per channel")
        if weighting != "natural":
            raise ValueError("the noise cube is defined for natural weighting only (DESIGN.md section 4)")
        return np.broadcast_to(s, (self.box.N,))

    def psf(self, weighting="natural"):
        """The point-spread function: the dirty cube of a unit impulse at pixel (0, 0) of every channel; 1 there in every
        channel that is not empty.  A real DeviceArray."""
        self._check_weighting(weighting)
        eng = self.box.engine
        eng.need_memory((0 if self._coverage is not None else 4 * eng.N ** 3) + eng.nbytes[FULL],
                        "psf: a %d^3 box takes" % self.box.N)
        imp = self._zeros()
        ones = np.ones(eng.N, dtype=eng.rdtype)                         # pixel (0, 0) of every channel: the first N values
        _lib.call("fb_memcpy_h2d", imp.ptr, ones.ctypes.data_as(ctypes.c_void_p), ones.nbytes, eng.stream)
        eng.sync()
        return self._apply(imp, WEIGHTINGS[weighting], self._normaliser(weighting))

    def noise(self, sigma, weighting="natural"):
        """The noise cube of naturally weighted visibilities: N sigma_c ifft2(sqrt(S) fft2(g)) / tot[c] for a unit white real
        cube g, whose per-pixel variance is exactly sigma_c^2 / tot[c].  ``sigma``: the rms modulus of the noise of ONE
        visibility sample, in the units of the cube, a number or (N,) per channel -- converting a system temperature,
        bandwidth and integration time into it is the caller's business.  g follows the box: rng='numpy' draws
        ``np.random.normal`` on the host, rng='device' the counter generator with the box's next sky seed."""
        self._check_weighting(weighting)
        sig = self._check_sigma(sigma, weighting)
        box, eng = self.box, self.box.engine
        N = eng.N
        eng.need_memory((0 if self._coverage is not None else 4 * N ** 3) + eng.nbytes[FULL], "noise: a %d^3 box takes" % box.N)
        cov = self.uv_coverage()
        if box.rng == "numpy":
            g = eng.upload(np.random.normal(0., 1., (N, N, N)), REAL)
        else:
            g = eng.empty(REAL)
            one = np.ones(N)
            _lib.call("fb_sky_noise_cube", eng._plan, one.ctypes.data_as(_lib.P_double), None, _Maps(box).next_seed(), g.ptr,
                      eng.stream)
            eng.sync()                       # `one` must outlive the copy
        tot = cov.tot.astype(np.float64)
        scale = np.zeros(N)
        np.divide(float(N) * sig, tot, out=scale, where=tot > 0)
        return self._apply(g, _MODE_SQRT, scale)

    def observe(self, cube, weighting="natural", primary_beam=None, sigma=None, return_psf=False):
        """The dirty cube of `cube` (a real DeviceArray or a host (N, N, N) array): per channel
        ``ifft2(fft2(A T) f(S)) N^2 / w`` with f(S) = S, w = tot ('natural') or f(S) = [S > 0], w = ncell ('uniform');
        a channel no sample reaches is exactly 0.  ``primary_beam``: a BeamModel (its ``beam_cube()``), a cube, or None.
        ``sigma``: see ``noise`` -- the noise is added to ``dirty`` and kept in ``noise``.  Returns an ``Observation``."""
        self._check_weighting(weighting)
        sig = None if sigma is None else self._check_sigma(sigma, weighting)
        box, eng = self.box, self.box.engine
        N = eng.N
        if tuple(np.shape(cube)) != (N, N, N):
            raise ValueError("expected a cube of shape %s, got %s" % ((N, N, N), tuple(np.shape(cube))))
        beam = primary_beam.beam_cube() if hasattr(primary_beam, "beam_cube") else primary_beam
        if beam is not None and tuple(np.shape(beam)) != (N, N, N):
            raise ValueError("expected a primary-beam cube of shape %s, got %s" % ((N, N, N), tuple(np.shape(beam))))
        eng.need_memory((0 if self._coverage is not None else 4 * N ** 3) + eng.nbytes[FULL], "observe: a %d^3 box takes" % box.N)
        cov = self.uv_coverage()
        field = box._as_real(cube)
        if beam is not None:
            field = eng.multiply(box._as_real(beam), field)
        dirty = self._apply(field, WEIGHTINGS[weighting], self._normaliser(weighting))
        noise = None
        if sig is not None:
            noise = self.noise(sig, weighting)
            dirty = eng.axpby(dirty, noise, 1.0, 1.0, 0.0)
        psf = self.psf(weighting) if return_psf else None
        return Observation(dirty, noise, psf, cov, weighting)
