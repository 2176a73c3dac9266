"""
Halo tracers on the device: the counterpart of the reference's fastbox/halos.py.

    from fastbox_amd.halos import HaloDistribution          # as fastbox.halos
    halos = HaloDistribution(box, mass_range=(1e12, 1e15), mass_bins=10)
    counts = halos.halo_count_field(box.delta_x, nbar=1e-3, bias=1.)      # real DeviceArray of integer counts
    cat = halos.realise_halo_catalogue(counts, scatter=True)               # HaloCatalogue, (Nh, 3) fp64 on the device
    mesh = box.paint_catalogue(cat, window='tsc', compensated=True)        # nbodykit's to_mesh

Random numbers follow the box, as in ``sky.py``: ``rng='numpy'`` draws the reference's legacy global stream on the host in
the reference's order (``np.random.seed(s)`` gives the reference's counts and catalogue); ``rng='device'`` draws Philox
streams 5 (counts) and 6 (catalogue offsets) on the device, reproduced by ``fastbox_amd.rng`` (``stream_poisson``,
``scatter_uniforms``).

Limits: an expected count above 2^24 raises ValueError, so that fp32 counts stay exact; a count drawn above 2^24 -- possible
from an expected count some 15-20 thousand below the limit, sigma being 4096 there -- is stored rounded to fp32, to an even
number, on a single-precision plan.  An
all-zero count field gives an empty (0, 3) catalogue, where the reference raises.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, REAL

LAM_MAX = float(2 ** 24)
WINDOWS = {"ngp": 0, "cic": 1, "tsc": 2}
_SCALAR, _ZPROFILE, _FIELD, _FIELD_F64 = 0, 1, 2, 3


class HaloCatalogue(object):
    """Halo positions (comoving, Mpc) on the device: fp64 [Nh][3].  ``np.asarray(cat)`` is the (Nh, 3) array."""

    def __init__(self, engine, buf, n):
        self.engine, self._buf, self.n = engine, buf, int(n)
        self._host = None

    @property
    def ptr(self):
        return self._buf.ptr if self._buf is not None else None

    def __len__(self):
        return self.n

    @property
    def shape(self):
        return (self.n, 3)

    def host(self):
        if self._host is None:
            h = np.empty((self.n, 3), dtype=np.float64)
            if self.n:
                _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), self.ptr, h.nbytes, self.engine.stream)
            h.setflags(write=False)
            self._host = h
        return self._host

    def __array__(self, dtype=None, copy=None):
        h = self.host()
        return h if dtype is None or np.dtype(dtype) == h.dtype else h.astype(dtype)

    def __repr__(self):
        return "HaloCatalogue(%d halos)" % self.n


class ColaParticles(HaloCatalogue):
    """The particles of CosmoBox.realise_density_cola: positions (Mpc, wrapped to [0, L)) as a HaloCatalogue -- so
    ``paint_catalogue`` takes them -- and ``velocities``, the peculiar velocities a dx/dt in km/s, fp64 (n, 3) on the device
    (``np.asarray(p.velocities)`` is the host copy)."""

    def __init__(self, engine, buf, n, vel_buf):
        HaloCatalogue.__init__(self, engine, buf, n)
        self.velocities = HaloCatalogue(engine, vel_buf, n)

    def __repr__(self):
        return "ColaParticles(%d particles)" % self.n


def _next_realisation(box):
    r = getattr(box, "_halo_draws", 0)
    box._halo_draws = r + 1
    return r


class HaloDistribution(object):

    def __init__(self, box, mass_range, mass_bins):
        """Halos on top of a realisation of a density field in ``box`` (a CosmoBox); mass_range (Msun) and mass_bins are kept
        as the reference keeps them."""
        self.box = box
        self.Mmin, self.Mmax = mass_range
        self.mass_bins = mass_bins
        self.last_realisation = None

    def construct_bins(self, z):
        raise NotImplementedError("construct_bins needs a halo mass function (pyccl), which this port does not have; the "
                                  "reference's version also uses an undefined `cosmo`")

    # ------------------------------------------------------------------ counts
    def _param(self, v, name, keep):
        """(pointer, kind, value) of nbar / bias: a scalar, a length-N profile along z, or an (N, N, N) host / device array."""
        box, eng = self.box, self.box.engine
        N = box.N
        if isinstance(v, DeviceArray):
            if v.engine is not eng or v.kind != REAL:
                raise ValueError("%s: a real field of this box" % name)
            return v.ptr, _FIELD, 0.0
        a = np.asarray(v, dtype=np.float64)
        if a.size == 1 and a.ndim <= 1:
            return None, _SCALAR, float(a.reshape(-1)[0])
        if a.ndim == 1 and a.size == N:
            buf = eng.upload_raw(np.ascontiguousarray(a))
            keep.append(buf)
            return buf.ptr, _ZPROFILE, 0.0
        if a.shape == (N, N, N):
            buf = eng.upload_raw(np.ascontiguousarray(a))
            keep.append(buf)
            return buf.ptr, _FIELD_F64, 0.0
        raise ValueError("%s: a scalar, a length-%d array along z or an array of shape %s" % (name, N, (N, N, N)))

    def _args(self, delta_x, nbar, bias, keep):
        box = self.box
        d = box._as_real(delta_x)
        keep.append(d)
        pn, kn, vn = self._param(nbar, "nbar", keep)
        pb, kb, vb = self._param(bias, "bias", keep)
        voxel_vol = box.Lx * box.Ly * box.Lz / box.N ** 3.
        return d.ptr, pn, kn, vn, pb, kb, vb, voxel_vol

    def expected_counts(self, delta_x, nbar, bias, lognormal=False):
        """Host fp64 (N, N, N): the expected count per voxel, lam, that halo_count_field draws from."""
        eng, N = self.box.engine, self.box.N
        keep = []
        args = self._args(delta_x, nbar, bias, keep)
        buf = eng._alloc_bytes(8 * N ** 3)
        _lib.call("fb_halo_lambda", eng._plan, *args, int(bool(lognormal)), buf.ptr, eng.stream)
        lam = np.empty((N, N, N), dtype=np.float64)
        _lib.call("fb_memcpy_d2h", lam.ctypes.data_as(ctypes.c_void_p), buf.ptr, lam.nbytes, eng.stream)
        return lam

    def halo_count_field(self, delta_x, nbar, bias, lognormal=False, realisation=None):
        """Poisson halo counts per voxel (halos.py:53-117): lam = voxel_vol * nbar * (1 + delta_h), delta_h = bias * delta_x or,
        with ``lognormal``, exp(delta_h) / mean(exp(delta_h)) - 1 (formed with a shift on single-precision plans); negative lam
        is set to 0 unless log-normal, NaN to 0.  ``nbar``, ``bias``: scalar, length-N array along z (the last axis), or an
        (N, N, N) host array / DeviceArray.  Returns a real DeviceArray of integer counts.  ValueError if any lam > 2^24.
        ``realisation`` (rng='device'): the counter of the draw (default: the box's next one; kept in last_realisation)."""
        box, eng, N = self.box, self.box.engine, self.box.N
        if box.rng == "numpy":
            lam = self.expected_counts(delta_x, nbar, bias, lognormal)
            if np.max(lam) > LAM_MAX:
                raise ValueError("expected halo count above 2^24 in a voxel: counts would not be exact in fp32")
            counts = np.random.poisson(lam=lam)
            return eng.upload(counts.astype(eng.rdtype), REAL)
        keep = []
        args = self._args(delta_x, nbar, bias, keep)
        real = _next_realisation(box) if realisation is None else int(realisation)
        self.last_realisation = real
        out = eng.empty(REAL)
        over = ctypes.c_int32(0)
        _lib.call("fb_halo_counts", eng._plan, *args, int(bool(lognormal)), box.seed & (2 ** 64 - 1), real, out.ptr,
                  ctypes.byref(over), eng.stream)
        if over.value:
            raise ValueError("expected halo count above 2^24 in a voxel: counts would not be exact in fp32")
        return out

    # ------------------------------------------------------------------ catalogue
    def realise_halo_catalogue(self, Nhalo, scatter=False, scatter_type='uniform', realisation=None):
        """Halo positions (halos.py:120-176) in the reference's order: ascending count; within a count, voxels in C order,
        each repeated `count` times; pos = (index + u) * (L_a / N).  ``scatter``: u uniform on [0, 1 - 1e-8) (rng='numpy':
        np.random.uniform(0., 1.-1e-8, 3 Nh) row-major; rng='device': stream 6), else 0.  ``Nhalo``: the device counts or a
        host integer array.  Returns a HaloCatalogue (empty, shape (0, 3), for an all-zero field)."""
        box, eng, N = self.box, self.box.engine, self.box.N
        if scatter and scatter_type != 'uniform':
            raise ValueError("scatter_type='%s' not recognised" % scatter_type)
        if isinstance(Nhalo, DeviceArray):
            if Nhalo.engine is not eng or Nhalo.kind != REAL:
                raise ValueError("Nhalo: a real field of this box")
            counts = Nhalo
        else:
            a = np.asarray(Nhalo)
            if a.shape != (N, N, N):
                raise ValueError("Nhalo: expected an array of shape %s, got %s" % ((N, N, N), a.shape))
            if a.size and (np.min(a) < 0 or np.any(a != np.floor(a)) or np.max(a) > LAM_MAX):
                raise ValueError("Nhalo: non-negative integers up to 2^24")
            counts = eng.upload(a.astype(eng.rdtype), REAL)
        kt = (ctypes.c_int64 * 2)()
        _lib.call("fb_halo_catalogue_size", eng._plan, counts.ptr, kt, eng.stream)
        kmax, total = int(kt[0]), int(kt[1])
        if total == 0:
            return HaloCatalogue(eng, None, 0)
        buf = eng._alloc_bytes(24 * total)
        mode, upos, seed, real = 0, None, 0, 0
        keep = None
        if scatter:
            if box.rng == "numpy":
                u = np.random.uniform(0., 1. - 1e-8, 3 * total)
                keep = eng.upload_raw(u)
                mode, upos = 1, keep.ptr
            else:
                mode, seed = 2, box.seed & (2 ** 64 - 1)
                real = _next_realisation(box) if realisation is None else int(realisation)
                self.last_realisation = real
        _lib.call("fb_halo_catalogue", eng._plan, counts.ptr, kmax, total, upos, mode, seed, real, buf.ptr, eng.stream)
        if keep is not None:
            eng.sync()              # the host array behind the upload must outlive the copy
        return HaloCatalogue(eng, buf, total)


def paint(box, positions, weights=None, window='cic', compensated=False):
    """CosmoBox.paint_catalogue: see there."""
    eng, N = box.engine, box.N
    if window not in WINDOWS:
        raise ValueError("window must be one of %s" % sorted(WINDOWS))
    keep = []
    if isinstance(positions, HaloCatalogue):
        if positions.engine is not eng:
            raise ValueError("positions: a catalogue of this box")
        n, pptr = positions.n, positions.ptr
    else:
        p = np.ascontiguousarray(positions, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("positions: an (n, 3) array")
        n = p.shape[0]
        buf = eng.upload_raw(p) if n else None
        keep.append(buf)
        pptr = buf.ptr if n else None
    wptr = None
    if weights is not None:
        if hasattr(weights, "data_ptr"):          # a device tensor: fp64, contiguous, n values
            if str(getattr(weights, "dtype", "")) != "torch.float64" or not weights.is_contiguous() \
                    or weights.numel() != n or not weights.is_cuda:
                raise ValueError("weights: a contiguous float64 device tensor of %d values" % n)
            wptr = weights.data_ptr() if n else None
        else:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if w.size != n:
                raise ValueError("weights: expected %d values, got %d" % (n, w.size))
            if n:
                wb = eng.upload_raw(w)
                keep.append(wb)
                wptr = wb.ptr
    out = eng.empty(REAL)
    _lib.call("fb_paint", eng._plan, pptr, wptr, int(n), WINDOWS[window], out.ptr, eng.stream)
    if compensated:
        work = eng.empty("half")
        _lib.call("fb_paint_compensate", eng._plan, out.ptr, work.ptr, WINDOWS[window], eng.stream)
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    return out
