"""
Cosmic-web classification on the device: the tidal tensor of a density (T-web; Hahn et al. 2007, Forero-Romero et al. 2009),
the shear tensor of a velocity (V-web; Hoffman et al. 2012), their eigenvalues per voxel and the classes void, sheet, filament
and knot -- the number of eigenvalues above a threshold -- with volume and mass fractions over a scan of thresholds and class
masks that the other statistics take as fields.  Definition, Nyquist rules and limits: DESIGN.md section 4; numpy statement:
tests/web_numpy.py; kernels: csrc/fb_web.hip.

    cw = box.cosmic_web(smoothing=4., threshold=0.2)                     # CosmicWeb of box.delta_x
    cw.volume_fraction[0]                                                # void, sheet, filament, knot
    k, pk, modes = box.power_spectrum(cw.mask('filament'))
    T = box.tidal_tensor(smoothing=4.)                                   # TensorField: T.xx ... T.yz, T.trace()
    scan = web.classify(T, threshold=np.linspace(0., 1., 16), weight=1. + box.delta_x)
    scan.mass_fraction                                                   # (16, 4)
    S = web.shear_tensor(box, (vx, vy, vz), smoothing=4.)                # three real cubes, km/s

The pure numpy functions (``web_device_bytes``, ``class_index``) need no GPU.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, FULL, HALF, REAL

NT_MAX = 16                              # FB_WEB_NT_MAX of the library
COMPONENTS = ("xx", "yy", "zz", "xy", "xz", "yz")
CLASS_NAMES = ("void", "sheet", "filament", "knot")
NAN_CLASS = 255
KINDS = ("tidal", "shear")

_P_void = ctypes.POINTER(ctypes.c_void_p)
_P_u64 = ctypes.POINTER(ctypes.c_uint64)


# ---------------------------------------------------------------------- host arithmetic
def class_index(kind):
    """0 .. 3 of a class given by number or by name ('void', 'sheet', 'filament', 'knot')."""
    if isinstance(kind, str):
        if kind not in CLASS_NAMES:
            raise ValueError("kind: one of %s, or 0 .. 3" % (CLASS_NAMES,))
        return CLASS_NAMES.index(kind)
    if isinstance(kind, bool) or int(kind) != kind or not 0 <= int(kind) <= 3:
        raise ValueError("kind: one of %s, or 0 .. 3" % (CLASS_NAMES,))
    return int(kind)


def field_bytes(N, precision):
    """(real, half) bytes of one real cube and of one half spectrum as the library stores them: T[N^3] and complex
    [N][N + 1][pitch] with pitch = N/2 + 1 rounded up to 16."""
    if precision not in ("f32", "f64"):
        raise ValueError("precision must be 'f32' or 'f64'")
    N, prec = int(N), 4 if precision == "f32" else 8
    pitch = (N // 2 + 1 + 15) & ~15
    return N ** 3 * prec, N * (N + 1) * pitch * 2 * prec


def web_device_bytes(N, precision="f32", kind="tidal", from_spectrum=False, eigenvalues=False, classes=True, stage=None):
    """Device bytes of the cosmic-web calls beside their inputs.  ``stage='tensor'``: six work spectra, the six component
    cubes and the input spectra formed from real fields (one for 'tidal' unless ``from_spectrum``, three for 'shear');
    ``stage='classify'``: the three eigenvalue cubes and the class cube asked for, and the work buffer; None: the larger of
    the first and the six components plus the second -- what ``CosmoBox.cosmic_web`` holds at its peak (the spectra are idle
    again when the classification starts)."""
    if kind not in KINDS:
        raise ValueError("kind must be 'tidal' or 'shear'")
    if stage not in (None, "tensor", "classify"):
        raise ValueError("stage: None, 'tensor' or 'classify'")
    real, half = field_bytes(N, precision)
    nin = 3 if kind == "shear" else (0 if from_spectrum else 1)
    tensor = (6 + nin) * half + 6 * real
    cls = (3 * real if eigenvalues else 0) + (int(N) ** 3 if classes else 0) + (1 << 20)
    if stage == "tensor":
        return tensor
    if stage == "classify":
        return cls
    return max(tensor, 6 * real + cls)


# ---------------------------------------------------------------------- results
class TensorField(object):
    """A symmetric tensor field of a box on the device: six real DeviceArrays ``xx``, ``yy``, ``zz``, ``xy``, ``xz``, ``yz``
    (``components``, in that order), ``kind`` ('tidal', 'shear' or None for given components) and ``smoothing`` (Mpc)."""

    def __init__(self, engine, components, kind=None, smoothing=0.):
        self.engine, self.components = engine, tuple(components)
        self.kind, self.smoothing = kind, float(smoothing)
        assert len(self.components) == 6
        for name, c in zip(COMPONENTS, self.components):
            setattr(self, name, c)

    def trace(self):
        """xx + yy + zz, a real DeviceArray: for the tidal tensor the smoothed field minus its mean."""
        eng = self.engine
        return eng.axpby(eng.axpby(self.xx, self.yy, 1., 1., 0.), self.zz, 1., 1., 0.)

    def __repr__(self):
        return "TensorField(kind=%s, N = %d, smoothing = %g Mpc)" % (self.kind, self.engine.N, self.smoothing)


class ClassCube(DeviceBuffer):
    """The classes of every voxel on the device, uint8 (N, N, N): 0 void, 1 sheet, 2 filament, 3 knot, 255 where the tensor is
    not finite.  ``host()`` / ``np.asarray`` give the host copy."""

    def __init__(self, engine, buf):
        DeviceBuffer.__init__(self, engine, buf, (engine.N,) * 3, np.uint8)

    def __repr__(self):
        return "ClassCube(shape=%s)" % (self.shape,)


class CosmicWeb(object):
    """The result of ``classify``: ``thresholds`` (nt,), ``counts`` (nt, 4) int64 voxels per class (void, sheet, filament,
    knot) and threshold, ``n_nan`` (voxels whose tensor is not finite: class 255, in no count), ``volume_fraction`` = counts /
    N^3, ``weight_sums`` (nt, 4) fp64 sums of ``weight`` per class (None without a weight) and ``mass_fraction`` = weight_sums
    over their sum per threshold (the mass fractions when the weight is 1 + delta), ``classes`` (a ``ClassCube``; only with a
    scalar threshold, else None), ``eigenvalues`` (three real DeviceArrays lambda_1 >= lambda_2 >= lambda_3, or None)."""

    def __init__(self, engine, thresholds, counts, n_nan, weight_sums, classes, eigenvalues):
        self.engine, self.thresholds, self.counts, self.n_nan = engine, thresholds, counts, int(n_nan)
        self.weight_sums, self.classes, self.eigenvalues = weight_sums, classes, eigenvalues
        self.N = engine.N

    @property
    def volume_fraction(self):
        return self.counts / float(self.N) ** 3

    @property
    def mass_fraction(self):
        if self.weight_sums is None:
            raise ValueError("mass_fraction: classify(..., weight=1 + delta) first")
        return self.weight_sums / np.sum(self.weight_sums, axis=1, keepdims=True)

    def mask(self, kind):
        """A real DeviceArray that is 1 in the voxels of one class ('void', 'sheet', 'filament', 'knot' or 0 .. 3) and 0
        elsewhere: a field for ``power_spectrum``, ``halo_profiles`` or the void stacker."""
        c = class_index(kind)
        if self.classes is None:
            raise ValueError("mask: classes were not kept (a scalar threshold and return_classes=True)")
        self.engine.need_memory(self.engine.nbytes[REAL], "mask: a %d^3 grid takes" % self.N)
        out = self.engine.empty(REAL)
        _lib.call("fb_web_mask", self.engine._plan, self.classes.ptr, c, out.ptr, self.engine.stream)
        return out

    def __repr__(self):
        return "CosmicWeb(N = %d, %d threshold%s)" % (self.N, self.thresholds.size, "" if self.thresholds.size == 1 else "s")


# ---------------------------------------------------------------------- arguments
def _check_smoothing(smoothing):
    R = float(smoothing)
    if not (np.isfinite(R) and R >= 0.):
        raise ValueError("smoothing: a length >= 0 in Mpc")
    return R


def _check_real(eng, a, name):
    """Checks of one real field of this engine, before any upload: a DeviceArray is returned, a host array as float64."""
    N = eng.N
    if isinstance(a, DeviceArray):
        if a.engine is not eng:
            raise ValueError("%s: a field of this box" % name)
        if a.kind != REAL or a._as_complex:
            raise TypeError("%s: a real field, not a complex one or a spectrum" % name)
        return a
    if isinstance(a, (str, bytes)):
        raise TypeError("%s: a real field" % name)
    h = np.asarray(a)
    if np.iscomplexobj(h):
        raise TypeError("%s: a real field, not a complex one" % name)
    if h.shape != (N, N, N):
        raise ValueError("%s: expected an array of shape %s, got %s" % (name, (N, N, N), h.shape))
    return h


def _device(eng, a):
    return a if isinstance(a, DeviceArray) else eng.upload(a, REAL)


def _check_thresholds(threshold):
    """(thresholds (nt,), scalar?)"""
    t = np.array(threshold, dtype=np.float64, order='C')
    scalar = t.ndim == 0
    if scalar:
        t = t.reshape(1)
    if t.ndim != 1 or not 1 <= t.size <= NT_MAX:
        raise ValueError("threshold: a number or between 1 and %d of them, shape (nt,)" % NT_MAX)
    if not np.all(np.isfinite(t)):
        raise ValueError("threshold: thresholds must be finite")
    if np.any(np.diff(t) <= 0.):
        raise ValueError("threshold: thresholds must be strictly ascending")
    return t, scalar


def _ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])


def _components_of(eng, spectra, kind, smoothing):
    """c2r of the six spectra (destroyed; each goes back to the pool as its cube is made)"""
    comps = []
    while spectra:
        comps.append(eng.fft_c2r(spectra.pop(0), destroy=True))
    return TensorField(eng, comps, kind, smoothing)


# ---------------------------------------------------------------------- tensors
def tensor_field(box, components, kind=None, smoothing=0.):
    """A ``TensorField`` from six given real cubes (xx, yy, zz, xy, xz, yz) of ``box``: DeviceArrays or host (N, N, N) arrays."""
    eng = box.engine
    components = list(components)
    if len(components) != 6:
        raise ValueError("components: six real fields (xx, yy, zz, xy, xz, yz)")
    checked = [_check_real(eng, c, "components") for c in components]
    eng.need_memory(sum(eng.nbytes[REAL] for c in checked if not isinstance(c, DeviceArray)),
                    "tensor_field: a %d^3 grid takes" % eng.N)
    out = TensorField(eng, [_device(eng, c) for c in checked], kind, smoothing)
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    return out


def tidal_tensor(box, delta_x=None, delta_k=None, smoothing=0.):
    """The tidal tensor T_ij = d_i d_j of the potential of a density: the inverse transforms of k_i k_j / k^2 exp(-k^2 R^2 / 2)
    delta(k), R = ``smoothing`` (Mpc); a ``TensorField``.  ``delta_x``: a real field of ``box`` (DeviceArray or host array;
    default ``box.delta_x``), or ``delta_k``: its spectrum (a device half or full spectrum, or a host complex array).  The
    trace is the smoothed field minus its mean; zero at k = 0; the off-diagonal components are zero on the Nyquist planes of
    their two axes.  Bad arguments raise before any device work."""
    eng = box.engine
    if delta_x is not None and delta_k is not None:
        raise ValueError("delta_x and delta_k specified; can only specify one")
    R = _check_smoothing(smoothing)
    if delta_k is not None:
        if isinstance(delta_k, DeviceArray):
            if delta_k.engine is not eng:
                raise ValueError("delta_k: a spectrum of this box")
            if delta_k.kind == REAL:
                raise TypeError("delta_k: a spectrum, not a real field")
        elif np.shape(delta_k) != (eng.N,) * 3:
            raise ValueError("delta_k: expected an array of shape %s, got %s" % ((eng.N,) * 3, np.shape(delta_k)))
        src = None
    else:
        if delta_x is None:
            delta_x = getattr(box, "delta_x", None)
            if delta_x is None:
                raise ValueError("no delta_x: realise_density() first, or pass delta_x or delta_k")
        src = _check_real(eng, delta_x, "delta_x")
    eng.need_memory(web_device_bytes(eng.N, eng.precision, "tidal", stage="tensor")
                    + (eng.nbytes[FULL] if delta_k is not None and not isinstance(delta_k, DeviceArray) else 0),
                    "tidal_tensor: a %d^3 grid takes" % eng.N)
    if src is not None:
        half = eng.fft_r2c(_device(eng, src))
    else:
        half = delta_k if isinstance(delta_k, DeviceArray) else eng.upload(np.asarray(delta_k), FULL)
        if half.kind == FULL:
            half = eng.crop_full(half)
    spectra = [eng.empty(HALF) for _ in range(6)]
    _lib.call("fb_tidal_k", eng._plan, half.ptr, _ptrs(spectra), R, eng.stream)
    out = _components_of(eng, spectra, "tidal", R)
    eng.sync()
    return out


def shear_tensor(box, velocity, smoothing=0., H0=None):
    """The velocity-shear tensor Sigma_ij = -(d_i v_j + d_j v_i) / (2 H0): the inverse transforms of -(i / 2 H0) (k_i v_j(k) +
    k_j v_i(k)) exp(-k^2 R^2 / 2); a ``TensorField``.  ``velocity``: three real cubes (v_x, v_y, v_z) of ``box`` in km/s,
    DeviceArrays or host arrays -- ``cola_grid_velocity``'s, or ``box.to_real`` of ``realise_velocity``'s; ``H0`` in km/s/Mpc
    (default 100 h).  For the linear velocity of ``realise_velocity`` this is (f H a / H0) times the tidal tensor, away from
    the Nyquist planes.  Bad arguments raise before any device work."""
    eng = box.engine
    R = _check_smoothing(smoothing)
    H0 = 100. * float(box.cosmo['h']) if H0 is None else float(H0)
    if not (np.isfinite(H0) and H0 > 0.):
        raise ValueError("H0: a positive number (km/s/Mpc)")
    try:
        vel = list(velocity)
    except TypeError:
        raise TypeError("velocity: three real fields (v_x, v_y, v_z)")
    if len(vel) != 3:
        raise ValueError("velocity: three real fields (v_x, v_y, v_z)")
    vel = [_check_real(eng, v, "velocity") for v in vel]
    eng.need_memory(web_device_bytes(eng.N, eng.precision, "shear", stage="tensor")
                    + sum(eng.nbytes[REAL] for v in vel if not isinstance(v, DeviceArray)), "shear_tensor: a %d^3 grid takes" % eng.N)
    vk = [eng.fft_r2c(_device(eng, v)) for v in vel]
    spectra = [eng.empty(HALF) for _ in range(6)]
    _lib.call("fb_shear_k", eng._plan, _ptrs(vk), _ptrs(spectra), R, H0, eng.stream)
    out = _components_of(eng, spectra, "shear", R)
    eng.sync()
    return out


# ---------------------------------------------------------------------- eigenvalues and classes
def _tensor(tensor):
    if not isinstance(tensor, TensorField):
        raise TypeError("tensor: a TensorField (tidal_tensor, shear_tensor or tensor_field)")
    return tensor


def _eigen(tensor, thresholds, class_at, weight, want_eig, want_classes, want_counts):
    eng = tensor.engine
    N, nt = eng.N, 0 if thresholds is None else thresholds.size
    eig = [eng.empty(REAL) for _ in range(3)] if want_eig else None
    classes = ClassCube(eng, eng._alloc_bytes(N ** 3)) if want_classes else None
    counts = np.zeros((nt, 4), dtype=np.uint64)
    wsum = np.zeros((nt, 4), dtype=np.float64)
    n_nan = ctypes.c_uint64(0)
    _lib.call("fb_web_eigen", eng._plan, _ptrs(tensor.components),
              thresholds.ctypes.data_as(_lib.P_double) if nt else None, nt, class_at,
              weight.ptr if weight is not None else None, _ptrs(eig) if want_eig else None,
              classes.ptr if want_classes else None, counts.ctypes.data_as(_P_u64) if want_counts else None,
              wsum.ctypes.data_as(_lib.P_double) if weight is not None else None,
              ctypes.byref(n_nan) if want_counts else None, eng.stream)
    return eig, classes, counts.astype(np.int64), (wsum if weight is not None else None), int(n_nan.value)


def eigenvalues(tensor):
    """(lambda_1, lambda_2, lambda_3), real DeviceArrays with lambda_1 >= lambda_2 >= lambda_3 per voxel, of a ``TensorField``:
    cyclic Jacobi in fp64 on both precisions, the error of the order of 2^-53 ||A||_F whatever the spectrum; NaN where a
    component is not finite."""
    tensor = _tensor(tensor)
    eng = tensor.engine
    eng.need_memory(web_device_bytes(eng.N, eng.precision, eigenvalues=True, classes=False, stage="classify"),
                    "eigenvalues: a %d^3 grid takes" % eng.N)
    return tuple(_eigen(tensor, None, -1, None, True, False, False)[0])


def classify(tensor, threshold=0., weight=None, return_classes=True, return_eigenvalues=False):
    """The classes of a ``TensorField``: per voxel the number of eigenvalues > ``threshold`` (0 void, 1 sheet, 2 filament,
    3 knot), decided in fp64; a ``CosmicWeb``.  ``threshold``: a number, or up to 16 strictly ascending ones -- the counts,
    fractions and weight sums of all of them come from the one pass; the class cube is kept for a scalar threshold only.
    ``weight``: a real field of the same box (1 + delta for mass fractions), summed per class in fp64 in a fixed order.  A
    voxel with a component that is not finite is class 255, counted in ``n_nan`` and in no class.  Bad arguments raise
    before any device work."""
    tensor = _tensor(tensor)
    eng = tensor.engine
    t, scalar = _check_thresholds(threshold)
    w = _check_real(eng, weight, "weight") if weight is not None else None
    keep = bool(return_classes) and scalar
    eng.need_memory(web_device_bytes(eng.N, eng.precision, eigenvalues=bool(return_eigenvalues), classes=keep, stage="classify")
                    + (eng.nbytes[REAL] if w is not None and not isinstance(w, DeviceArray) else 0), "classify: a %d^3 grid takes" % eng.N)
    wd = _device(eng, w) if w is not None else None
    eig, classes, counts, wsum, n_nan = _eigen(tensor, t, 0, wd, bool(return_eigenvalues), keep, True)
    return CosmicWeb(eng, t, counts, n_nan, wsum, classes, tuple(eig) if eig is not None else None)


def cosmic_web(box, delta_x=None, smoothing=0., threshold=0., kind='tidal', velocity=None, weight=None, return_classes=True,
               return_eigenvalues=False, H0=None):
    """CosmoBox.cosmic_web: see there."""
    if kind not in KINDS:
        raise ValueError("kind must be 'tidal' (T-web of a density) or 'shear' (V-web of a velocity)")
    _check_thresholds(threshold)
    if weight is not None:
        _check_real(box.engine, weight, "weight")
    if kind == 'shear':
        if velocity is None:
            raise ValueError("velocity: kind='shear' needs three real velocity cubes")
        if delta_x is not None:
            raise ValueError("delta_x: kind='shear' takes velocity only")
        tensor = shear_tensor(box, velocity, smoothing=smoothing, H0=H0)
    else:
        if velocity is not None:
            raise ValueError("velocity: with kind='shear' only")
        if H0 is not None:
            raise ValueError("H0: with kind='shear' only")
        tensor = tidal_tensor(box, delta_x=delta_x, smoothing=smoothing)
    return classify(tensor, threshold=threshold, weight=weight, return_classes=return_classes,
                    return_eigenvalues=return_eigenvalues)
