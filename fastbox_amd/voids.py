"""
Void finding on the device: the counterpart of the reference's fastbox/voids.py (and examples/example_void_detection.py).

    from fastbox_amd.voids import watershed, apply_watershed, region_statistics, trim_by_volume, stack_voids
    labels = watershed(delta_s, markers=None)                  # VoidLabels: int32 labels on the device, 0 outside the mask
    voids = apply_watershed(delta, mask_threshold=0., merge_threshold=0.2)
    st = region_statistics(labels, delta)                      # per-label numpy arrays: count, mean, arg-min, sums
    cat = trim_by_volume(voids, 10, 10**5)
    stacked, failures = stack_voids(cat, voids, box, delta)

Definitions (restated in numpy by tests/voids_numpy.py): steepest descent on the strict order (f, i) over
the 6 face neighbours of a box that is not periodic; labels 1..n numbered by the raster order of the minima; merging by the
connected components of the adjacency of regions whose means differ by less than the threshold; stacking by trilinear
interpolation inside each void.  Agreement with skimage's watershed / rag_mean_color / cut_threshold and with scipy's griddata
is intended, not verified.  Only ``markers=None``.  One box on one GPU (a CosmoBox, not a SlabBox).
"""
import ctypes
import time

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, REAL

MASK_ALL, MASK_THRESHOLD, MASK_U8, MASK_FIELD = 0, 1, 2, 3        # FB_VOID_MASK_*
NCOL = 11                                                           # columns of fb_region_stats
KINDS = ("uniform", "minimum", "density")
MAX_LABEL = 2 ** 30
MAX_WATERSHED_N = 1290                                              # N^3 < 2^31: bit 31 of a parent word marks a root


class VoidLabels(DeviceBuffer):
    """Region labels on the device: int32 [N][N][N] in C order, 0 = outside the mask, 1..n_labels.  ``np.asarray(labels)`` is
    the (N, N, N) int32 host copy."""

    def __init__(self, engine, buf, n_labels):
        DeviceBuffer.__init__(self, engine, buf, (engine.N,) * 3, np.int32)
        self.n_labels = int(n_labels)

    def __repr__(self):
        return "VoidLabels(%d regions, N=%d)" % (self.n_labels, self.engine.N)


class RegionStats(object):
    """Per-label statistics, index = label (0 included), from one fb_region_stats call: ``count``; ``argmin`` (flat voxel index of
    the least (f, i), -1 where there is none); ``index_sum`` (n, 3); ``sum`` and ``mean`` of f; ``weight_sum`` (w = max(-f, 0))
    and ``weighted_index_sum`` (n, 3).  Without a field only count and index_sum are meaningful."""

    def __init__(self, labels, raw, dev):
        n1 = labels.n_labels + 1
        self.labels, self.n_labels, self._dev = labels, labels.n_labels, dev
        ints = raw[:5 * n1].view(np.int64).reshape(5, n1)
        dbl = raw[5 * n1:].reshape(6, n1)
        self.count, self.argmin = ints[0], ints[1]
        self.index_sum = ints[2:5].T.copy()
        self.sum, self.weight_sum = dbl[0], dbl[1]
        self.weighted_index_sum = dbl[2:5].T.copy()
        self.mean = dbl[5]

    @property
    def means_ptr(self):
        """device double[n_labels + 1]: the mean column (what fb_merge_regions reads)"""
        return self._dev.ptr + 10 * (self.n_labels + 1) * 8

    def centroids(self, box, kind="uniform"):
        """(n_labels + 1, 3) box coordinates per label: 'uniform' the mean of box.x[ix] etc. (x0 + dx mean(ix)), 'density'
        x0 + dx sum(w ix) / sum(w) (NaN where sum(w) = 0), 'minimum' the coordinates of the arg-min (NaN where there is none)."""
        if kind not in KINDS:
            raise ValueError("Centroid kind '%s' not recognised." % kind)
        x0, dx = _axes(box)
        with np.errstate(invalid="ignore", divide="ignore"):
            if kind == "uniform":
                return x0 + dx * (self.index_sum / self.count[:, None])
            if kind == "density":
                return x0 + dx * (self.weighted_index_sum / self.weight_sum[:, None])
        N = box.N
        a = self.argmin
        out = np.full((a.size, 3), np.nan)
        ok = a >= 0
        ix, iy, iz = np.unravel_index(a[ok], (N, N, N))
        out[ok] = np.column_stack([box.x[ix], box.y[iy], box.z[iz]])
        return out

    def radii(self, box):
        """(3 dV n / 4 pi)^(1/3) per label, dV = dx dy dz from box.x / y / z (voids.py:102-112)."""
        dV = (box.x[1] - box.x[0]) * (box.y[1] - box.y[0]) * (box.z[1] - box.z[0])
        return (3. * dV * self.count / (4. * np.pi)) ** (1. / 3.)


def _axes(box):
    x0 = np.array([box.x[0], box.y[0], box.z[0]])
    return x0, np.array([box.x[1], box.y[1], box.z[1]]) - x0


def _check_markers(markers):
    if markers is not None:
        raise NotImplementedError("markers: only markers=None (one region per local minimum) is supported; seeded flooding "
                                  "from given markers is not a steepest-descent problem")


def _engine(field, box, name):
    if isinstance(field, DeviceArray):
        if box is not None and field.engine is not box.engine:
            raise ValueError("%s: a field of this box" % name)
        return field.engine
    if box is None:
        raise ValueError("%s: a real DeviceArray of a box, or a host (N, N, N) array together with box=" % name)
    return box.engine


def _real_arg(field, eng, name):
    """Check a field argument without touching the device: a real DeviceArray of eng, or a host (N, N, N) array (its real part)."""
    if isinstance(field, DeviceArray):
        if field.engine is not eng or field.kind != REAL:
            raise ValueError("%s: a real field of this box" % name)
        return field
    a = np.asarray(field)
    if a.shape != (eng.N,) * 3:
        raise ValueError("%s: expected an array of shape %s, got %s" % (name, (eng.N,) * 3, a.shape))
    return a.real if np.iscomplexobj(a) else a


def _real(field, eng):
    """A checked field argument (_real_arg) on the device: the DeviceArray itself, or the host array uploaded in the plan's
    precision."""
    if isinstance(field, DeviceArray):
        field.ptr                              # materialise a deferred field
        return field
    return eng.upload(field, REAL)


def _labels_arg(void_labels, eng):
    """Check a labels argument without touching the device: VoidLabels of eng, or a host integer array (as int32)."""
    if isinstance(void_labels, VoidLabels):
        if eng is not None and void_labels.engine is not eng:
            raise ValueError("void_labels: labels of this box")
        return void_labels
    a = np.asarray(void_labels)
    if a.shape != (eng.N,) * 3:
        raise ValueError("void_labels: expected an array of shape %s, got %s" % ((eng.N,) * 3, a.shape))
    if not np.issubdtype(a.dtype, np.integer) and not np.all(a == np.floor(a)):
        raise ValueError("void_labels: integer labels")
    lo, hi = (int(np.min(a)), int(np.max(a))) if a.size else (0, 0)
    if lo < 0 or hi >= MAX_LABEL:
        raise ValueError("void_labels: labels in 0 .. 2^30 - 1")
    return np.ascontiguousarray(a, dtype=np.int32)


def _n_labels(lab):
    return lab.n_labels if isinstance(lab, VoidLabels) else int(lab.max()) if lab.size else 0


def _labels(lab, eng):
    """A checked labels argument (_labels_arg) on the device: VoidLabels (n_labels = the largest value of a host array)."""
    if isinstance(lab, VoidLabels):
        return lab
    return VoidLabels(eng, eng.upload_raw(lab), _n_labels(lab))


def _cat(void_cat, n_labels):
    c = np.asarray(void_cat).reshape(-1)
    if c.size and not np.all(c == np.floor(c)):
        raise ValueError("void_cat: integer labels")
    ci = c.astype(np.int64)
    if ci.size and (ci.min() < 0 or ci.max() > n_labels):
        raise ValueError("void_cat: labels in 0 .. %d" % n_labels)
    return c, ci


def _watershed(eng, f, kind, thr, mask_ptr):
    if eng.N ** 3 >= 2 ** 31:
        raise ValueError("watershed: N^3 must be below 2^31 (N <= %d), got N = %d: a parent word holds a voxel index in 31 bits"
                         % (MAX_WATERSHED_N, eng.N))
    buf = eng._alloc_bytes(4 * eng.N ** 3)
    n = ctypes.c_int64(0)
    _lib.call("fb_watershed", eng._plan, f.ptr, kind, float(thr), mask_ptr, buf.ptr, ctypes.byref(n), eng.stream)
    return VoidLabels(eng, buf, n.value)


def watershed(field, markers=None, mask=None, box=None):
    """skimage.segmentation.watershed(field, markers=None, mask=mask) as the example calls it: steepest descent on (f, i), one
    region per local minimum, labels 1..n in the raster order of the minima, 0 outside the mask.  ``field``: a real DeviceArray
    of a box, or a host (N, N, N) array with ``box=`` (uploaded in the box's precision).  ``mask``: None (every finite voxel),
    a host boolean array or a real DeviceArray (nonzero = inside); non-finite voxels are always outside.  N^3 < 2^31, i.e.
    N <= 1290 (a parent word holds a voxel index in 31 bits, bit 31 marks a root): ValueError beyond.  Returns VoidLabels."""
    _check_markers(markers)
    eng = _engine(field, box, "field")
    N = eng.N
    f = _real_arg(field, eng, "field")
    kind, mptr, keep = MASK_ALL, None, None
    if isinstance(mask, DeviceArray):
        if mask.engine is not eng or mask.kind != REAL:
            raise ValueError("mask: a real field of this box")
        kind, mptr, keep = MASK_FIELD, mask.ptr, mask
    elif mask is not None:
        m = np.asarray(mask)
        if m.shape != (N, N, N):
            raise ValueError("mask: expected an array of shape %s, got %s" % ((N, N, N), m.shape))
        keep = eng.upload_raw(np.ascontiguousarray(m != 0, dtype=np.uint8))
        kind, mptr = MASK_U8, keep.ptr
    f = _real(f, eng)
    out = _watershed(eng, f, kind, 0.0, mptr)
    del keep
    return out


def region_statistics(labels, field=None, box=None):
    """Per-label statistics of ``field`` (see RegionStats) over ``labels`` (VoidLabels, or a host int array with ``box=`` or a
    DeviceArray field giving the box).  Sums in fp64, fixed point: the same bit for bit from call to call.  ValueError if the
    field is not finite in a voxel of label >= 1."""
    if isinstance(labels, VoidLabels):
        eng = labels.engine
    elif isinstance(field, DeviceArray):
        eng = field.engine
    elif box is not None:
        eng = box.engine
    else:
        raise ValueError("labels: VoidLabels, or a host array together with box=")
    lab = _labels_arg(labels, eng)
    f = _real_arg(field, eng, "field") if field is not None else None
    lab = _labels(lab, eng)
    f = _real(f, eng) if f is not None else None
    n1 = lab.n_labels + 1
    dev = eng._alloc_bytes(NCOL * n1 * 8)
    bad = ctypes.c_int32(0)
    _lib.call("fb_region_stats", eng._plan, lab.ptr, lab.n_labels, f.ptr if f is not None else None, dev.ptr, ctypes.byref(bad),
              eng.stream)
    if bad.value & 2:
        raise ValueError("void_labels: labels outside 0 .. %d" % lab.n_labels)
    if bad.value & 1:
        raise ValueError("field: not finite in a voxel of a region (label >= 1)")
    return RegionStats(lab, eng.download_raw(dev, NCOL * n1), dev)


def merge_regions(labels, field, merge_threshold, box=None):
    """Merged labels: the connected components of the adjacency of regions >= 1 whose means of ``field`` differ by less than
    ``merge_threshold``, numbered 1..M by their least label; 0 stays 0 (the intent of rag_mean_color + cut_threshold)."""
    st = labels if isinstance(labels, RegionStats) else region_statistics(labels, field, box)
    lab = st.labels
    eng = lab.engine
    buf = eng._alloc_bytes(4 * eng.N ** 3)
    m = ctypes.c_int64(0)
    _lib.call("fb_merge_regions", eng._plan, lab.ptr, lab.n_labels, st.means_ptr, float(merge_threshold), buf.ptr,
              ctypes.byref(m), eng.stream)
    return VoidLabels(eng, buf, m.value)


def apply_watershed(field, markers=None, mask_threshold=0., merge_threshold=0.2, verbose=True, box=None):
    """Voids of ``field`` (voids.py:139-203): the watershed inside the mask f <= mask_threshold (in fp64), then the merging of
    adjacent regions whose means differ by less than merge_threshold.  The field is used as given: the reference divides by the
    mean only when the mean is exactly 0 (an inverted test), so every field with a non-zero mean reaches it unchanged there too.
    Returns VoidLabels."""
    _check_markers(markers)
    eng = _engine(field, box, "field")
    thr, mth = float(mask_threshold), float(merge_threshold)
    f = _real(_real_arg(field, eng, "field"), eng)
    if verbose:
        print("Running watershed algorithm")
    t0 = time.time()
    lab = _watershed(eng, f, MASK_THRESHOLD, thr, None)
    st = region_statistics(lab, f)
    masked = 1 if st.count[0] > 0 else 0
    if verbose:
        print("Watershed took %2.2f sec" % (time.time() - t0))
        print("No. regions:", lab.n_labels + masked)
    t0 = time.time()
    if verbose:
        print("Running merging algorithm")
    out = merge_regions(st, None, mth)
    if verbose:
        print("Merging took %2.2f sec" % (time.time() - t0))
        print("No. regions after merging:", out.n_labels + masked)
    return out


# ---- catalogue functions (voids.py:10-136): array forms, and the reference's dict forms on top of them ----------------------
def void_centroids(void_cat, void_labels, box, field=None, kind='uniform'):
    """(len(void_cat), 3) centroids (see RegionStats.centroids); 'minimum' and 'density' need ``field``."""
    if kind not in KINDS:
        raise ValueError("Centroid kind '%s' not recognised." % kind)
    if kind != "uniform" and field is None:
        raise ValueError("field: needed by kind='%s'" % kind)
    lab = _labels_arg(void_labels, box.engine)
    _, ci = _cat(void_cat, _n_labels(lab))
    f = _real_arg(field, box.engine, "field") if kind != "uniform" else None
    st = region_statistics(_labels(lab, box.engine), f)
    return st.centroids(box, kind)[ci]


def void_centroid(void_cat, void_labels, box, field=None, kind='uniform'):
    """{label: ndarray(3)} (voids.py:10-79)."""
    c, _ = _cat(void_cat, MAX_LABEL)
    return dict(zip(c.tolist(), void_centroids(void_cat, void_labels, box, field, kind)))


def void_radii_array(void_cat, void_labels, box):
    """(len(void_cat),) radii (3 dV n / 4 pi)^(1/3)."""
    lab = _labels_arg(void_labels, box.engine)
    _, ci = _cat(void_cat, _n_labels(lab))
    return region_statistics(_labels(lab, box.engine)).radii(box)[ci]


def void_radii(void_cat, void_labels, box):
    """{label: radius} (voids.py:82-113)."""
    c, _ = _cat(void_cat, MAX_LABEL)
    return dict(zip(c.tolist(), void_radii_array(void_cat, void_labels, box)))


def trim_by_volume(void_labels, nmin, nmax):
    """The labels with nmin <= voxel count <= nmax, label 0 included when it is present and qualifies (voids.py:116-136).
    VoidLabels: the counts come from one device call and the result is int32 (the labels' own type).  A host label array is
    counted on the host with np.unique, as the reference does, and the result keeps the array's dtype."""
    if isinstance(void_labels, VoidLabels):
        count = region_statistics(void_labels).count
        lbl = np.arange(count.size)
        return lbl[(count > 0) & (count >= nmin) & (count <= nmax)].astype(np.int32)
    unique, counts = np.unique(np.asarray(void_labels), return_counts=True)
    return unique[np.logical_and(counts >= nmin, counts <= nmax)]


def stack_voids_at(void_cat, void_labels, box, field, centres, radii, grid_scale=1., grid_pix=31):
    """stack_voids with given centres ((n, 3)) and radii ((n,)): returns (np.ma array (grid_pix,)*3, failures, counts)."""
    grid_pix = int(grid_pix)
    if not 1 <= grid_pix <= 1024:
        raise ValueError("grid_pix: 1 .. 1024")
    eng = box.engine
    lab = _labels_arg(void_labels, eng)
    c, ci = _cat(void_cat, _n_labels(lab))
    f = _real_arg(field, eng, "field")
    nv = ci.size
    cen, rad = np.asarray(centres, dtype=np.float64), np.asarray(radii, dtype=np.float64)
    if cen.size != 3 * nv or rad.size != nv:
        raise ValueError("centres, radii: (%d, 3) and (%d,) values for the %d voids" % (nv, nv, nv))
    geom = np.ascontiguousarray(np.column_stack([cen.reshape(nv, 3), rad.reshape(nv)]))
    lab, f = _labels(lab, eng), _real(f, eng)
    grid = np.linspace(-grid_scale, grid_scale, grid_pix)
    P = grid_pix ** 3
    x0, dx = _axes(box)
    axes = (ctypes.c_double * 6)(x0[0], dx[0], x0[1], dx[1], x0[2], dx[2])
    gbuf = eng.upload_raw(grid)
    vbuf = eng.upload_raw(ci.astype(np.int32)) if nv else None
    cbuf = eng.upload_raw(geom) if nv else None
    mean_d, cnt_d, hit_d = eng._alloc_bytes(8 * P), eng._alloc_bytes(8 * P), eng._alloc_bytes(4 * max(nv, 1))
    _lib.call("fb_stack_voids", eng._plan, lab.ptr, f.ptr, vbuf.ptr if nv else None, cbuf.ptr if nv else None, nv, axes,
              gbuf.ptr, grid_pix, mean_d.ptr, cnt_d.ptr, hit_d.ptr, eng.stream)
    mean, cnt = eng.download_raw(mean_d, P), eng.download_raw(cnt_d, P, np.int64)
    hit = eng.download_raw(hit_d, max(nv, 1), np.int32)
    shape = (grid_pix,) * 3
    stacked = np.ma.array(mean.reshape(shape), mask=(cnt == 0).reshape(shape))
    failures = [x for x, h in zip(c.tolist(), hit[:nv]) if not h]
    return stacked, failures, cnt.reshape(shape)


def stack_voids(void_cat, void_labels, box, field, centroid_kind=None, grid_scale=1., grid_pix=31):
    """Mean of ``field`` over the voids, each centred on its centroid and scaled by its radius (voids.py:206-301): grid =
    linspace(-grid_scale, grid_scale, grid_pix), gx, gy, gz = meshgrid(grid, grid, grid); the point of void v is c_v + R_v (gx,
    gy, gz), its value the trilinear interpolation of ``field`` when the 8 surrounding voxels lie in the box and carry the void's
    label (scipy's griddata over the void's voxels in the reference).  ``centroid_kind``: None is 'uniform' (the reference
    ignores the argument and uses 'uniform').  Returns (np.ma array, masked where no void is valid; list of the voids with no
    valid point)."""
    kind = "uniform" if centroid_kind is None else centroid_kind
    if kind not in KINDS:
        raise ValueError("Centroid kind '%s' not recognised." % kind)
    if not 1 <= int(grid_pix) <= 1024:
        raise ValueError("grid_pix: 1 .. 1024")
    lab = _labels_arg(void_labels, box.engine)
    _, ci = _cat(void_cat, _n_labels(lab))
    f = _real(_real_arg(field, box.engine, "field"), box.engine)
    lab = _labels(lab, box.engine)
    st = region_statistics(lab, f if kind != "uniform" else None)
    stacked, failures, _ = stack_voids_at(void_cat, lab, box, f, st.centroids(box, kind)[ci], st.radii(box)[ci],
                                          grid_scale, grid_pix)
    return stacked, failures
