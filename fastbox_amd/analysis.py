"""
Small data-analysis helpers on the device (the reference's fastbox/analysis.py).
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, REAL
from .filters import _as_cube
from .halos import HaloCatalogue


def replace_nan_with_channel_mean(field, box=None):
    """Replace every NaN of the cube by the mean of its frequency channel (last axis) over the voxels that are not NaN.
    Other voxels are copied bit for bit; a channel that is NaN throughout stays NaN.  Returns a new REAL DeviceArray."""
    cube = _as_cube(field, box)
    eng = cube.engine
    out = eng.empty(REAL)
    _lib.call("fb_replace_nan_channel_mean", eng._plan, cube.ptr, out.ptr, None, eng.stream)
    return out


def _axis(a, what, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1 or a.size < 1 or (n is not None and a.size != n):
        raise ValueError("%s: a 1-d array%s" % (what, "" if n is None else " of %d values" % n))
    return a


def _result(eng, buf, shape):
    """A buffer of the plan's reals as a REAL DeviceArray where the shape is the box's, else as a host fp64 array."""
    if tuple(shape) == (eng.N,) * 3:
        return DeviceArray(eng, REAL, buf)
    return eng.download_raw(buf, shape, eng.rdtype).astype(np.float64)


def interpolate_onto_grid(field, coords_orig, coords_new, box=None, indexing='xy'):
    """Interpolate a cube given on rectilinear coordinates trilinearly onto another grid, on the device (analysis.py:31-70):
    ``scipy.interpolate.RegularGridInterpolator(coords_orig, filled, method='linear', bounds_error=False, fill_value=nan)``
    at the points of ``np.meshgrid(*coords_new)``, where ``filled`` is ``field`` with every NaN replaced by the mean of its
    channel (last axis) over the voxels that are not NaN.

    ``field``: a host array of any shape (nx, ny, nz) with every axis >= 2, or a real DeviceArray; it is held in the box's
    precision.  ``coords_orig`` = (x, y, z): strictly ascending, possibly non-uniform, one value per node.  ``coords_new`` =
    (x_new, y_new, z_new): any length >= 1, any order.  All coordinate and weight arithmetic is fp64.  ``box`` (or a
    DeviceArray ``field``) names the engine.

    A new point outside the closed range of the original coordinates on any axis gives NaN; a channel that is NaN throughout
    stays NaN and gives NaN wherever one of its two nodes is a corner, weight 0 included (as scipy does).

    The reference builds its points with numpy's default ``'xy'`` meshgrid, so its result has shape (len(y_new), len(x_new),
    len(z_new)) with element [j, i, k] at (x_new[i], y_new[j], z_new[k]) -- axes 0 and 1 of the input come back swapped.
    ``indexing='xy'`` (default) reproduces that; ``indexing='ij'`` returns (len(x_new), len(y_new), len(z_new)).

    Returns a real DeviceArray of the box where the result has the box's shape (N, N, N), else a host fp64 array.
    ValueError before any kernel runs for coordinates that do not fit the cube or are not strictly ascending."""
    if indexing not in ('xy', 'ij'):
        raise ValueError("indexing must be 'xy' or 'ij'")
    if isinstance(field, DeviceArray):
        if field.kind != REAL:
            raise TypeError("expected a real-space cube")
        eng, shape, cube = field.engine, field.shape, field
    else:
        if box is None:
            raise TypeError("a host array needs `box=` (the CosmoBox whose engine holds the cube)")
        eng = box.engine
        f = np.asarray(field)
        if np.iscomplexobj(f):
            f = f.real
        shape, cube = f.shape, None
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("field: a 3-d cube with two nodes or more along every axis, got shape %s" % (shape,))
    if len(coords_orig) != 3 or len(coords_new) != 3:
        raise ValueError("coords_orig and coords_new: three arrays each, in the order (x, y, z)")
    g = [_axis(c, "coords_orig[%d]" % a, shape[a]) for a, c in enumerate(coords_orig)]
    for a in range(3):
        if not np.all(np.diff(g[a]) > 0.):
            raise ValueError("coords_orig[%d] must be strictly ascending" % a)
    p = [_axis(c, "coords_new[%d]" % a) for a, c in enumerate(coords_new)]
    if max(shape) > 2 ** 31 - 1 or max(q.size for q in p) > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 nodes or points along an axis")
    if cube is None:
        cube = eng.upload_raw(np.ascontiguousarray(f, dtype=eng.rdtype))
    tabs = eng.upload_raw(np.concatenate(g + p))
    ptr, off = [], 0
    for q in g + p:
        ptr.append(tabs.ptr + 8 * off)
        off += q.size
    swap = indexing == 'xy'
    oshape = (p[1].size, p[0].size, p[2].size) if swap else (p[0].size, p[1].size, p[2].size)
    out = eng._alloc_bytes(oshape[0] * oshape[1] * oshape[2] * np.dtype(eng.rdtype).itemsize)
    _lib.call("fb_regrid_trilinear", eng._plan, cube.ptr, shape[0], shape[1], shape[2], ptr[0], ptr[1], ptr[2],
              ptr[3], p[0].size, ptr[4], p[1].size, ptr[5], p[2].size, int(swap), out.ptr, eng.stream)
    res = _result(eng, out, oshape)
    eng.sync()                          # the coordinate tables and an uploaded cube must outlive the kernels
    return res


def _limits(lim, what):
    lo, hi = (float(v) for v in lim)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("%s: the range %r is not finite" % (what, (lo, hi)))
    if lo > hi:
        raise ValueError("%s: max must be larger than min" % what)
    if lo == hi:                        # np.histogramdd widens an empty range by a half either way
        lo, hi = lo - 0.5, hi + 0.5
    return lo, hi


def grid_catalogue(x, y=None, z=None, w=None, xlim=None, ylim=None, zlim=None, nx=None, ny=None, nz=None, box=None):
    """Bin a catalogue of 3-d positions onto a regular grid on the device (analysis.py:73-118):
    ``np.histogramdd(np.vstack([x, y, z]).T, bins=(nx, ny, nz), range=[xlim, ylim, zlim], weights=w)``.

    ``x, y, z``: host arrays of equal length, as in the reference; or ``x`` alone an (n, 3) host array or a HaloCatalogue
    (FoFHalos, SOHalos, ColaParticles), whose positions stay on the device.  ``w``: optional host weights.  With ``box=`` a
    missing ``nx, ny, nz`` is N and a missing limit is (0, Lx), (0, Ly), (0, Lz).  Without it the reference's rule holds:
    every n must be given, and a missing limit is the minimum and maximum of the data (a device reduction); data that is not
    finite then raises ValueError, as numpy does.  A range with lo == hi is widened to (lo - 0.5, hi + 0.5), as numpy does.
    ``box`` or a catalogue names the engine.

    The edges are ``np.linspace(lo, hi, n + 1)``, made on the host, so the device compares with the same doubles as numpy:
    bin = searchsorted(edges, p, 'right') - 1, a point equal to the last edge falls into the last bin, and a point outside
    the range or NaN on any axis is dropped.  Sums are fixed-point, as in ``paint_catalogue``: the grid is the same bit for bit
    from call to call and for any order of the particles, and unweighted counts are exact integers -- up to 2^24 per cell on a
    single-precision box (what its storage holds exactly), 2^53 in double precision; at most 2^31 particles per cell.

    Returns ``(grid, (xgrid, ygrid, zgrid))`` with ``xgrid = np.linspace(lo, hi, nx)`` etc., as the reference returns them:
    n points from the first to the last edge -- they are *not* the bin centres (the reference's comment says they are).
    ``grid`` is a real DeviceArray where its shape is the box's (N, N, N), else a host fp64 array.

    Not ``paint_catalogue(window='ngp')``: that one assigns to the nearest *node* m L / N -- cells [(m - 1/2) L / N,
    (m + 1/2) L / N) -- and is periodic; this one fills the cells [i L / N, (i + 1) L / N) of the histogram, is not periodic,
    and drops what lies outside.  MemoryError before any kernel runs if the accumulators do not fit."""
    eng = box.engine if box is not None else None
    keep, pos = [], None
    if isinstance(x, HaloCatalogue):
        if y is not None or z is not None:
            raise ValueError("a catalogue brings all three coordinates: leave y and z out")
        if eng is not None and x.engine is not eng:
            raise ValueError("x: a catalogue of this box")
        eng, n = x.engine, x.n
    else:
        if y is None and z is None:
            pos = np.ascontiguousarray(x, dtype=np.float64)
            if pos.ndim != 2 or pos.shape[1] != 3:
                raise ValueError("x alone: an (n, 3) array")
        elif y is None or z is None:
            raise ValueError("give x, y and z, or x alone as an (n, 3) array or a catalogue")
        else:
            cols = [np.asarray(c, dtype=np.float64).reshape(-1) for c in (x, y, z)]
            if not cols[0].size == cols[1].size == cols[2].size:
                raise ValueError("x, y, z: arrays of equal length")
            pos = np.ascontiguousarray(np.vstack(cols).T)
        if eng is None:
            raise TypeError("host positions need `box=` (the CosmoBox whose engine does the work)")
        n = pos.shape[0]
    if box is not None:
        nx, ny, nz = [box.N if m is None else m for m in (nx, ny, nz)]
        xlim, ylim, zlim = [(0., float(Lb)) if lim is None else lim
                            for lim, Lb in ((xlim, box.Lx), (ylim, box.Ly), (zlim, box.Lz))]
    if nx is None or ny is None or nz is None:
        raise ValueError("nx, ny, and nz must be specified.")
    nbin = [int(m) for m in (nx, ny, nz)]
    if min(nbin) < 1 or max(nbin) > 2 ** 31 - 2:
        raise ValueError("nx, ny, nz: 1 <= n < 2^31 - 1")
    wh = None
    if w is not None:
        wh = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
        if wh.size != n:
            raise ValueError("w: expected %d values, got %d" % (n, wh.size))
    ncell = nbin[0] * nbin[1] * nbin[2]
    item = np.dtype(eng.rdtype).itemsize
    need = ncell * (2 * item + item) + (24 * n if pos is not None else 0) + (8 * n if wh is not None else 0)
    eng.need_memory(need, "grid_catalogue: %d x %d x %d cells and %d particles take" % (tuple(nbin) + (n,)))
    if pos is not None:
        pptr = None
        if n:
            keep.append(eng.upload_raw(pos))
            pptr = keep[-1].ptr
    else:
        pptr = x.ptr if n else None
    lims = [xlim, ylim, zlim]
    if any(lim is None for lim in lims):
        if n == 0:
            raise ValueError("an empty catalogue has no range: give xlim, ylim and zlim")
        lohi = (ctypes.c_double * 6)()
        _lib.call("fb_position_range", eng._plan, pptr, int(n), lohi, eng.stream)
        lims = [(lohi[2 * a], lohi[2 * a + 1]) if lim is None else lim for a, lim in enumerate(lims)]
    lims = [_limits(lim, name) for lim, name in zip(lims, ("xlim", "ylim", "zlim"))]
    edges = [np.linspace(lo, hi, m + 1) for (lo, hi), m in zip(lims, nbin)]
    grids = tuple(np.linspace(lo, hi, m) for (lo, hi), m in zip(lims, nbin))
    etab = eng.upload_raw(np.concatenate(edges))
    eptr = [etab.ptr, etab.ptr + 8 * edges[0].size, etab.ptr + 8 * (edges[0].size + edges[1].size)]
    wptr = None
    if wh is not None and n:
        keep.append(eng.upload_raw(wh))
        wptr = keep[-1].ptr
    out = eng._alloc_bytes(ncell * item)
    _lib.call("fb_grid_catalogue", eng._plan, pptr, wptr, int(n), eptr[0], nbin[0], eptr[1], nbin[1], eptr[2], nbin[2],
              out.ptr, eng.stream)
    grid = _result(eng, out, tuple(nbin))
    eng.sync()                          # the uploads must outlive the kernels
    return grid, grids
