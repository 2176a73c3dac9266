"""The numpy statement of the Minkowski-functional counts (kernel: fastbox_amd/csrc/fb_minkowski.hip), for
any N.  A voxel is a closed cell of the periodic lattice; an element of the cell complex -- cell, face, edge, vertex -- lies in
the excursion set of threshold t iff the maximum of its adjacent voxels is >= t.  The maxima are formed with np.maximum and
np.roll, one array per kind and orientation of element, and counted against all thresholds by a sort and np.searchsorted.  A NaN
is below every threshold (mapped to -inf) and counted in n_nan.  Every count is an int64."""
import numpy as np


def stored(field, dtype):
    """The field as a plan of that precision holds it, promoted back to fp64 exactly."""
    return np.asarray(field).astype(dtype).astype(np.float64)


def _at_least(values, thresholds):
    """#{values >= t} for every t"""
    s = np.sort(values, axis=None)
    return (s.size - np.searchsorted(s, thresholds, side="left")).astype(np.int64)


def _clean(field):
    f = np.array(field, dtype=np.float64)
    nan = np.isnan(f)
    f[nan] = -np.inf
    return f, nan


def _up(f, *axes):
    """max over the 2^len(axes) voxels at offsets 0 / +1 along the given axes, periodic"""
    for a in axes:
        f = np.maximum(f, np.roll(f, -1, axis=a))
    return f


def counts_3d(field, thresholds):
    """dict n3 (nt,), n2 (3, nt) faces by normal, n1 (3, nt) edges by the axis they run along, n0 (nt,), n_nan"""
    f, nan = _clean(field)
    t = np.asarray(thresholds, dtype=np.float64)
    others = ((1, 2), (0, 2), (0, 1))
    return dict(n3=_at_least(f, t),
                n2=np.array([_at_least(_up(f, d), t) for d in range(3)]),
                n1=np.array([_at_least(_up(f, *others[d]), t) for d in range(3)]),
                n0=_at_least(_up(f, 0, 1, 2), t),
                n_nan=int(nan.sum()))


def counts_2d_map(m, thresholds):
    """One periodic 2-D map: dict n2 (nt,) pixels, n1 (2, nt) edges by the axis they run along (their 2 pixels differ in the
    other axis), n0 (nt,) vertices, n_nan"""
    f, nan = _clean(m)
    t = np.asarray(thresholds, dtype=np.float64)
    return dict(n2=_at_least(f, t), n1=np.array([_at_least(_up(f, 1), t), _at_least(_up(f, 0), t)]),
                n0=_at_least(_up(f, 0, 1), t), n_nan=int(nan.sum()))


def counts_per_channel(cube, thresholds):
    """Every z-slice of the cube as a 2-D map: dict n2 (N, nt), n1 (2, N, nt), n0 (N, nt), n_nan (N,); thresholds (nt,), or
    (N, nt) with a row per channel"""
    cube = np.asarray(cube)
    N = cube.shape[2]
    t = np.asarray(thresholds, dtype=np.float64)
    per = [counts_2d_map(cube[:, :, c], t if t.ndim == 1 else t[c]) for c in range(N)]
    return dict(n2=np.array([p["n2"] for p in per]), n1=np.array([p["n1"] for p in per]).transpose(1, 0, 2),
                n0=np.array([p["n0"] for p in per]), n_nan=np.array([p["n_nan"] for p in per], dtype=np.int64))


def euler_3d(c):
    return c["n0"] - c["n1"].sum(axis=0) + c["n2"].sum(axis=0) - c["n3"]


def euler_2d(c):
    return c["n0"] - c["n1"].sum(axis=0) + c["n2"]
