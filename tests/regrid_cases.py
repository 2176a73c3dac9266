"""Constructed inputs for the regridding and catalogue-histogram kernels (fb_regrid.hip), numpy only.  Regrid cases: non-uniform
coordinates, new points on nodes, on the ends and one ulp outside them, an axis of two nodes, a NaN voxel, a wholly NaN channel,
output rows that are no multiple of a wave, a cube that several workgroups cross, and every point outside.  Histogram cases:
points on interior edges, on the first and the last edge, outside, NaN; neighbouring doubles around an edge that is not exactly
representable; a single particle (numpy's widened range); no particle; a non-cubic grid.  tests/test_regrid_cases_cpu.py holds
the numpy statements (tests/regrid_numpy.py) to scipy and np.histogramdd on these cases and asserts what keeps each from being
vacuous; tests/test_regrid_gpu.py runs them on the device."""
import numpy as np

BOX_N = 16                                   # the box of the cases that return a DeviceArray


def _coords(shape, seed):
    """Strictly ascending, non-uniform: cumulative sums of steps in [0.5, 1.5), from a different origin per axis."""
    rs = np.random.RandomState(seed)
    return [np.cumsum(0.5 + rs.random_sample(n)) + o for n, o in zip(shape, (-3., 10., 400.))]


def _field(shape, seed):
    return np.random.RandomState(seed).normal(size=shape) + 5.


def _span(g, n, lo=-0.04, hi=1.03):
    """n new points from a little before the first node to a little after the last."""
    return g[0] + (g[-1] - g[0]) * np.linspace(lo, hi, n)


def _inside(g, n):
    """n new points strictly between the first and the last node."""
    return _span(g, n, 0.02, 0.97)


def regrid_cases():
    """{name: dict(field, coords_orig, coords_new, box=True where the 'xy' result has the box's shape, outside=True where every
    point is outside)}."""
    shape = (5, 7, 6)
    g = _coords(shape, 1)
    f = _field(shape, 2)
    out = {}
    out["onto the box"] = dict(field=f, coords_orig=g, coords_new=[_span(q, BOX_N) for q in g], box=True)
    # 9 x 4 x 11: z_new leaves 53 lanes of the wave idle, 4 x 9 rows are one more than a multiple of the row lanes; descending y
    out["wave tail"] = dict(field=f, coords_orig=g, coords_new=[_span(g[0], 9), _inside(g[1], 4)[::-1].copy(), _span(g[2], 11)])
    # on every node, and one ulp outside: below the first x, above the last y, either side of z
    below, above = [[np.nextafter(q[0], -np.inf)] for q in g], [[np.nextafter(q[-1], np.inf)] for q in g]
    ends = [np.concatenate([below[0], g[0]]), np.concatenate([g[1], above[1]]), np.concatenate([below[2], g[2], above[2]])]
    out["on nodes"] = dict(field=f, coords_orig=g, coords_new=ends)
    g2 = _coords((2, 3, 2), 3)
    out["two nodes"] = dict(field=_field((2, 3, 2), 4), coords_orig=g2,
                            coords_new=[_inside(g2[0], 6), _inside(g2[1], 5), _span(g2[2], 7)])
    fv = f.copy()
    fv[2, 3, 4] = np.nan
    out["nan voxel"] = dict(field=fv, coords_orig=g, coords_new=[_span(g[0], 9), _inside(g[1], 4), _span(g[2], 11)])
    # channel 0 is NaN throughout: the first of five z cells is lost, the centre is not; z_new holds node 1 itself, where the
    # NaN node has weight 0 only if the point is taken into the cell above it
    fc = f.copy()
    fc[:, :, 0] = np.nan
    fc[1, 1, 3] = np.nan
    zc = np.sort(np.concatenate([_span(g[2], 9, -0.04, 0.97), [g[2][1], g[2][2]]]))
    out["nan channel"] = dict(field=fc, coords_orig=g, coords_new=[_inside(g[0], 9), _inside(g[1], 4), zc])
    # the channel before the last is NaN and z_new ends on the last node: cell nz - 2 with t = 1, so the NaN node has weight 0
    # and the sum is NaN all the same (scipy does not skip zero weights); the other points stay below the lost cells
    fz = f.copy()
    fz[:, :, -2] = np.nan
    zz = np.concatenate([g[2][0] + (g[2][3] - g[2][0]) * np.linspace(0., 1., 10), [g[2][-1]]])
    out["nan of weight zero"] = dict(field=fz, coords_orig=g, coords_new=[_inside(g[0], 9), _inside(g[1], 4), zz], zero_weight=True)
    big = (48, 40, 56)
    gb = _coords(big, 5)
    out["several workgroups"] = dict(field=_field(big, 6), coords_orig=gb, coords_new=[_span(q, 64) for q in gb])
    far = [g[0] + 100., _inside(g[1], 4), _span(g[2], 11)]
    out["all outside"] = dict(field=f, coords_orig=g, coords_new=far, outside=True)
    return out


def filled_max(field):
    """max |v| over the input with its NaNs filled: the scale of the error bounds."""
    from tests import regrid_numpy as rn
    v = rn.fill_nan_channel_mean(field)
    return float(np.nanmax(np.abs(v)))


def grid_cases():
    """{name: dict(pos (n, 3), w or None, limits [three (lo, hi) or None], nbin)}."""
    out = {}
    # edges of np.linspace(0, 1, 5) and np.linspace(-2, 2, 9): interior edges, the first, the last, outside either way, NaN
    e = np.linspace(0., 1., 5)
    vals = np.concatenate([e, [np.nextafter(0., -1.), np.nextafter(1., 2.), -0.25, 1.5, np.nan, 0.1, 0.6]])
    pos = np.array([[a, b, c] for a in vals for b in (0.5, vals[1]) for c in (4 * a - 2. if a == a else 0., 0.)])
    pos = np.concatenate([pos, [[0.5, np.nan, 0.], [0.5, 0.5, np.nan], [0.5, 0.5, 2.], [0.5, 0.5, -2.], [1., 1., 2.], [0., 0., -2.]]])
    out["on edges"] = dict(pos=pos, w=None, limits=[(0., 1.), (0., 1.), (-2., 2.)], nbin=(4, 4, 8))
    # 0.3 beside 0.30000000000000004, and every edge of np.linspace(0.1, 0.7, 7) with the doubles next to it on either side:
    # (p - lo) n / (hi - lo) alone puts some of them into the neighbouring bin
    e = np.linspace(0.1, 0.7, 7)
    near = np.concatenate([[0.3, 0.30000000000000004], np.nextafter(e[1:-1], -1.), e, np.nextafter(e[1:-1], 1.)])
    out["beside an edge"] = dict(pos=np.stack([near, near[::-1], np.full(near.size, 0.2)], axis=1), w=None,
                                 limits=[(0.1, 0.7)] * 3, nbin=(6, 6, 6))
    out["one particle"] = dict(pos=np.array([[1.25, -3., 7.5]]), w=None, limits=[None, None, None], nbin=(3, 2, 4))
    out["no particle"] = dict(pos=np.zeros((0, 3)), w=None, limits=[(0., 1.), (0., 2.), (0., 3.)], nbin=(2, 3, 4))
    rs = np.random.RandomState(11)
    p = rs.random_sample((700, 3)) * [3.3, 5.5, 7.7] - [0.1, 0.2, 0.3]
    out["non-cubic"] = dict(pos=p, w=None, limits=[(0., 3.), (0., 5.), (0., 7.)], nbin=(3, 5, 70))
    out["data range"] = dict(pos=p, w=None, limits=[None, (0., 5.), None], nbin=(4, 5, 6))
    return out


def cloud(n, L, seed=21):
    """n points over [-0.05 L, 1.05 L) per axis, a few of them exactly on cell edges of the N = BOX_N grid and on 0 and L."""
    rs = np.random.RandomState(seed)
    L = np.asarray(L, dtype=np.float64)
    p = (rs.random_sample((n, 3)) * 1.1 - 0.05) * L
    k = rs.randint(0, BOX_N + 1, (n // 10, 3))
    p[:n // 10] = k * (L / BOX_N)
    return p
