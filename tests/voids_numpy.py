"""numpy statement of the void-finding definitions (fastbox_amd/voids.py): the oracle the tests hold the
device to.  Fields are (N, N, N) arrays of the stored values (fp32 values widened to fp64 compare exactly as fp32 ones do)."""
import numpy as np


def inside(f, mask=None, threshold=None):
    """The voxels that take part: finite, and f <= threshold (fp64) / mask != 0 where given."""
    ins = np.isfinite(f)
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            ins &= np.asarray(f, dtype=np.float64) <= threshold
    if mask is not None:
        ins &= np.asarray(mask) != 0
    return ins


def descend(f, ins):
    """Flat parent of every voxel: the least of itself and its in-mask face neighbours in (f, i) order; -1 outside the mask."""
    N = f.shape[0]
    fl = np.asarray(f).reshape(-1)
    m = ins.reshape(-1)
    idx = np.arange(N ** 3, dtype=np.int64)
    coord = np.unravel_index(idx, (N, N, N))
    bv, bj = fl.copy(), idx.copy()
    for a, step in ((0, N * N), (1, N), (2, 1)):
        for sgn in (-1, 1):
            ok = (coord[a] + sgn >= 0) & (coord[a] + sgn < N)
            j = np.where(ok, idx + sgn * step, 0)
            ok &= m[j]
            v = fl[j]
            better = ok & ((v < bv) | ((v == bv) & (j < bj)))
            bv, bj = np.where(better, v, bv), np.where(better, j, bj)
    return np.where(m, bj, -1)


def roots(parent):
    """Pointer jumping to the fixed point."""
    p = parent.copy()
    ins = p >= 0
    while True:
        q = p.copy()
        q[ins] = p[p[ins]]
        if np.array_equal(q, p):
            return p
        p = q


def watershed(f, ins):
    """(labels int32 (N, N, N), n_regions): label = 1 + the rank of the root among all minima in raster order, 0 outside."""
    N = f.shape[0]
    par = descend(f, ins)
    r = roots(par)
    idx = np.arange(N ** 3)
    minima = par == idx
    rank = np.cumsum(minima)
    lab = np.zeros(N ** 3, dtype=np.int32)
    m = r >= 0
    lab[m] = rank[r[m]]
    return lab.reshape(N, N, N), int(minima.sum())


def region_stats(lab, n_labels, f=None):
    """dict of per-label arrays (index = label, 0 included): count, index_sum (n, 3); with f also sum, weight_sum,
    weighted_index_sum (n, 3), mean, argmin.  Non-finite voxels of label 0 add to count and index_sum only; a non-finite voxel
    of label >= 1 raises ValueError."""
    n1 = n_labels + 1
    N = lab.shape[0]
    l = lab.reshape(-1).astype(np.int64)
    idx = np.arange(N ** 3, dtype=np.int64)
    coord = np.unravel_index(idx, (N, N, N))
    out = dict(count=np.bincount(l, minlength=n1).astype(np.int64),
               index_sum=np.column_stack([np.bincount(l, weights=c, minlength=n1) for c in coord]).astype(np.int64))
    if f is None:
        return out
    fv = np.asarray(f, dtype=np.float64).reshape(-1)
    fin = np.isfinite(fv)
    if np.any(~fin & (l > 0)):
        raise ValueError("field: not finite in a voxel of a region")
    fz = np.where(fin, fv, 0.)
    w = np.maximum(-fz, 0.)
    out["sum"] = np.bincount(l, weights=fz, minlength=n1)
    out["weight_sum"] = np.bincount(l, weights=w, minlength=n1)
    out["weighted_index_sum"] = np.column_stack([np.bincount(l, weights=w * c, minlength=n1) for c in coord])
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mean"] = out["sum"] / out["count"]
    sel = idx[fin]
    o = sel[np.lexsort((sel, fv[sel]))]                 # (f, i) order
    am = np.full(n1, -1, dtype=np.int64)
    u, first = np.unique(l[o], return_index=True)
    am[u] = o[first]
    out["argmin"] = am
    return out


def axes(box):
    x0 = np.array([box.x[0], box.y[0], box.z[0]])
    return x0, np.array([box.x[1], box.y[1], box.z[1]]) - x0


def centroids(st, box, kind):
    """(n_labels + 1, 3): 'uniform' x0 + dx index_sum / count, 'density' x0 + dx weighted_index_sum / weight_sum, 'minimum' the
    box coordinates of the arg-min."""
    x0, dx = axes(box)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "uniform":
            return x0 + dx * (st["index_sum"] / st["count"][:, None])
        if kind == "density":
            return x0 + dx * (st["weighted_index_sum"] / st["weight_sum"][:, None])
    N = len(box.x)
    out = np.full((st["argmin"].size, 3), np.nan)
    ok = st["argmin"] >= 0
    ix, iy, iz = np.unravel_index(st["argmin"][ok], (N, N, N))
    out[ok] = np.column_stack([box.x[ix], box.y[iy], box.z[iz]])
    return out


def radii(st, box):
    dV = (box.x[1] - box.x[0]) * (box.y[1] - box.y[0]) * (box.z[1] - box.z[0])
    return (3. * dV * st["count"] / (4. * np.pi)) ** (1. / 3.)


def trim(st, nmin, nmax):
    c = st["count"]
    return np.nonzero((c > 0) & (c >= nmin) & (c <= nmax))[0]


def adjacent_pairs(lab):
    """(a, b) label pairs of face neighbours with a != b, both >= 1 (with repeats)."""
    A, B = [], []
    for ax in range(3):
        a = np.moveaxis(lab, ax, 0)[:-1].reshape(-1)
        b = np.moveaxis(lab, ax, 0)[1:].reshape(-1)
        k = (a > 0) & (b > 0) & (a != b)
        A.append(a[k])
        B.append(b[k])
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def merge(lab, n_labels, mean, threshold, margin=None):
    """(merged labels, M): connected components of the regions >= 1 joined where |mean_a - mean_b| < threshold, numbered 1..M by
    their least label.  ``margin``: assert that no adjacent pair's |d mean| lies within it of the threshold."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n1 = n_labels + 1
    a, b = adjacent_pairs(lab)
    d = np.abs(mean[a] - mean[b])
    if margin is not None:
        assert not np.any(np.abs(d - threshold) < margin), "an adjacent pair's mean difference lies at the threshold"
    k = d < threshold
    g = coo_matrix((np.ones(int(k.sum())), (a[k], b[k])), shape=(n1, n1)).tocsr()
    _, comp = connected_components(g, directed=False)
    least = np.full(comp.max() + 1, n1, dtype=np.int64)
    np.minimum.at(least, comp[1:], np.arange(1, n1))
    used = np.unique(comp[1:])
    order = used[np.argsort(least[used])]
    newid = np.zeros(comp.max() + 1, dtype=np.int64)
    newid[order] = np.arange(1, order.size + 1)
    out = np.where(lab > 0, newid[comp[lab]], 0).astype(np.int32)
    return out, int(order.size)


def stack(lab, f, cat, centres, radii_, box, grid_scale=1., grid_pix=31):
    """(np.ma mean, failures, counts): point (a, b, c) of void v is c_v + R_v (grid[b], grid[a], grid[c]); u = (p - x0) / dx; valid
    when the 8 voxels floor(u) + {0, 1}^3 lie in the box, carry the label, and the trilinear value is finite."""
    N = lab.shape[0]
    fl = np.asarray(f, dtype=np.float64)
    grid = np.linspace(-grid_scale, grid_scale, grid_pix)
    gx, gy, gz = np.meshgrid(grid, grid, grid)
    x0, dx = axes(box)
    tot = np.zeros(gx.shape)
    cnt = np.zeros(gx.shape, dtype=np.int64)
    failures = []
    for v, L in enumerate(cat):
        c, R = centres[v], radii_[v]
        with np.errstate(invalid="ignore"):
            u = [((c[0] + R * gx) - x0[0]) / dx[0], ((c[1] + R * gy) - x0[1]) / dx[1], ((c[2] + R * gz) - x0[2]) / dx[2]]
            fu = [np.floor(x) for x in u]
            ok = np.ones(gx.shape, dtype=bool)
            for x in fu:
                ok &= (x >= 0) & (x <= N - 2)
        i0 = [np.where(ok, x, 0).astype(np.int64) for x in fu]
        w = {}
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    ok &= lab[i0[0] + d0, i0[1] + d1, i0[2] + d2] == L
                    w[4 * d0 + 2 * d1 + d2] = fl[i0[0] + d0, i0[1] + d1, i0[2] + d2]
        with np.errstate(invalid="ignore"):
            tx, ty, tz = [x - y for x, y in zip(u, fu)]
            val = (1.0 - tx) * ((1.0 - ty) * ((1.0 - tz) * w[0] + tz * w[1]) + ty * ((1.0 - tz) * w[2] + tz * w[3])) \
                + tx * ((1.0 - ty) * ((1.0 - tz) * w[4] + tz * w[5]) + ty * ((1.0 - tz) * w[6] + tz * w[7]))
        ok &= np.isfinite(val)
        tot += np.where(ok, val, 0.)
        cnt += ok
        if not ok.any():
            failures.append(L)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, tot / cnt, np.nan)
    return np.ma.array(mean, mask=cnt == 0), failures, cnt
