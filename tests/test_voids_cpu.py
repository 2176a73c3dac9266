"""CPU: the numpy statement of the void definitions (tests/voids_numpy.py) against a brute-force walk per voxel, its invariants,
and the reference's own per-label loops (fastbox/voids.py, restated with np.where per label); the library exports the void
entries and the module refuses bad arguments before it touches a device."""
import os
import types

import numpy as np
import pytest

from tests import voids_numpy as vn

STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def _box(N, scale=(1e3, 1e3, 1e3)):
    b = types.SimpleNamespace(N=N)
    b.x, b.y, b.z = [np.linspace(-0.5 * s, 0.5 * s, N) for s in scale]
    return b


def _field(N, seed, quantum=None):
    f = np.random.RandomState(seed).normal(size=(N, N, N))
    f = f + 0.5 * (np.roll(f, 1, 0) + np.roll(f, 1, 1) + np.roll(f, 1, 2))     # basins of several voxels
    if quantum:
        f = np.round(f / quantum) * quantum                                         # plateaus: many equal neighbours
    return f


def brute(f, ins):
    """Per voxel: step to the least in-mask face neighbour while it is below (f, i); minima numbered in raster order."""
    N = f.shape[0]

    def nxt(i):
        x, y, z = np.unravel_index(i, (N, N, N))
        best = i
        for dx, dy, dz in STEPS:
            a, b, c = x + dx, y + dy, z + dz
            if 0 <= a < N and 0 <= b < N and 0 <= c < N:
                j = (a * N + b) * N + c
                if ins.flat[j] and (f.flat[j], j) < (f.flat[best], best):
                    best = j
        return best

    par = {i: nxt(i) for i in range(N ** 3) if ins.flat[i]}
    minima = sorted(i for i, p in par.items() if p == i)
    num = {m: k + 1 for k, m in enumerate(minima)}
    lab = np.zeros(N ** 3, dtype=np.int32)
    for i in par:
        j = i
        while par[j] != j:
            j = par[j]
        lab[i] = num[j]
    return lab.reshape(N, N, N), len(minima)


def _cases(N, seed):
    f = _field(N, seed)
    q = _field(N, seed, quantum=0.5)
    cub = np.zeros((N, N, N), dtype=bool)
    cub[1:N - 1, 0:N - 2, 2:N] = True                       # a cuboid mask
    g = f.copy()
    g.flat[np.random.RandomState(seed).choice(N ** 3, N, replace=False)] = np.nan
    return [("plain", f, vn.inside(f)), ("plateaus", q, vn.inside(q)), ("cuboid mask", q, vn.inside(q, mask=cub)),
            ("threshold", f, vn.inside(f, threshold=0.)), ("nan", g, vn.inside(g))]


@pytest.mark.parametrize("N", [6, 8, 10])
def test_oracle_watershed_is_the_per_voxel_walk(N):
    for name, f, ins in _cases(N, N):
        lab, n = vn.watershed(f, ins)
        blab, bn = brute(f, ins)
        assert n == bn, name
        np.testing.assert_array_equal(lab, blab, err_msg=name)


@pytest.mark.parametrize("N", [10, 16])
def test_oracle_invariants(N):
    for name, f, ins in _cases(N, N + 1):
        lab, n = vn.watershed(f, ins)
        par = vn.descend(f, ins)
        fl, idx = f.reshape(-1), np.arange(N ** 3)
        m = par >= 0
        assert np.array_equal(m, ins.reshape(-1)) and np.all(lab.reshape(-1)[~m] == 0), name
        # every step strictly descends in (f, i), and stays in the mask
        step = m & (par != idx)
        j = par[step]
        assert np.all((fl[j] < fl[step]) | ((fl[j] == fl[step]) & (j < idx[step]))), name
        assert np.all(ins.reshape(-1)[j]), name
        # labels are dense and every region holds exactly one minimum
        minima = idx[par == idx]
        assert sorted(np.unique(lab[lab > 0]).tolist()) == list(range(1, n + 1)), name
        assert np.array_equal(np.sort(lab.reshape(-1)[minima]), np.arange(1, n + 1)), name
        assert np.array_equal(lab.reshape(-1)[minima], np.arange(1, n + 1)), name       # raster order of the minima


def _ref_centroid(void_cat, labels, box, field, kind):
    out = {}
    for lbl in void_cat:
        ix, iy, iz = idxs = np.where(labels == lbl)
        if kind == 'minimum':
            ii = np.argmin(field[idxs])
            out[lbl] = np.array([box.x[ix[ii]], box.y[iy[ii]], box.z[iz[ii]]])
            continue
        if kind == 'uniform':
            w = 1. / ix.size
        else:
            w = field[idxs].flatten()
            w *= -1.
            w[w < 0.] = 0.
            w /= np.sum(w)
        out[lbl] = np.array([np.sum(w * box.x[ix]), np.sum(w * box.y[iy]), np.sum(w * box.z[iz])])
    return out


def _ref_radii(void_cat, labels, box):
    dV = (box.x[1] - box.x[0]) * (box.y[1] - box.y[0]) * (box.z[1] - box.z[0])
    return {lbl: (3. * dV * np.where(labels == lbl)[0].size / (4. * np.pi)) ** (1. / 3.) for lbl in void_cat}


def _ref_trim(labels, nmin, nmax):
    unique, counts = np.unique(labels, return_counts=True)
    return unique[np.logical_and(counts >= nmin, counts <= nmax)]


@pytest.mark.parametrize("scale", [(1e3, 1e3, 1e3), (1e3, 7e2, 1.3e3)])
def test_oracle_catalogue_is_the_reference_loops(scale):
    N = 16
    box = _box(N, scale)
    f = _field(N, 4)
    lab, n = vn.watershed(f, vn.inside(f, threshold=0.5))
    st = vn.region_stats(lab, n, f)
    assert st["count"][0] > 0
    for nmin, nmax in ((1, 10 ** 9), (3, 40), (st["count"][0], st["count"][0])):
        np.testing.assert_array_equal(vn.trim(st, nmin, nmax), _ref_trim(lab, nmin, nmax))
    assert 0 in vn.trim(st, 1, 10 ** 9)                       # label 0 qualifies like any other
    cat = vn.trim(st, 1, 10 ** 9)
    r = _ref_radii(cat, lab, box)
    np.testing.assert_allclose(vn.radii(st, box)[cat], [r[k] for k in cat], rtol=1e-14)
    for kind in ("uniform", "minimum", "density"):
        ref = _ref_centroid(cat[1:], lab, box, f, kind)
        np.testing.assert_allclose(vn.centroids(st, box, kind)[cat[1:]], [ref[k] for k in cat[1:]], rtol=0,
                                   atol=1e-12 * max(scale))


def test_oracle_merge_and_stack_basics():
    N = 12
    box = _box(N)
    f = _field(N, 9)
    lab, n = vn.watershed(f, vn.inside(f))
    st = vn.region_stats(lab, n, f)
    same, m0 = vn.merge(lab, n, st["mean"], 0.)
    assert m0 == n and np.array_equal(same, lab)                # nothing below a zero threshold
    one, m1 = vn.merge(lab, n, st["mean"], np.inf)
    assert m1 == 1 and np.all(one == 1)                         # one connected box
    # a constant field stacks to itself wherever a void is valid
    c = np.full((N, N, N), 2.5)
    cat = vn.trim(st, 8, 10 ** 9)
    cat = cat[cat > 0]
    cen, rad = vn.centroids(st, box, "uniform")[cat], vn.radii(st, box)[cat]
    o, fail, cnt = vn.stack(lab, c, cat, cen, rad, box, 1., 9)
    assert cnt.sum() > 0 and np.allclose(o.compressed(), 2.5) and set(fail) < set(cat.tolist())


def test_library_exports_void_entries():
    from fastbox_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load()
    for name in ("fb_watershed", "fb_region_stats", "fb_merge_regions", "fb_stack_voids"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_arguments_are_checked_before_the_device():
    from fastbox_amd import voids
    with pytest.raises(NotImplementedError, match="markers"):
        voids.watershed(np.zeros((4, 4, 4)), markers=5)
    with pytest.raises(NotImplementedError, match="markers"):
        voids.apply_watershed(np.zeros((4, 4, 4)), markers=np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="box="):
        voids.watershed(np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="not recognised"):
        voids.void_centroids([1], np.zeros((4, 4, 4)), _box(4), kind="median")
    with pytest.raises(ValueError, match="not recognised"):
        voids.stack_voids([1], np.zeros((4, 4, 4)), _box(4), np.zeros((4, 4, 4)), centroid_kind="median")
    lab = np.array([[[0, 1], [1, 2]], [[2, 2], [0, 0]]])
    np.testing.assert_array_equal(voids.trim_by_volume(lab, 2, 3), _ref_trim(lab, 2, 3))
