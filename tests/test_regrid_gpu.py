"""GPU: interpolate_onto_grid and grid_catalogue (fb_regrid.hip) on the constructed cases of tests/regrid_cases.py, in both
precisions, against the numpy statements of tests/regrid_numpy.py -- which tests/test_regrid_cases_cpu.py holds to scipy, to
np.histogramdd and to the reference's own results -- and against np.histogramdd itself.  Every shape is 64^3 or smaller."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, DeviceArray, analysis, default_cosmo
from fastbox_amd.halos import HaloCatalogue
from tests import particle_cases as pc
from tests import regrid_cases as rc
from tests import regrid_numpy as rn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
RG = rc.regrid_cases()
GC = rc.grid_cases()
L = (32., 32., 32.)


@functools.lru_cache(maxsize=None)
def _box(prec, N=rc.BOX_N):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng="device", seed=7)


@functools.lru_cache(maxsize=None)
def _statement(name, indexing):
    c = RG[name]
    want = rn.interpolate_onto_grid(c["field"], c["coords_orig"], c["coords_new"], indexing=indexing)
    want.setflags(write=False)
    return want


def _bound(c, prec):
    """fp64 plan: (64 + nx ny) 2^-53 max|v| -- eight products of three rounded factors with weights that sum to 1 cost a few tens
    of ulps, the channel mean at most nx ny ulps of reordering.  f32 plan: 3 2^-24 max|v| -- one rounding on upload, one on
    store, and a convex combination does not amplify them.  max|v| over the filled input."""
    nx, ny, _ = c["field"].shape
    return ((64 + nx * ny) * 2. ** -53 if prec == "f64" else 3. * 2. ** -24) * rc.filled_max(c["field"])


def _regrid(c, prec, indexing="xy"):
    return analysis.interpolate_onto_grid(c["field"], c["coords_orig"], c["coords_new"], box=_box(prec), indexing=indexing)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(RG))
def test_regrid_is_the_statement(name, prec):
    c = RG[name]
    for indexing in ("xy", "ij"):
        got = _regrid(c, prec, indexing)
        want = _statement(name, indexing)
        assert isinstance(got, DeviceArray if c.get("box") else np.ndarray)
        got = np.asarray(got)
        assert got.shape == want.shape and got.dtype == np.float64
        if indexing == "xy":
            assert got.shape == (c["coords_new"][1].size, c["coords_new"][0].size, c["coords_new"][2].size)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if c.get("outside"):
            assert not ok.any()
            continue
        assert 2 * ok.sum() >= ok.size
        err = np.max(np.abs(got[ok] - want[ok]))
        print("%s, %s, %s: max error %.3e, bound %.3e" % (name, prec, indexing, err, _bound(c, prec)))
        assert err <= _bound(c, prec)
        np.testing.assert_array_equal(np.asarray(_regrid(c, prec, indexing)), got)          # bitwise repeatable


@pytest.mark.parametrize("prec", PRECS)
def test_regrid_wave_tail_has_the_xy_shape(prec):
    got = _regrid(RG["wave tail"], prec)
    assert got.shape == (4, 9, 11)
    np.testing.assert_array_equal(_regrid(RG["wave tail"], prec, "ij").transpose(1, 0, 2), got)


@pytest.mark.parametrize("prec", PRECS)
def test_regrid_of_a_device_cube(prec):
    """A real DeviceArray names the engine itself; its values are the box's precision already."""
    box = _box(prec)
    N = box.N
    f = np.random.RandomState(5).normal(size=(N, N, N)).astype(DT[prec]).astype(np.float64)
    f[3, 4, 5] = np.nan
    g = [np.arange(N) * 2., np.arange(N) * 2. + 1., np.cumsum(np.arange(1., N + 1.))]
    new = [rc._span(g[0], 9), rc._inside(g[1], 4), rc._span(g[2], 11)]
    got = analysis.interpolate_onto_grid(box.engine.upload(f, "real"), g, new)
    want = rn.interpolate_onto_grid(f, g, new)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert 2 * ok.sum() >= ok.size
    c = dict(field=f)
    assert np.max(np.abs(got[ok] - want[ok])) <= _bound(c, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_regrid_refuses_bad_coordinates(prec):
    c = RG["wave tail"]
    box = _box(prec)
    g = c["coords_orig"]
    for bad in ([g[0][::-1], g[1], g[2]], [g[0], g[1], np.concatenate([g[2][:2], g[2][1:-1]])], [g[0], g[1][:-1], g[2]]):
        with pytest.raises(ValueError):
            analysis.interpolate_onto_grid(c["field"], bad, c["coords_new"], box=box)
    with pytest.raises(TypeError):
        analysis.interpolate_onto_grid(c["field"], g, c["coords_new"])
    with pytest.raises(ValueError):
        analysis.interpolate_onto_grid(c["field"][:, :, :1], [g[0], g[1], g[2][:1]], c["coords_new"], box=box)


# ---- grid_catalogue ---------------------------------------------------------------------------------------------------------------
def _catalogue(box, pos):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    return HaloCatalogue(box.engine, box.engine.upload_raw(pos) if pos.shape[0] else None, pos.shape[0])


def _histogramdd(pos, w, limits, nbin):
    lims = [rn.hist_limits(*((pos[:, a].min(), pos[:, a].max()) if limits[a] is None else limits[a])) for a in range(3)]
    return np.histogramdd(pos, bins=nbin, range=lims, weights=w)[0], lims


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(GC))
def test_grid_is_histogramdd(name, prec):
    c = GC[name]
    box = _box(prec)
    pos, nbin = c["pos"], c["nbin"]
    kw = dict(nx=nbin[0], ny=nbin[1], nz=nbin[2])
    for key, lim in zip(("xlim", "ylim", "zlim"), c["limits"]):
        if lim is not None:
            kw[key] = lim
    if any(lim is None for lim in c["limits"]):                  # the data's range: a catalogue, no box
        grid, grids = analysis.grid_catalogue(_catalogue(box, pos), **kw)
    else:
        grid, grids = analysis.grid_catalogue(pos[:, 0], pos[:, 1], pos[:, 2], box=box, **kw)
    want, lims = _histogramdd(pos, None, c["limits"], nbin)
    assert isinstance(grid, np.ndarray) and grid.dtype == np.float64 and grid.shape == tuple(nbin)
    np.testing.assert_array_equal(grid, want)
    for a in range(3):
        np.testing.assert_array_equal(grids[a], np.linspace(lims[a][0], lims[a][1], nbin[a]))
    # the (n, 3) form and a second call give the same bits
    if all(lim is not None for lim in c["limits"]):
        np.testing.assert_array_equal(analysis.grid_catalogue(pos, box=box, **kw)[0], grid)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("wname", ["unweighted", "signed", "span 2^40"])
def test_grid_cloud_onto_the_box(wname, prec):
    box = _box(prec)
    N = box.N
    pos = rc.cloud(5000, L)
    n = pos.shape[0]
    w = pc.weight_sets(n)[wname][0]
    grid, grids = analysis.grid_catalogue(pos, w=w, box=box)               # nx, ny, nz and the limits from the box
    assert isinstance(grid, DeviceArray)
    got = np.asarray(grid)
    want, _ = np.histogramdd(pos, bins=(N,) * 3, range=[(0., 32.)] * 3, weights=w)
    count, _ = np.histogramdd(pos, bins=(N,) * 3, range=[(0., 32.)] * 3)
    assert 0.7 * n < count.sum() < n
    if w is None:
        np.testing.assert_array_equal(got, want)
    F = pc.paint_exponent(w, n) + (32 if prec == "f64" else 0)
    tol = count * 2. ** -F + pc.storage_bound(want, DT[prec])
    err = np.abs(got - want)
    print("%s, %s: F = %d, largest error %.3e where the bound is %.3e" % (wname, prec, F, err.max(), tol.flat[np.argmax(err)]))
    assert np.all(err <= tol)
    for a in range(3):
        np.testing.assert_array_equal(grids[a], np.linspace(0., 32., N))
    # the same bits from call to call, for any order of the particles, and from a catalogue on the device
    np.testing.assert_array_equal(np.asarray(analysis.grid_catalogue(pos, w=w, box=box)[0]), got)
    perm = np.random.RandomState(3).permutation(n)
    np.testing.assert_array_equal(np.asarray(analysis.grid_catalogue(pos[perm], w=None if w is None else w[perm], box=box)[0]), got)
    np.testing.assert_array_equal(np.asarray(analysis.grid_catalogue(_catalogue(box, pos), w=w, box=box)[0]), got)


@pytest.mark.parametrize("prec", PRECS)
def test_grid_refuses_what_numpy_refuses(prec):
    box = _box(prec)
    pos = GC["non-cubic"]["pos"]
    with pytest.raises(TypeError):
        analysis.grid_catalogue(pos, nx=2, ny=2, nz=2)                     # host positions and no box: no engine
    with pytest.raises(ValueError):
        analysis.grid_catalogue(_catalogue(box, pos), nx=2, ny=2)          # a missing n without a box
    bad = pos.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError):
        analysis.grid_catalogue(_catalogue(box, bad), nx=2, ny=2, nz=2)    # a range that is not finite
    grid, _ = analysis.grid_catalogue(_catalogue(box, bad), nx=2, ny=2, nz=2, ylim=(0., 5.))
    assert grid.sum() == np.histogramdd(bad, bins=(2, 2, 2), range=[(bad[:, 0].min(), bad[:, 0].max()), (0., 5.),
                                                                    (bad[:, 2].min(), bad[:, 2].max())])[0].sum()
    with pytest.raises(ValueError):
        analysis.grid_catalogue(pos, w=np.ones(3), box=box)
