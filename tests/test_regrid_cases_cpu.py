"""CPU: the numpy statements of tests/regrid_numpy.py against scipy's RegularGridInterpolator behind the NaN fill, against
np.histogramdd, and against the reference's own results (tests/golden/analysis_n16.npz, which pins the 'xy' axis order), on every
case of tests/regrid_cases.py; what keeps each case from being vacuous; and comoving_dimensions_from_survey."""
import os

import numpy as np
import pytest

from tests import particle_cases as pc
from tests import regrid_cases as rc
from tests import regrid_numpy as rn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis_n16.npz")
RG = rc.regrid_cases()
GC = rc.grid_cases()


def _scipy_regrid(field, coords_orig, coords_new):
    """analysis.py:31-70 written out: the fill, the interpolator, numpy's default 'xy' meshgrid."""
    from scipy.interpolate import RegularGridInterpolator
    interp = RegularGridInterpolator(tuple(coords_orig), rn.fill_nan_channel_mean(field), method="linear", bounds_error=False,
                                     fill_value=np.nan)
    x3, y3, z3 = np.meshgrid(*coords_new)
    return interp(np.array([x3.flatten(), y3.flatten(), z3.flatten()]).T).reshape(x3.shape)


def fp64_bound(case):
    """(64 + nx ny) 2^-53 max|v|: eight products of three rounded factors with weights that sum to 1 cost a few tens of ulps, the
    channel mean at most nx ny ulps of reordering."""
    nx, ny, _ = case["field"].shape
    return (64 + nx * ny) * 2. ** -53 * rc.filled_max(case["field"])


@pytest.mark.parametrize("name", sorted(RG))
def test_regrid_statement_is_scipy(name):
    c = RG[name]
    got = rn.interpolate_onto_grid(c["field"], c["coords_orig"], c["coords_new"])
    want = _scipy_regrid(c["field"], c["coords_orig"], c["coords_new"])
    assert got.shape == want.shape == (c["coords_new"][1].size, c["coords_new"][0].size, c["coords_new"][2].size)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if c.get("outside"):
        assert not ok.any()
        return
    assert 2 * ok.sum() >= ok.size, "%d of %d are NaN" % ((~ok).sum(), ok.size)
    assert np.max(np.abs(got[ok] - want[ok])) <= fp64_bound(c)
    ij = rn.interpolate_onto_grid(c["field"], c["coords_orig"], c["coords_new"], indexing="ij")
    np.testing.assert_array_equal(ij.transpose(1, 0, 2), got)


def test_regrid_cases_are_what_they_claim():
    assert rn.interpolate_onto_grid(**_args(RG["onto the box"])).shape == (rc.BOX_N,) * 3
    assert all(np.all(np.diff(g) > 0) and np.ptp(np.diff(g)) > 0.1 for g in RG["onto the box"]["coords_orig"])     # non-uniform
    assert RG["wave tail"]["coords_new"][2].size == 11 and np.all(np.diff(RG["wave tail"]["coords_new"][1]) < 0)
    # on the nodes the result is the input; one ulp outside is NaN on that axis alone
    c = RG["on nodes"]
    v = rn.interpolate_onto_grid(**_args(c), indexing="ij")
    np.testing.assert_array_equal(v[1:, :-1, 1:-1], c["field"])
    assert np.isnan(v[0]).all() and np.isnan(v[:, -1]).all() and np.isnan(v[:, :, 0]).all() and np.isnan(v[:, :, -1]).all()
    assert min(RG["two nodes"]["field"].shape) == 2
    # one NaN voxel reads as its channel's mean: the result is finite and differs from what a zero would give
    c = RG["nan voxel"]
    v = rn.interpolate_onto_grid(**_args(c))
    z = rn.interpolate_onto_grid(np.nan_to_num(c["field"]), c["coords_orig"], c["coords_new"])
    np.testing.assert_array_equal(np.isnan(v), np.isnan(z))
    assert np.nanmax(np.abs(v - z)) > 0.1
    # a NaN channel is lost with the cells it bounds, and with weight 0 too
    c = RG["nan channel"]
    v = rn.interpolate_onto_grid(**_args(c), indexing="ij")
    zin = c["coords_new"][2]
    lost = (zin >= c["coords_orig"][2][0]) & (zin < c["coords_orig"][2][1])
    assert lost.any() and np.isnan(v[:, :, lost]).all() and np.isfinite(v[:, :, zin >= c["coords_orig"][2][1]]).all()
    c = RG["nan of weight zero"]
    v = rn.interpolate_onto_grid(**_args(c), indexing="ij")
    assert c["coords_new"][2][-1] == c["coords_orig"][2][-1] and np.isnan(v[:, :, -1]).all() and np.isfinite(v[:, :, 0]).all()
    assert np.isfinite(c["field"][:, :, -1]).all()               # the node the point sits on is finite: only the weight-0 node is not
    assert RG["several workgroups"]["field"].shape == (48, 40, 56)


def _args(c):
    return dict(field=c["field"], coords_orig=c["coords_orig"], coords_new=c["coords_new"])


def _histogramdd(c):
    pos = c["pos"]
    lims = [rn.hist_limits(*((pos[:, a].min(), pos[:, a].max()) if c["limits"][a] is None else c["limits"][a])) for a in range(3)]
    grid, _ = np.histogramdd(pos, bins=c["nbin"], range=lims, weights=c["w"])
    return grid


@pytest.mark.parametrize("name", sorted(GC))
def test_grid_statement_is_histogramdd(name):
    c = GC[name]
    grid, grids = rn.grid_catalogue(c["pos"], c["w"], c["limits"], c["nbin"])
    np.testing.assert_array_equal(grid, _histogramdd(c))
    assert grid.shape == tuple(c["nbin"]) and [g.size for g in grids] == list(c["nbin"])


def test_grid_cases_are_what_they_claim():
    c = GC["on edges"]
    grid, _ = rn.grid_catalogue(c["pos"], None, c["limits"], c["nbin"])
    assert 0 < grid.sum() < c["pos"].shape[0] and np.isnan(c["pos"]).any()
    assert grid[-1, -1, -1] >= 1 and grid[0, 0, 0] >= 1                   # the last edge is in the last bin, the first in the first
    c = GC["beside an edge"]
    x = c["pos"][:, 0]
    b = rn.hist_bins(x, 0.1, 0.7, 6)
    assert list(b[2:7]) == [0, 1, 2, 3, 4] and list(b[7:14]) == [0, 1, 2, 3, 4, 5, 5] and list(b[14:]) == [1, 2, 3, 4, 5]
    guess = np.minimum(((x - 0.1) * (6 / (0.7 - 0.1))).astype(int), 5)
    assert np.sum(guess != b) >= 2                               # the arithmetic guess alone misplaces points on an edge
    c = GC["one particle"]
    grid, grids = rn.grid_catalogue(c["pos"], None, c["limits"], c["nbin"])
    assert grid.sum() == 1 and grids[0][0] == 0.75 and grids[0][-1] == 1.75
    assert rn.grid_catalogue(GC["no particle"]["pos"], None, GC["no particle"]["limits"], (2, 3, 4))[0].sum() == 0
    assert GC["non-cubic"]["nbin"] == (3, 5, 70)


@pytest.mark.parametrize("wname", ["unweighted", "signed", "span 2^40"])
def test_weighted_cloud_is_histogramdd(wname):
    L = (32., 32., 32.)
    pos = rc.cloud(5000, L)
    w = pc.weight_sets(pos.shape[0])[wname][0]
    grid, _ = rn.grid_catalogue(pos, w, [(0., 32.)] * 3, (16,) * 3)
    want, _ = np.histogramdd(pos, bins=(16,) * 3, range=[(0., 32.)] * 3, weights=w)
    np.testing.assert_array_equal(grid, want)                    # integer weights below 2^53: every order of the adds is exact
    assert 0.7 * pos.shape[0] < np.histogramdd(pos, bins=(16,) * 3, range=[(0., 32.)] * 3)[0].sum() < pos.shape[0]


def test_statements_against_the_reference():
    g = np.load(GOLD)
    orig = [g["rg_x"], g["rg_y"], g["rg_z"]]
    for new, key in (([g["rg_xnew"], g["rg_ynew"], g["rg_znew"]], "rg_out"),
                     ([g["rg_box_xnew"], g["rg_box_ynew"], g["rg_box_znew"]], "rg_box")):
        got = rn.interpolate_onto_grid(g["rg_field"], orig, new)
        want = g[key]
        assert got.shape == want.shape == (new[1].size, new[0].size, new[2].size)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert 2 * ok.sum() >= ok.size
        assert np.max(np.abs(got[ok] - want[ok])) <= (64 + 35) * 2. ** -53 * rc.filled_max(g["rg_field"])
    # the 'xy' order is not a symmetric accident: x_new and y_new differ in length
    assert g["rg_out"].shape == (4, 9, 11)
    lim = [(0., 32.)] * 3
    np.testing.assert_array_equal(rn.grid_catalogue(g["gc_pos"], None, lim, (16,) * 3)[0], g["gc_count"])
    np.testing.assert_array_equal(rn.grid_catalogue(g["gc_pos"], g["gc_w"], lim, (16,) * 3)[0], g["gc_weighted"])
    grid, grids = rn.grid_catalogue(g["gc_pos"], None, [None] * 3, (3, 5, 7))
    np.testing.assert_array_equal(grid, g["gc_range"])
    assert grid.sum() == g["gc_pos"].shape[0]
    for a, key in enumerate(("gc_x", "gc_y", "gc_z")):
        np.testing.assert_array_equal(grids[a], g[key])          # np.linspace(lo, hi, n): not the bin centres


def test_comoving_dimensions_from_survey():
    from fastbox_amd import default_cosmo
    from fastbox_amd.box import _ccl
    from fastbox_amd.utils import comoving_dimensions_from_survey, LINE_FREQ
    cosmo = default_cosmo if isinstance(default_cosmo, _ccl.Cosmology) else _ccl.Cosmology(**default_cosmo)
    freqs = (1000., 1100.)
    zr = (LINE_FREQ / freqs[0] - 1., LINE_FREQ / freqs[1] - 1.)
    zc, (Lx, Ly, Lz) = comoving_dimensions_from_survey(cosmo, (10., 30.), freq_range=freqs)
    zc2, dims2 = comoving_dimensions_from_survey(cosmo, (10., 30.), z_range=zr)
    assert zc == zc2 and (Lx, Ly, Lz) == dims2
    zmin, zmax = sorted(zr)
    r = [_ccl.comoving_radial_distance(cosmo, 1. / (1. + z)) for z in (zmin, zmax)]
    assert Lz == r[1] - r[0] and Lz > 0.
    assert zmin < zc < zmax
    assert Ly / Lx == pytest.approx(3., rel=1e-15)
    assert Lx == pytest.approx(10. * np.pi / 180. * _ccl.comoving_angular_distance(cosmo, 1. / (1. + zc)), rel=1e-15)
    # the array form of the radial distance is the scalar form, element by element
    a = 1. / (1. + np.linspace(zmin, zmax, 5))
    np.testing.assert_array_equal(_ccl.comoving_radial_distance(cosmo, a), [_ccl.comoving_radial_distance(cosmo, float(v)) for v in a])
    with pytest.raises(ValueError):
        comoving_dimensions_from_survey(cosmo, (10., 30.), freq_range=freqs, z_range=zr)
    with pytest.raises(ValueError):
        comoving_dimensions_from_survey(cosmo, (10., 30.))
