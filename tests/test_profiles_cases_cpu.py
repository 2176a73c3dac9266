"""CPU: the constructed halo-profile cases of tests/profiles_cases.py do what they claim, the numpy statement
tests/profiles_numpy.py agrees with scipy's periodic k-d tree, and the product's pure-numpy spherical-overdensity finish
(fastbox_amd.halos.so_from_enclosed) agrees with the statement.  tests/test_profiles_gpu.py runs the same cases on the
device."""
import numpy as np
import pytest

from fastbox_amd import halos
from tests import pairs_numpy as pn
from tests import profiles_cases as pc
from tests import profiles_numpy as pf
from tests.fof_numpy import min_image, wrap

NCASES = len(pc.NAMES)


def _cells(case):
    return halos.pair_cells(case["L"], (case["edges"][-1],) * 3, max(case["pos"].shape[0], 1))


def _d2(case, h):
    L = np.array(case["L"])
    d = min_image(wrap(case["pos"], L) - wrap(case["centres"][h], L), L)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@pytest.mark.parametrize("index", range(NCASES), ids=pc.NAMES)
def test_statement_agrees_with_the_tree(index):
    """N(< e_j) of the statement against the tree's #{d <= e_j}: equal wherever no particle is at distance e_j exactly; the
    ties are counted on squares and account for every difference."""
    case, inner, counts = pc.reference(index)
    enclosed = np.concatenate([inner[:, None], inner[:, None] + np.cumsum(counts, axis=1)], axis=1)
    tree = pf.tree_profiles(case["centres"], case["pos"], case["L"], case["edges"])
    e2 = case["edges"] * case["edges"]
    ties = np.array([[np.count_nonzero(_d2(case, h) == e2[j]) for j in range(e2.size)] for h in range(min(len(inner), 64))])
    if case["name"].startswith("1 edges"):      # on e0 (or the centre itself at e0 = 0), on the interior edge, on the last edge
        assert ties.sum() == (3 if case["edges"][0] > 0. else 4)
    else:                                       # random coordinates: nothing on an edge
        assert ties.sum() == 0
        np.testing.assert_array_equal(tree, enclosed)
    np.testing.assert_array_equal(tree[:ties.shape[0]] - ties, enclosed[:ties.shape[0]])
    assert enclosed.max() > 0


def test_edge_cases_have_the_rows_stated_by_hand():
    for name in ("1 edges e0=0.5", "1 edges e0=0"):
        case, inner, counts = pc.reference(pc.index_of(name))
        np.testing.assert_array_equal(inner, case["expect_inner"])
        np.testing.assert_array_equal(counts, case["expect_counts"])
        d2 = _d2(case, 0)
        e2 = case["edges"] * case["edges"]
        assert np.count_nonzero(d2 == 0.) == 1 and np.count_nonzero(d2 == e2[-1]) == 1 and np.count_nonzero(d2 == e2[-2]) == 1
        assert np.count_nonzero(d2 == 0.25) == 1                    # 0.5^2: the first edge, or an interior one


def test_seam_centres():
    case, inner, counts = pc.reference(pc.index_of("2 seam"))
    L = np.array(case["L"])
    w = wrap(case["centres"], L)
    np.testing.assert_array_equal(w[0], w[1])                        # the shifted copy wraps onto the centre exactly
    assert np.all(w[2] < 8.) and np.all(w[2] == np.nextafter(8., 0.)) and np.all(case["centres"][1] != case["centres"][0])
    np.testing.assert_array_equal(counts[0], counts[1])
    assert inner[0] == inner[1]
    # members across all three faces: of the particles inside the last edge, some in each of the eight octants
    d = min_image(wrap(case["pos"], L) - w[0], L)
    inside = (d * d).sum(axis=1) < case["edges"][-1] ** 2
    octants = set(map(tuple, (d[inside] > 0.).astype(int)))
    assert len(octants) == 8 and counts[0].sum() > 50 and counts[2].sum() > 50
    raw = case["pos"][inside] - w[0]
    assert np.any(np.abs(raw) > 4., axis=1).sum() > 40               # their plain differences are a box length off


def test_cuboid_cells_coincide():
    case, inner, counts = pc.reference(pc.index_of("3 cuboid (2, 3, 7) cells"))
    assert _cells(case) == pc.CUBOID_CELLS
    occ = pn.cells_of(case["centres"], case["L"], pc.CUBOID_CELLS).reshape(pc.CUBOID_CELLS)
    assert occ[:, :, 0].sum() > 0 and occ[:, :, -1].sum() > 0 and occ[:, :, 1:-1].sum() > 0      # both seam columns and inner ones
    assert counts.sum() > 1000


@pytest.mark.parametrize("k", pc.CROWDED)
def test_crowded_cell_holds_exactly_k(k):
    case, inner, counts = pc.reference(pc.index_of("4 crowded cell of %d" % k))
    cells = _cells(case)
    occ = pn.cells_of(case["pos"], case["L"], cells)
    assert occ.max() == k and np.count_nonzero(occ) == 1 and cells[0] in (5, 8)
    assert counts[0].sum() == k and counts[1].sum() == k and 0 < counts[2].sum() < k


def test_many_centres_outnumber_the_workgroups():
    case, inner, counts = pc.reference(pc.index_of("5 many centres"))
    assert case["centres"].shape[0] == 3000 > 8 * 256 and case["pos"].shape[0] == 5000
    np.testing.assert_array_equal(case["centres"][0], case["centres"][1])
    np.testing.assert_array_equal(counts[0], counts[1])
    assert counts[0].sum() > 0 and np.count_nonzero(counts.sum(axis=1)) > 2900


def test_bin_count_limits():
    for nr in (1, 256):
        case, inner, counts = pc.reference(pc.index_of("6 nr=%d" % nr))
        assert counts.shape == (20, nr) == (20, halos.profile_edges(case["L"], case["edges"]).size - 1) and counts.sum() > 100
    assert halos.PROFILE_MAX_NR == 256
    with pytest.raises(ValueError, match="at most 256 bins"):
        halos.profile_edges((16.,) * 3, np.linspace(0., 3.5, 258))
    with pytest.raises(ValueError, match="strictly ascending"):
        halos.profile_edges((16.,) * 3, [1., 3., 2.])
    with pytest.raises(ValueError, match="below half"):
        halos.profile_edges((16., 16., 40.), [1., 8.])


def test_blobs_have_radii_and_the_finish_agrees_with_the_statement():
    """status 0 for the three blobs at both thresholds, so that the device comparison cannot pass on NaN alone; status 1 in
    the void; status 2 with rmax = 0.3; and the product's vectorised finish against the statement's loop."""
    case, inner, counts = pc.reference(pc.index_of("7 blobs rmax=4"))
    so = case["so"]
    enclosed = np.concatenate([inner[:, None], inner[:, None] + np.cumsum(counts, axis=1)], axis=1)
    radii = {}
    for delta in so["deltas"]:
        r, m, st = pf.so_statement(case["edges"], inner, counts, so["particle_mass"], so["rho_ref"], delta)
        print("Delta = %g: R = %s, status %s" % (delta, r, st))
        np.testing.assert_array_equal(st, [0, 0, 0, 1])
        assert np.all(np.isfinite(r[:3])) and np.isnan(r[3]) and np.isnan(m[3])
        np.testing.assert_allclose(m[:3], 4. * np.pi / 3. * delta * so["rho_ref"] * r[:3] ** 3, rtol=1e-14)
        gr, gm, gs = halos.so_from_enclosed(case["edges"], enclosed, so["particle_mass"], so["rho_ref"], delta)
        np.testing.assert_array_equal(gs, st)
        np.testing.assert_allclose(gr, r, rtol=1e-12)
        np.testing.assert_allclose(gm, m, rtol=1e-12)
        radii[delta] = r
    assert np.all(radii[500.][:3] < radii[200.][:3])
    # the largest blob, 1200 points of sigma = 0.8, has R_200 beyond 2 sigma; the smallest, 150 of sigma = 0.3, near 3 sigma
    assert 1.6 < radii[200.][2] < 2.2 and 0.7 < radii[200.][1] < 1.3 and 1.2 < radii[200.][0] < 1.9
    assert pc.void_centre(case["pos"])[1] > 1.
    case, inner, counts = pc.reference(pc.index_of("7 blobs rmax=0.3"))
    enclosed = np.concatenate([inner[:, None], inner[:, None] + np.cumsum(counts, axis=1)], axis=1)
    for delta in so["deltas"]:
        r, m, st = pf.so_statement(case["edges"], inner, counts, so["particle_mass"], so["rho_ref"], delta)
        np.testing.assert_array_equal(st, [2, 2, 2, 1])
        gr, gm, gs = halos.so_from_enclosed(case["edges"], enclosed, so["particle_mass"], so["rho_ref"], delta)
        np.testing.assert_array_equal(gs, st)
        assert np.all(np.isnan(gr)) and np.all(np.isnan(gm)) and np.all(np.isnan(r))


def test_finish_on_hand_made_enclosed_counts():
    """One row per status, and the interpolation by hand: edges (1, 2, 4), unit mass and rho_ref, threshold 5."""
    e = np.array([1., 2., 4.])
    v = 4. * np.pi / 3. * e ** 3
    enclosed = np.array([[50, 60, 61],                               # rho = 11.9, 1.79, 0.23: crosses between 1 and 2
                         [1, 2, 3],                                  # never above 5
                         [100, 800, 6400],                           # rho = 23.9 at every edge: still above at the last
                         [50, 60, 1400],                             # above again at the last edge: status 2, not the first crossing
                         [1, 200, 210]])                             # below at edge 0, above at 1, below at 2: the outermost crossing
    r, m, st = halos.so_from_enclosed(e, enclosed, 1., 1., 5.)
    np.testing.assert_array_equal(st, [0, 1, 2, 2, 0])
    rho0, rho1 = 50. / v[0], 60. / v[1]
    want = np.exp(np.log(1.) + (np.log(5.) - np.log(rho0)) * (np.log(2.) - np.log(1.)) / (np.log(rho1) - np.log(rho0)))
    assert abs(r[0] / want - 1.) < 1e-14 and 1. < r[0] < 2. and abs(m[0] / (4. * np.pi / 3. * 5. * want ** 3) - 1.) < 1e-14
    assert 2. < r[4] < 4. and np.all(np.isnan(r[1:4])) and np.all(np.isnan(m[1:4]))
    sr, sm, ss = pf.so_statement(e, enclosed[:, 0], np.diff(enclosed, axis=1), 1., 1., 5.)
    np.testing.assert_array_equal(ss, st)
    np.testing.assert_allclose(r, sr, rtol=1e-12)
    # an edge of 0 carries no density: a particle on the centre does not make the halo "above" there
    r, m, st = halos.so_from_enclosed([0., 1., 2.], [[1, 50, 60], [1, 1, 1]], 1., 1., 5.)
    np.testing.assert_array_equal(st, [0, 1])
    # rho_ref and the profile members
    p = halos.HaloProfiles(e, [50], [[10, 1]], 2.)
    np.testing.assert_array_equal(p.enclosed, [[50, 60, 61]])
    np.testing.assert_allclose(p.enclosed_density, 2. * np.array([[50, 60, 61]]) / v[None, :], rtol=1e-15)
    np.testing.assert_allclose(p.density, 2. * np.array([[10, 1]]) / np.diff(v)[None, :], rtol=1e-15)
    np.testing.assert_array_equal(p.r, [1.5, 3.])


def test_aperture_case():
    case = pc.all_cases()[pc.index_of("8 apertures")]
    ref = pc.aperture_reference(pc.index_of("8 apertures"))
    d2 = _d2(case, 1)
    assert np.count_nonzero(d2 == case["r2"][1]) == 1 and np.count_nonzero(_d2(case, 0) == 0.) == 1
    assert ref["count"][0] == 0 and np.all(np.isnan(ref["com"][0])) and np.isnan(ref["sigma_v"][0])
    assert ref["count"][1] == np.count_nonzero(d2 < case["r2"][1]) >= 2 and np.all(ref["count"][1:] >= 2)
    # the cancellation: sum v.v / m is 1.4e7, sigma_v^2 some 25: six digits are lost
    assert np.all(ref["svv"][1:] > 1.3e7) and np.all(ref["sigma_v"][1:] > 0.) and np.all(np.abs(ref["sigma_v"][3:] - 5.) < 2.)
    L = np.array(case["L"])
    assert np.all(np.abs(min_image(ref["com"][1:] - wrap(case["centres"][1:], L), L)) < 1.)
    assert pf.fx_bits(605 * 8.) == 93 - 13 and pf.fx_bits(0.) == 93
