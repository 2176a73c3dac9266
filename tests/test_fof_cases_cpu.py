"""CPU: the constructed friends-of-friends cases of tests/fof_cases.py are what they claim to be -- the two statements of the
definition (tests/fof_numpy.py) agree on each, no random case has a pair near the linking length, and each case holds the
feature it was built for (ties in count, groups across the seam, a cell above one LDS tile, exact ties, a single long chain)."""
import numpy as np
import pytest

from fastbox_amd import halos
from tests import fof_cases as fc
from tests import fof_numpy as fn

CASES = fc.all_cases()


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_loop_and_tree_agree_and_no_near_tie(index):
    case = CASES[index]
    ell = fc.length(case)
    loop, tie = fn.groups_loop(case["pos"], case["L"], ell)
    tree = fn.groups_tree(case["pos"], case["L"], ell)
    print("%s: n = %d, l = %.6g, %d groups, nearest tie %.3g" % (case["name"], loop.size, ell, np.unique(loop).size, tie))
    if case["name"].startswith("D ties ell=1.0") and case["ell"] == 1.0:
        assert tie == 0.                                        # the pair at exactly l: only the loop is the definition
        assert np.unique(loop).size == 2 and np.unique(tree).size == 1
    else:
        np.testing.assert_array_equal(loop, tree)
    if case["random"]:
        assert tie >= 1e-9
    np.testing.assert_array_equal(fc.exact_roots(case), loop)


def test_case_a_has_many_groups_and_ties_in_count():
    case, cat = fc.reference(0)
    assert cat["count"].size >= 50 and cat["count"].min() >= 5
    assert np.unique(cat["count"]).size < cat["count"].size           # ties: ordered by root
    same = cat["count"][1:] == cat["count"][:-1]
    assert np.all(cat["roots"][1:][same] > cat["roots"][:-1][same])


def test_case_b_crosses_the_seam_and_overfills_a_tile():
    case, cat = fc.reference(1)
    assert cat["count"].size >= 12 and cat["count"][0] > 300
    assert fc.seam_groups(case, cat) >= 8
    L, n = case["L"], case["pos"].shape[0]
    cells = halos.fof_cells(L, case["ell"], n)
    assert min(cells) >= 3                                             # the half shell of 13 neighbours
    w = fn.wrap(case["pos"], np.array(L))
    idx = np.minimum((w * (np.array(cells) / np.array(L))).astype(int), np.array(cells) - 1)
    occ = np.bincount((idx[:, 0] * cells[1] + idx[:, 1]) * cells[2] + idx[:, 2])
    assert occ.max() > 2 * halos.FOF_TILE                              # home tiles beyond the first, neighbour tiles too
    assert np.any(case["pos"] < 0.) and np.any(case["pos"] >= np.array(L))    # wrapped on read


def test_case_c_cells_and_limits():
    for ell, nc in ((2.5, 3), (3.9, 2)):
        assert halos.fof_cells((8., 8., 8.), ell, 12) == (nc,) * 3
        assert halos.fof_linking_length((8., 8., 8.), 12, ell, absolute=True) == ell
    for ell in (4.0, 0., -1., np.nan, 5.):
        with pytest.raises(ValueError, match="linking length"):
            halos.fof_linking_length((8., 8., 8.), 12, ell, absolute=True)
    _, c25 = fc.reference(2)
    _, c39 = fc.reference(3)
    assert c25["n_groups_all"] > 1 and c25["count"][0] >= 2 and c39["n_groups_all"] == 1


def test_case_d_exact_ties():
    case, cat = fc.reference(4)
    np.testing.assert_array_equal(cat["roots"], [0, 20])
    np.testing.assert_array_equal(cat["count"], [20, 20])
    w = case["pos"][:, 0]
    assert w.min() < 4. and w.max() > 60.                              # the chain crosses the seam
    _, one = fc.reference(5)
    np.testing.assert_array_equal(one["roots"], [0])


@pytest.mark.parametrize("index", [6, 7, 8])
def test_case_e_is_one_chain(index):
    case, cat = fc.reference(index)
    np.testing.assert_array_equal(cat["count"], [8192])
    np.testing.assert_array_equal(cat["roots"], [0])
    step = np.linalg.norm(np.diff(fc.case_e("index")["pos"][:400], axis=0), axis=1)
    assert np.all(np.abs(step / 0.25 - 0.6) < 0.01)


def test_case_f_degenerate():
    _, co = fc.reference(9)
    np.testing.assert_array_equal(co["labels"], [0, -1, 0, -1])
    case, out = fc.reference(10)
    np.testing.assert_array_equal(out["labels"], [0, 0, 0, 0, 1, 1, 1, 1, -1])
    assert np.all(out["position"] >= 0.) and np.all(out["position"] < 32.)
    assert fn.wrap(-1e-20, 32.) == 0. and fn.wrap(32., 32.) == 0. and fn.wrap(-0.1, 32.) == 32. - 0.1
    for n in (0, 1):
        t = fc.case_f_tiny(n)
        roots = fn.groups_loop(t["pos"], t["L"], t["ell"])[0]
        cat = fn.catalogue(t["pos"], None, roots, t["L"], 2)
        assert cat["count"].size == 0 and cat["velocity"] is None and cat["labels"].size == n


def test_default_particle_mass_convention():
    """Lengths are Mpc (not Mpc/h) throughout the package, so rho_crit = 2.77536627e11 h^2 Msun / Mpc^3 gives Msun."""
    from fastbox_amd import default_cosmo
    h, om = default_cosmo['h'], default_cosmo['Omega_c'] + default_cosmo['Omega_b']
    # 3 H0^2 / (8 pi G) with H0 = 100 h km/s/Mpc, G = 4.30091e-9 Mpc (km/s)^2 / Msun
    rho = 3. * (100. * h) ** 2 / (8. * np.pi * 4.30091e-9)
    assert abs(rho / (halos.RHO_CRIT * h * h) - 1.) < 1e-4 and 0.2 < om < 0.4


def test_case_g_three_pairs_in_the_corner_cells():
    """The case of the raw link call on 128 x 128 x 64 cells: a pair in cell 0, a pair in the last cell, a pair through the
    periodic corner between those two cells, everything else single; cells no smaller than the linking length."""
    pos, L, ell, roots = fc.case_g_many_cells()
    n, cells = pos.shape[0], np.array(fc.G_CELLS)
    assert n == 300 and np.all(np.array(L) / cells >= ell) and ell > 0.999 / 128.
    assert cells.prod() + 1 == 256 * 4096 + 1                            # the scan's outputs: one past 256 chunks
    np.testing.assert_array_equal(roots, fn.groups_tree(pos, L, ell))
    np.testing.assert_array_equal(roots[:6], [0, 0, 2, 2, 4, 4])
    np.testing.assert_array_equal(roots[6:], np.arange(6, n))
    assert fn.groups_loop(pos, L, ell)[1] >= 1e-3                         # no pair near the linking length
    idx = np.minimum((fn.wrap(pos, np.array(L)) * cells).astype(int), cells - 1)
    cell = (idx[:, 0] * cells[1] + idx[:, 1]) * cells[2] + idx[:, 2]
    np.testing.assert_array_equal(cell[:6], [0, 0, cells.prod() - 1, cells.prod() - 1, 0, cells.prod() - 1])
    assert np.unique(cell[6:]).size > 250 and cell[6:].min() > 0 and cell[6:].max() < cells.prod() - 1
