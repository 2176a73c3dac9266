"""CPU: the two numpy statements of the three-point multipole moments (tests/threepoint_numpy.py) agree on every constructed
case of tests/threepoint_cases.py, each case is what it is meant to be, and ``three_point_normalisation`` is its formula."""
import numpy as np
import pytest
from numpy.polynomial import legendre

from fastbox_amd.halos import pair_cells, three_point_normalisation, triplet_edges, triplet_fx_bits
from tests import threepoint_cases as tc
from tests import threepoint_numpy as tn
from tests.fof_numpy import wrap

NCASES = len(tc.NAMES)
# The issue's bound: the two statements differ by rounding only, measured at 1.1e-16 T; a margin of about a thousand covers
# the growth with neighbour count and l, and a missing m-term or a sign error moves the l >= 1 rows by far more.
GAP_BOUND = 1e-13


@pytest.mark.parametrize("index", range(NCASES), ids=tc.NAMES)
def test_statements_agree(index):
    ref, M = tc.reference(index), tc.legendre(index)
    g = tn.gap(ref, M)
    print("%s: largest gap g = %.3e T" % (tc.NAMES[index], g))
    assert g <= GAP_BOUND
    np.testing.assert_array_equal(ref["M"], np.swapaxes(ref["M"], 1, 2))        # symmetric in the bins
    assert ref["npairs"].sum() % 2 == 0                                         # ordered pairs


def _cells(case):
    return pair_cells(case["L"], (case["edges"][-1],) * 3, max(case["pos"].shape[0], 1))


def test_triangle():
    case, ref = tc.all_cases()[0], tc.reference(0)
    want = np.zeros((11, 2, 2))
    want[:, 0, 1] = want[:, 1, 0] = legendre.legvander(np.array([tc.COS_THETA]), 10)[0]
    assert np.abs(ref["M"] - want).max() < 1e-14
    np.testing.assert_array_equal(ref["N"], [[1, 1], [1, 0], [0, 1]])


def test_seam():
    case, ref = tc.all_cases()[1], tc.reference(1)
    h = case["half"]
    assert ref["alm"][:h].tobytes() == ref["alm"][h:].tobytes() and ref["N"].sum() > 0      # exact differences: the same bits
    w = wrap(case["pos"], np.array(case["L"]))
    nc = _cells(case)
    cell = np.floor(w / (np.array(case["L"]) / nc)).astype(int)
    assert len({tuple(c) for c in cell[:h]}) == 1 and len({tuple(c) for c in cell[h:]}) == 8   # across the corner: 8 cells
    assert np.any(cell[h:] == nc[0] - 1) and np.any(cell[h:] == 0)


def test_two_cells_and_lattice():
    assert _cells(tc.all_cases()[2]) == (2, 2, 2) and _cells(tc.all_cases()[3]) == (2, 2, 2)
    ref = tc.reference(3)
    # 6 neighbours at d^2 = 1 (on the first edge) and 12 at 2; 8 at 3; 6 at 4 (on an edge), 24 at 5, 24 at 6
    assert np.all(ref["N"] == [18, 8, 54])
    T = ref["T"]
    # odd l: the lattice is its own mirror image, so every a_lm vanishes and with it every moment but the j = k terms that
    # the diagonal subtracts, -sum_i S_i(b) = -216 N(b) (an antipodal pair gives P_l(-1) = -1)
    assert np.abs(ref["alm"][:, [1, 2, 3, 9, 12, 15, 25, 30, 35], :]).max() <= 1e-13 * 54
    assert np.abs(ref["M"][1::2] + 216. * np.diag([18., 8., 54.])[None]).max() <= 1e-13 * T.max()
    N = np.array([18., 8., 54.])
    assert np.abs(ref["M"][0] - 216. * (np.outer(N, N) - np.diag(N))).max() <= 1e-13 * T.max()


def test_crowded():
    case, ref = tc.all_cases()[4], tc.reference(4)
    assert _cells(case) == case["cells"]
    np.testing.assert_array_equal(ref["N"][case["centres"]].sum(axis=1), tc.CROWD)
    w = wrap(case["pos"], np.array(case["L"]))
    cell = np.floor(w / (40. / 12.)).astype(int)
    assert np.count_nonzero(np.all(cell == case["crowded_cell"], axis=1)) == 1100
    assert ref["N"][-1].sum() > 0


def test_coincident_and_lonely():
    case, ref = tc.all_cases()[5], tc.reference(5)
    single = tn.alm_statement(case["pos"][:40], None, case["L"], case["edges"], case["lmax"])
    # a twin is no neighbour of its twin, and both see the same third parties
    assert ref["alm"][:10].tobytes() == ref["alm"][40:].tobytes()
    # a third party counts both twins: every pair of the single catalogue that involves one of the first ten is doubled
    assert ref["npairs"].sum() > single["npairs"].sum()
    np.testing.assert_array_equal(ref["N"][:10], ref["N"][40:])
    case, ref = tc.all_cases()[6], tc.reference(6)
    assert ref["N"][20].sum() == 0 and np.all(ref["alm"][20] == 0.) and ref["N"][:20].sum() > 0


def test_sizes_of_the_large_cases():
    c8, c9, c10 = (tc.all_cases()[i] for i in (7, 8, 9))
    assert c8["pos"].shape == (400, 3) and c8["lmax"] == 10 and c8["edges"].size == 21 and c8["weights"].min() < 0. < c8["weights"].max()
    assert c9["lmax"] == 0 and c9["edges"].size == 2
    assert c10["pos"].shape == (1500, 3) and abs(c10["weights"].sum()) < 1e-12


def test_normalisation_is_its_formula():
    e, L = np.array([2., 5., 9.]), (100., 120., 150.)
    vol, norm = three_point_normalisation(e, L, 1000.)
    for b in range(2):
        assert abs(vol[b] / (4. * np.pi / 3. * (e[b + 1] ** 3 - e[b] ** 3)) - 1.) < 1e-15
    V = 100. * 120. * 150.
    for b1 in range(2):
        for b2 in range(2):
            assert abs(norm[b1, b2] / (1000. ** 3 / V ** 2 * vol[b1] * vol[b2]) - 1.) < 1e-15
    assert norm.shape == (2, 2)


def test_argument_checks_and_fixed_point_bits():
    for bad in ([0., 1.], [2., 1.], [1., 1.], [1., 5.], [1., np.nan], np.linspace(0.1, 4., 34)):
        with pytest.raises(ValueError, match="edges"):
            triplet_edges((10., 10., 10.), bad)
    for lmax in (11, -1, 2.5):
        with pytest.raises(ValueError, match="lmax"):
            triplet_edges((10., 10., 10.), [1., 2.], lmax)
    assert triplet_edges((10., 10., 10.), [1., 2.], 10)[1] == 10
    # 2 n wmax = 800 < 2^10, n wmax^2 = 400 < 2^9, 4 (n wmax)^3 = 2.56e8 < 2^28
    assert triplet_fx_bits(400, 1.) == (83, 84, 65)
