"""CPU: the pair-count reference (tests/pairs_numpy.py) is validated against scipy's periodic tree on the random cases, each
constructed case of tests/pairs_cases.py holds the feature it was built for (cells per axis, pairs exactly on an edge, a
crowded cell, coincident points), PairCounts derives rr, xi, poles and wp from given counts by the formulas of DESIGN.md
section 4, and pair_counts refuses bad arguments before it touches a device."""
import types

import numpy as np
import pytest

from fastbox_amd import halos
from tests import fof_cases as fc
from tests import pairs_cases as pc
from tests import pairs_numpy as pn

CASES = pc.all_cases()
RANDOM = [i for i, c in enumerate(CASES) if c["random"]]


def _cells(case, kw):
    e, nsub, sub_max, reach = halos.pair_setup(case["L"], 16, case["edges"], **kw)
    n = max(case["first"].shape[0], 0 if case["second"] is None else case["second"].shape[0])
    return halos.pair_cells(case["L"], reach, n)


@pytest.mark.parametrize("index", RANDOM, ids=[pc.NAMES[i] for i in RANDOM])
def test_brute_force_equals_the_tree_where_no_pair_is_near_an_edge(index):
    case, ref = pc.reference(index)
    near, ties = pn.edge_distances(case["first"], case["second"], case["L"], case["edges"])
    print("%s: nearest pair to an edge %.3g Mpc" % (case["name"], near))
    assert near >= 1e-9 and ties == 0                                   # so the two statements cannot legitimately differ
    one_d = ref[[kw["mode"] for kw in case["runs"]].index('1d')]
    np.testing.assert_array_equal(one_d, pn.tree_counts(case["first"], case["second"], case["L"], case["edges"]))
    assert one_d.sum() > 0


@pytest.mark.parametrize("index", range(len(CASES)), ids=pc.NAMES)
def test_sub_bins_sum_to_the_radial_counts_and_auto_counts_are_even(index):
    case, ref = pc.reference(index)
    modes = [kw["mode"] for kw in case["runs"]]
    one_d = ref[modes.index('1d')]
    if '2d' in modes:
        np.testing.assert_array_equal(ref[modes.index('2d')].sum(axis=1), one_d)
    n1 = case["first"].shape[0]
    if case["second"] is None:
        assert all(np.all(c % 2 == 0) for c in ref) and one_d.sum() <= n1 * (n1 - 1)
    else:
        assert one_d.sum() <= n1 * case["second"].shape[0]


def test_case_1_takes_the_half_shell_with_one_and_two_home_tiles():
    case = CASES[pc.index_of("1 uniform half shell")]
    for kw in case["runs"]:
        cells = _cells(case, kw)
        assert min(cells) >= 3                                          # the half shell of 13 neighbours
        occ = pn.cells_of(case["first"], case["L"], cells)
        assert occ.max() > halos.FOF_TILE > occ.min()                   # cells of one home tile and cells of two
    assert _cells(case, case["runs"][0]) == (4, 4, 4)


def test_case_2_crosses_the_seam_and_overfills_a_tile():
    case = CASES[pc.index_of("2 cuboid blobs")]
    cells = _cells(case, case["runs"][0])
    assert cells == (6, 9, 12)
    occ = pn.cells_of(case["first"], case["L"], cells)
    assert occ.max() > 256 + halos.FOF_TILE                             # more than one neighbour tile, several home tiles
    assert np.any(case["first"] < 0.) and np.any(case["first"] >= np.array(case["L"]))      # wrapped on read


def test_case_3_cells_per_axis():
    want = {("3 L=8.0 rmax=3.9", '1d'): (2, 2, 2), ("3 L=8.0 rmax=2.5", '1d'): (3, 3, 3), ("3 L=(8.0, 12.0, 40.0) rmax=3.9", '1d'): (2, 3, 4),
            ("3 L=8.0 rmax=3.9", 'projected'): (2, 2, 2), ("3 L=8.0 rmax=2.5", 'projected'): (3, 3, 2),
            ("3 L=(8.0, 12.0, 40.0) rmax=3.9", 'projected'): (2, 3, 4)}
    seen = 0
    for case in CASES:
        for (prefix, mode), cells in want.items():
            if case["name"].startswith(prefix + " "):
                kw = [k for k in case["runs"] if k["mode"] == mode][0]
                assert _cells(case, kw) == cells, (case["name"], mode)
                seen += 1
    assert seen == 12                                                   # auto and cross of each
    assert 40. / 3.9 > 10                                               # 4 cells along z there is the cap, not the reach
    crowded = CASES[pc.index_of("3 crowded L=8 rmax=3.9 auto")]
    assert _cells(crowded, crowded["runs"][0]) == (2, 2, 2)
    occ = pn.cells_of(crowded["first"], crowded["L"], (2, 2, 2))
    assert occ.min() > halos.FOF_TILE and occ.max() < 2 * halos.FOF_TILE    # a second home tile, shorter than the cell, in each
    # with 2 cells on an axis a pair is met through one image only: the far image is beyond L / 2 > rmax
    case, ref = pc.reference(pc.index_of("3 L=8.0 rmax=3.9 auto"))
    assert ref[0].sum() > 0.3 * 200 * 199


def test_case_4_exact_ties():
    case, ref = pc.reference(pc.index_of("4 lattice auto"))
    near, ties = pn.edge_distances(case["first"], None, case["L"], case["edges"])
    assert near == 0. and ties > 1000
    # pairs on an edge go to the upper bin: the count of [0.75, 1.0) holds the 0.75 pairs, that of [0, 0.75) does not
    d2 = np.array([a * a + b * b + c * c for a in range(-5, 6) for b in range(-5, 6) for c in range(-5, 6)]) / 16.
    w = np.array([(6 - abs(a)) * (6 - abs(b)) * (6 - abs(c)) for a in range(-5, 6) for b in range(-5, 6) for c in range(-5, 6)])
    e2 = np.array(pc.TIE_EDGES) ** 2
    want = [int(w[(d2 >= lo) & (d2 < hi) & (d2 > 0)].sum()) for lo, hi in zip(e2[:-1], e2[1:])]
    np.testing.assert_array_equal(ref[0], want)
    assert np.any(case["first"] > 7.) and np.any(case["first"] < 1.)                           # across the seam
    case, ref = pc.reference(pc.index_of("4 tie pairs"))
    one_d, two_d, proj = ref
    np.testing.assert_array_equal(one_d, [0, 0, 0, 4])                  # both pairs have d = 1.25 exactly: bin [1.25, 2.0)
    assert two_d[3, 3] == 2 and two_d[3, 4] == 2                        # mu = 0.6 exactly -> m = 3; mu = 0.8 -> m = 4
    assert proj[2, 0] == 2 and proj[1, 1] == 2                          # r_p = 1.0, pi = 0.75; r_p = 0.75, pi = 1.0 -> bin 1


def test_case_5_coincident_points():
    auto0, cross0 = pc.reference(pc.index_of("5 coincident e0=0 auto"))[1], pc.reference(pc.index_of("5 coincident e0=0 cross"))[1]
    auto5, cross5 = pc.reference(pc.index_of("5 coincident e0=0.5 auto"))[1], pc.reference(pc.index_of("5 coincident e0=0.5 cross"))[1]
    n = pc.coincident_positions().shape[0]
    assert n == 61
    p = pc.coincident_positions()
    assert np.count_nonzero(np.all(p[:, None, :] == p[None, :, :], axis=2)) - n == pc.COINCIDENT_ORDERED_PAIRS
    np.testing.assert_array_equal(cross0[0] - auto0[0], [n, 0, 0])      # the copy adds the n self pairs, in the first bin
    np.testing.assert_array_equal(cross5[0], auto5[0])                  # edges[0] > 0: neither coincident nor self pairs
    assert auto0[0][0] - auto5[0][0] >= pc.COINCIDENT_ORDERED_PAIRS     # edges[0] = 0 holds the coincident distinct pairs
    assert auto0[1][0, 9] >= pc.COINCIDENT_ORDERED_PAIRS                # d = 0 lands in the last mu bin
    assert cross0[1][0, 9] - auto0[1][0, 9] == n


def test_case_6_is_symmetric_and_case_7_wraps():
    a, b = pc.reference(pc.index_of("6 unequal 300 x 4096"))[1], pc.reference(pc.index_of("6 unequal 4096 x 300"))[1]
    np.testing.assert_array_equal(a[0], b[0])
    raw, wrapped = pc.reference(pc.index_of("7 outside raw")), pc.reference(pc.index_of("7 outside wrapped"))
    assert np.any(raw[0]["first"] < 0.) and np.any(raw[0]["first"] >= 32.) and np.all(wrapped[0]["first"] >= 0.) \
        and np.all(wrapped[0]["first"] < 32.)
    for x, y in zip(raw[1], wrapped[1]):
        np.testing.assert_array_equal(x, y)
    assert raw[1][0].sum() >= 12                                        # the two clumps across the seam are counted
    for n in (0, 1):
        assert pn.counts(fc.case_f_tiny(n)["pos"], None, (32.,) * 3, pc.OUTSIDE_EDGES).sum() == 0


def test_pair_counts_object_follows_the_formulas():
    rs = np.random.RandomState(5)
    L = (64., 96., 128.)
    V = 64. * 96. * 128.
    e = np.array([0., 0.5, 1.25, 3., 7.])
    nr = 4
    # '1d', auto
    c1 = rs.randint(0, 1000, nr) * 2
    p = halos.PairCounts(e, c1, L, 1000, 1000, True, mode='1d')
    rr = np.array([1000. * 999. * (4. * np.pi / 3.) * (e[b + 1] ** 3 - e[b] ** 3) / V for b in range(nr)])
    np.testing.assert_allclose(p.rr, rr, rtol=1e-14)
    np.testing.assert_allclose(p.xi, c1 / rr - 1., rtol=1e-14)
    np.testing.assert_array_equal(p.r, [0.25, 0.875, 2.125, 5.])
    assert p.npairs.dtype == np.int64 and p.poles == {} and p.wp is None and p.mu_edges is None and p.pi_edges is None
    assert p.auto and p.n1 == 1000
    # '2d', cross, with multipoles
    nmu = 5
    c2 = rs.randint(0, 1000, (nr, nmu))
    p = halos.PairCounts(e, c2, L, 300, 4096, False, mode='2d', poles=(0, 2, 4))
    np.testing.assert_allclose(p.mu_edges, [0., 0.2, 0.4, 0.6, 0.8, 1.], rtol=1e-15)
    rr = np.array([[300. * 4096. * (4. * np.pi / 3.) * (e[b + 1] ** 3 - e[b] ** 3) * 0.2 / V for m in range(nmu)] for b in range(nr)])
    np.testing.assert_allclose(p.rr, rr, rtol=1e-14)
    xi = c2 / rr - 1.
    np.testing.assert_allclose(p.xi, xi, rtol=1e-14)
    mu = np.array([0.1, 0.3, 0.5, 0.7, 0.9])
    leg = {0: np.ones(5), 2: (3. * mu ** 2 - 1.) / 2., 4: (35. * mu ** 4 - 30. * mu ** 2 + 3.) / 8.}
    assert sorted(p.poles) == [0, 2, 4]
    for l in (0, 2, 4):
        want = np.array([(2 * l + 1) * sum(xi[b, m] * leg[l][m] * 0.2 for m in range(nmu)) for b in range(nr)])
        np.testing.assert_allclose(p.poles[l], want, rtol=1e-14)
    # 'projected'
    npi = 3
    c3 = rs.randint(0, 1000, (nr, npi)) * 2
    p = halos.PairCounts(e, c3, L, 500, 500, True, mode='projected')
    np.testing.assert_array_equal(p.pi_edges, [0., 1., 2., 3.])
    rr = np.array([[500. * 499. * np.pi * (e[b + 1] ** 2 - e[b] ** 2) * 2. * 1. / V for q in range(npi)] for b in range(nr)])
    np.testing.assert_allclose(p.rr, rr, rtol=1e-14)
    xi = c3 / rr - 1.
    np.testing.assert_allclose(p.xi, xi, rtol=1e-14)
    np.testing.assert_allclose(p.wp, [2. * sum(xi[b, q] * 1. for q in range(npi)) for b in range(nr)], rtol=1e-14)
    # empty catalogues: zero counts, xi NaN, no error
    for n in (0, 1):
        p = halos.PairCounts(e, np.zeros(nr, dtype=np.int64), L, n, n, True, mode='1d')
        assert np.all(p.rr == 0.) and np.all(np.isnan(p.xi)) and np.all(p.npairs == 0)
    with pytest.raises(ValueError, match="poles"):
        halos.PairCounts(e, c1, L, 10, 10, True, mode='1d', poles=(0,))


def test_arguments_are_checked_before_the_device():
    box = types.SimpleNamespace(engine=None, Lx=8., Ly=12., Lz=40., N=16)
    pos = np.zeros((12, 3))
    ok = [0.5, 1., 2.]
    bad = [dict(edges=[1., 1., 2.]), dict(edges=[2., 1.]), dict(edges=[-0.5, 1.]), dict(edges=[1.]), dict(edges=[[0.5, 1.]]),
           dict(edges=[0.5, np.nan]), dict(edges=[0.5, 4.0]), dict(edges=[0.5, 4.5], mode='2d'),
           dict(edges=[0.5, 4.0], mode='projected', pimax=5), dict(edges=ok, mode='projected'),
           dict(edges=ok, mode='projected', pimax=20), dict(edges=ok, mode='projected', pimax=2.5),
           dict(edges=ok, mode='projected', pimax=0), dict(edges=ok, mode='projected', pimax=-3), dict(edges=ok, mode='angular'),
           dict(edges=ok, mode='1d', poles=(0,)), dict(edges=ok, mode='projected', pimax=3, poles=(0, 2)),
           dict(edges=ok, mode='2d', poles=(1,)), dict(edges=ok, mode='2d', poles=(0, 6)), dict(edges=ok, mode='2d', Nmu=0),
           dict(edges=ok, mode='2d', Nmu=2.5), dict(edges=ok, mode='1d', pimax=3),
           dict(edges=np.linspace(0.1, 3.9, 258)), dict(edges=np.linspace(0.1, 3.9, 201), mode='2d', Nmu=21),
           dict(edges=np.linspace(0.1, 3.9, 201), mode='2d', Nmu=4097)]
    for kw in bad:
        with pytest.raises(ValueError):
            halos.pair_counts(box, pos, **kw)
    with pytest.raises(ValueError, match="at most 4096 bins in total"):
        halos.pair_counts(box, pos, edges=np.linspace(0.1, 3.9, 201), mode='2d', Nmu=21)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        halos.pair_counts(box, np.zeros((12, 2)), edges=ok)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        halos.pair_counts(box, pos, second=np.zeros(5), edges=ok)
    # what is accepted: 200 x 20 = 4000 bins; pimax just below Lz / 2; r_p up to min(Lx, Ly) / 2 only
    e, nsub, sub_max, reach = halos.pair_setup((8., 12., 40.), 16, np.linspace(0.1, 3.9, 201), '2d', 20)
    assert (e.size, nsub) == (201, 20)
    e, nsub, sub_max, reach = halos.pair_setup((8., 12., 40.), 16, ok, 'projected', pimax=19)
    assert (nsub, sub_max, reach) == (19, 19., (2., 2., 19.))
    # the default edges: 20 logarithmic bins from min(L) / N to min(L) / 8
    e = halos.pair_setup((8., 12., 40.), 16)[0]
    assert e.size == 21 and abs(e[0] - 0.5) < 1e-15 and abs(e[-1] - 1.) < 1e-15 and np.allclose(e[1:] / e[:-1], 2. ** 0.05)


def test_library_exports_the_pair_entries():
    from fastbox_amd import _lib
    _lib.build_library()
    lib = _lib.load()
    for name in ("fb_pair_work_bytes", "fb_pair_count", "fb_debug_pair_flush"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    n1, n2, ncells = 1000, 300, 64
    floor = 28 * (n1 + n2) + 2 * 4 * (2 * ncells + 1) + 8 * (n1 // 64) + 8 * 257
    got = lib.fb_pair_work_bytes(n1, n2, ncells)
    assert floor <= got <= floor + 4096
    assert lib.fb_pair_work_bytes(n1, 0, ncells) < got
    assert lib.fb_pair_work_bytes(-1, 0, 1) == -1 and lib.fb_pair_work_bytes(1, -1, 1) == -1 and lib.fb_pair_work_bytes(1, 0, 0) == -1
    assert halos.pair_device_bytes(n1, n2, (4, 4, 4), 20) >= got + 160
    assert lib.fb_debug_pair_flush(-1) != 0 and lib.fb_debug_pair_flush(2 ** 31 + 1) != 0       # at most 2^31: no counter can wrap
    assert lib.fb_debug_pair_flush(2 ** 31) == 0 and lib.fb_debug_pair_flush(0) == 0


def test_default_edges_need_more_than_eight_cells_per_side():
    with pytest.raises(ValueError, match="N > 8"):
        halos.pair_setup((8., 8., 8.), 8)
    assert halos.pair_setup((8., 8., 8.), 9)[0].size == 21
