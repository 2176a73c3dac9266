"""GPU: three-point multipole moments (fb_triplets.hip; fastbox_amd.halos.triplet_multipoles, three_point) on the constructed
cases of tests/threepoint_cases.py in both plan precisions: the pair counts are exactly those of the numpy statement
tests/threepoint_numpy.py, the probed a_lm and the moments M agree with it within ``tol`` (below) and the fixed-point step,
and a second call and a random permutation of the input give the same bits.  What each case is for is asserted on the CPU by
tests/test_threepoint_cases_cpu.py.  The largest input is the 3,606 points of the crowded case."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, halos
from fastbox_amd.halos import FoFHalos, HaloCatalogue, ThreePoint
from tests import threepoint_cases as tc
from tests import threepoint_numpy as tn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
NCASES = len(tc.NAMES)
TOL_MAX = 1e-11                          # a tolerance above this would make the comparison vacuous


@functools.lru_cache(maxsize=None)
def _box(L, prec, N=16):
    scale = L[0] if L[0] == L[1] == L[2] else tuple(L)
    box = CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, realise_now=False, precision=prec, rng="device", seed=7)
    assert (box.Lx, box.Ly, box.Lz) == tuple(L)
    return box


@functools.lru_cache(maxsize=None)
def _tol():
    """64 x the largest gap g between the two numpy statements over the cases, floored at 64 x 2^-53: the device differs from
    the statement only by the fixed-point quantisation (added where it is used) and, at worst, by last-bit differences in
    sqrt and division that propagate through l <= 10."""
    g = tc.largest_gap()
    tol = max(64. * g, 64. * 2. ** -53)
    print("largest CPU gap g = %.3e, tol = %.3e" % (g, tol))
    assert tol <= TOL_MAX
    return tol


def _check(case, ref, M, npairs, alm):
    n = case["pos"].shape[0]
    wmax = 1. if case["weights"] is None else float(np.abs(case["weights"]).max())
    Fa, _, Fm = halos.triplet_fx_bits(n, wmax)
    tol = _tol()
    np.testing.assert_array_equal(npairs, ref["npairs"])
    # every term enters its sum rounded to a multiple of 2^-F: N terms of an a_lm, n terms of M
    errM = np.abs(M - ref["M"])
    boundM = tol * ref["T"][None] + n * 2. ** -Fm
    pr = case["probe"]
    erra = np.abs(alm - ref["alm"][pr])
    bounda = tol * ref["A"][pr][:, None, :] + ref["N"][pr][:, None, :] * 2. ** -Fa
    relM = (errM / np.where(ref["T"] > 0., ref["T"], 1.)[None]).max()
    rela = (erra / np.where(ref["A"][pr] > 0., ref["A"][pr], 1.)[:, None, :]).max()
    print("%s: device error of M %.3e T, of a_lm %.3e A (tol %.3e, F_a = %d, F_M = %d)" % (case["name"], relM, rela, tol, Fa, Fm))
    assert np.all(errM <= boundM)
    assert np.all(erra <= bounda)
    np.testing.assert_array_equal(M, np.swapaxes(M, 1, 2))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("index", range(NCASES), ids=tc.NAMES)
def test_moments_equal_the_statement_and_repeat(index, prec):
    case, ref = tc.all_cases()[index], tc.reference(index)
    box = _box(case["L"], prec)
    kw = dict(lmax=case["lmax"], weights=case["weights"])
    M, npairs, alm = box.triplet_multipoles(case["pos"], case["edges"], probe=case["probe"], **kw)
    nr = case["edges"].size - 1
    assert M.shape == (case["lmax"] + 1, nr, nr) and npairs.dtype == np.int64 and alm.shape == (case["probe"].size, (case["lmax"] + 1) ** 2, nr)
    _check(case, ref, M, npairs, alm)
    # a second call, and the particles in another order: the same bits, for M and for the same particles' a_lm
    M2, npairs2, alm2 = box.triplet_multipoles(case["pos"], case["edges"], probe=case["probe"], **kw)
    assert M2.tobytes() == M.tobytes() and alm2.tobytes() == alm.tobytes() and np.array_equal(npairs2, npairs)
    order = np.random.RandomState(index).permutation(case["pos"].shape[0])
    where = np.argsort(order)                                   # particle i of the case is particle where[i] of the shuffled input
    w = None if case["weights"] is None else case["weights"][order]
    M3, npairs3, alm3 = box.triplet_multipoles(case["pos"][order], case["edges"], lmax=case["lmax"], weights=w, probe=where[case["probe"]])
    assert M3.tobytes() == M.tobytes() and alm3.tobytes() == alm.tobytes() and np.array_equal(npairs3, npairs)
    # the existing pair counts see the same pairs
    np.testing.assert_array_equal(box.pair_counts(case["pos"], edges=case["edges"]).npairs, npairs)
    if case["name"] == "1 triangle":
        want = np.zeros_like(M)
        want[:, 0, 1] = want[:, 1, 0] = np.polynomial.legendre.legvander(np.array([tc.COS_THETA]), 10)[0]
        assert np.abs(M - want).max() < 1e-13
    if case["name"] == "2 seam":
        assert alm[:2].tobytes() == alm[2:].tobytes()           # particles 0, 5 and their copies across the corner
    if case["name"] == "4 lattice on edges":
        T = ref["T"]
        assert np.abs(M[1::2] + 216. * np.diag([18., 8., 54.])[None]).max() <= _tol() * T.max() + 216 * 2. ** -halos.triplet_fx_bits(216)[2]
        np.testing.assert_array_equal(npairs, 216 * np.array([18, 8, 54]))
    if "crowded" in case["name"]:
        t = {}
        box.triplet_multipoles(case["pos"], case["edges"], lmax=case["lmax"], timings=t)
        assert t["cells"] == case["cells"] and t["bin_ms"] > 0. and t["sweep_ms"] > 0. and t["finish_ms"] > 0.
    if case["name"] == "7 lonely primary":
        assert np.all(alm[0] == 0.) and np.any(alm[1] != 0.)


@pytest.mark.parametrize("prec", PRECS)
def test_empty_catalogues(prec):
    box = _box((20., 20., 20.), prec)
    for pos in (np.zeros((0, 3)), np.array([[1., 2., 3.]])):
        M, npairs, alm = box.triplet_multipoles(pos, [0.5, 1.5, 3.], lmax=3, probe=[0] if len(pos) else None)
        assert M.shape == (4, 2, 2) and np.all(M == 0.) and np.all(npairs == 0) and (alm is None or np.all(alm == 0.))
    tp = box.three_point(np.zeros((0, 3)), [0.5, 1.5, 3.], lmax=2)
    assert isinstance(tp, ThreePoint) and tp.n_data == 0 and np.all(tp.multipoles == 0.)


@pytest.mark.parametrize("prec", PRECS)
def test_three_point_with_randoms_is_the_statement_on_the_joined_catalogue(prec):
    index = tc.index_of("10 D - R")
    case, ref = tc.all_cases()[index], tc.reference(index)
    box = _box(case["L"], prec)
    nd = case["n_data"]
    tp = box.three_point(case["pos"][:nd], case["edges"], lmax=case["lmax"], randoms=tc.DR_PER_DATUM, seed=tc.DR_SEED)
    assert isinstance(tp, ThreePoint) and tp.connected and (tp.n_data, tp.n_random, tp.lmax) == (nd, tc.DR_PER_DATUM * nd, case["lmax"])
    # the joined, weighted catalogue, read back: the data, then the drawn randoms with weight -W_d / n_r
    np.testing.assert_array_equal(np.asarray(tp.catalogue), case["pos"])
    np.testing.assert_array_equal(tp.weights, case["weights"])
    np.testing.assert_array_equal(tp.npairs, ref["npairs"])
    vol, norm = halos.three_point_normalisation(case["edges"], case["L"], float(nd))
    pref = (2. * np.arange(case["lmax"] + 1) + 1.)[:, None, None] / norm[None]
    Fm = halos.triplet_fx_bits(case["pos"].shape[0], 1.)[2]
    err = np.abs(tp.zeta - pref * ref["M"])
    print("D - R: largest error of zeta %.3e of %.3e" % (err.max(), np.abs(tp.zeta).max()))
    assert np.all(err <= pref * (_tol() * ref["T"][None] + 1500 * 2. ** -Fm) + 4. * np.spacing(np.abs(tp.zeta)))
    np.testing.assert_array_equal(tp.volumes, vol)
    np.testing.assert_array_equal(tp.edges, case["edges"])
    # device catalogues and explicit randoms give the same bits; without randoms zeta is the full function
    rand = box.uniform_catalogue(tc.DR_PER_DATUM * nd, seed=tc.DR_SEED)
    data = HaloCatalogue(box.engine, box.engine.upload_raw(case["pos"][:nd]), nd)
    again = box.three_point(data, case["edges"], lmax=case["lmax"], randoms=rand)
    assert again.zeta.tobytes() == tp.zeta.tobytes()
    full = box.three_point(data, case["edges"], lmax=case["lmax"])
    assert not full.connected and full.n_random == 0 and full.zeta.shape == tp.zeta.shape
    Md = box.triplet_multipoles(case["pos"][:nd], case["edges"], lmax=case["lmax"])[0]
    np.testing.assert_array_equal(full.multipoles, Md)
    np.testing.assert_allclose(full.zeta[0] + 1., Md[0] / norm, rtol=1e-14)


@pytest.mark.parametrize("prec", PRECS)
def test_catalogue_objects(prec):
    """The FoFHalos of a 16^3 COLA run go where a host array goes."""
    box = CosmoBox(cosmo=default_cosmo, box_scale=64., nsamp=16, realise_now=False, precision=prec, rng="device", seed=3)
    _, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    fof = box.find_halos(particles, linking_length=0.4, nmin=2)
    assert isinstance(fof, FoFHalos) and len(fof) >= 2
    edges = [4., 10., 20.]
    a = box.three_point(fof, edges, lmax=4)
    b = box.three_point(np.asarray(fof).copy(), edges, lmax=4)
    assert a.zeta.tobytes() == b.zeta.tobytes() and a.n_data == len(fof)
    p = box.three_point(particles, edges, lmax=2, randoms=1, seed=5)
    assert p.connected and p.n_random == 4096 and np.all(np.isfinite(p.zeta))
    other = _box((64., 64., 64.), prec)
    with pytest.raises(ValueError, match="of this box"):
        other.three_point(fof, edges)


def test_bad_arguments_raise_before_the_device(monkeypatch):
    box = _box((20., 20., 20.), "f64")
    good = np.random.RandomState(1).uniform(0., 20., (50, 3))
    calls = []
    real_call = halos._lib.call
    monkeypatch.setattr(halos._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for edges in ([0., 1., 2.], [1., 3., 2.], [1., 10.], np.linspace(0.1, 4., 34)):       # e_0 = 0, unsorted, >= L / 2, nr = 33
        with pytest.raises(ValueError, match="edges"):
            box.triplet_multipoles(good, edges)
        with pytest.raises(ValueError, match="edges"):
            box.three_point(good, edges)
    with pytest.raises(ValueError, match="lmax"):
        box.triplet_multipoles(good, [1., 2.], lmax=11)
    for value in (np.nan, np.inf):
        pos, w = good.copy(), np.ones(50)
        pos[3, 1] = value
        w[7] = value
        with pytest.raises(ValueError, match="not finite"):
            box.triplet_multipoles(pos, [1., 2.])
        with pytest.raises(ValueError, match="not finite"):
            box.triplet_multipoles(good, [1., 2.], weights=w)
        with pytest.raises(ValueError, match="not finite|finite"):
            box.three_point(good, [1., 2.], weights=w)
    with pytest.raises(ValueError, match="weights"):
        box.triplet_multipoles(good, [1., 2.], weights=np.ones(49))
    with pytest.raises(ValueError, match="probe"):
        box.triplet_multipoles(good, [1., 2.], probe=[50])
    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 20)
    with pytest.raises(MemoryError, match="work memory"):
        box.triplet_multipoles(np.zeros((200000, 3)), [1., 2.])
    assert calls == []
    monkeypatch.undo()
    # a device catalogue is checked on the device
    bad = good.copy()
    bad[3, 1] = np.nan
    cat = HaloCatalogue(box.engine, box.engine.upload_raw(bad), 50)
    with pytest.raises(ValueError, match="not finite, or too large"):
        box.triplet_multipoles(cat, [1., 2.])
    n = 1024 ** 3
    plain = halos.triplet_device_bytes(n, (64, 64, 64), 10, 10)
    assert 32 * n < plain < 33 * n and 48 * n < halos.triplet_device_bytes(n, (64, 64, 64), 10, 10, weighted=True) < 49 * n
