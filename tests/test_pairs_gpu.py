"""GPU: pair counts (fb_pairs.hip, fastbox_amd.halos.pair_counts) on the constructed cases of tests/pairs_cases.py in both plan
precisions: the counts are exactly those of the numpy statement tests/pairs_numpy.py.  What each case is for is asserted on
the CPU by tests/test_pairs_cases_cpu.py.  The largest input is the 7,000 points of the cuboid box."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo
from fastbox_amd.halos import ColaParticles, FoFHalos, PairCounts
from tests import fof_cases as fc
from tests import pairs_cases as pc
from tests import pairs_numpy as pn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
NCASES = len(pc.NAMES)


@functools.lru_cache(maxsize=None)
def _box(L, prec, N=16):
    scale = L[0] if L[0] == L[1] == L[2] else tuple(L)
    box = CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, realise_now=False, precision=prec, rng="device", seed=7)
    assert (box.Lx, box.Ly, box.Lz) == tuple(L)
    return box


def _count(case, prec, kw, swap=False):
    a, b = case["first"], case["second"]
    if swap:
        a, b = b, a
    return _box(case["L"], prec).pair_counts(a, second=b, edges=case["edges"], **kw)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("index", range(NCASES), ids=pc.NAMES)
def test_constructed_cases_equal_the_reference(index, prec):
    case, ref = pc.reference(index)
    n1 = case["first"].shape[0]
    auto = case["second"] is None
    got = {}
    for kw, want in zip(case["runs"], ref):
        p = _count(case, prec, kw)
        assert isinstance(p, PairCounts) and p.npairs.dtype == np.int64 and p.auto == auto and p.n1 == n1
        print("%s %s: %d pairs in the bins" % (case["name"], kw["mode"], p.npairs.sum()))
        np.testing.assert_array_equal(p.npairs, want)
        np.testing.assert_array_equal(p.edges, case["edges"])
        assert np.all(np.isfinite(p.xi)) and p.xi.shape == p.npairs.shape and np.all(p.rr > 0.)
        if auto:
            assert np.all(p.npairs % 2 == 0) and p.npairs.sum() <= n1 * (n1 - 1)
        got[kw["mode"]] = p
    if '2d' in got:
        np.testing.assert_array_equal(got['2d'].npairs.sum(axis=1), got['1d'].npairs)
    if 'projected' in got:
        assert got['projected'].wp.shape == got['1d'].npairs.shape and np.all(np.isfinite(got['projected'].wp))


@pytest.mark.parametrize("prec", PRECS)
def test_same_object_is_auto_and_a_copy_is_cross(prec):
    """edges[0] = 0: the auto-count holds the coincident distinct pairs and no self pair; the same positions as a separate
    array are cross-counts: the n self pairs more, in the first bin."""
    case, ref = pc.reference(pc.index_of("5 coincident e0=0 auto"))
    box, pos = _box(case["L"], prec), case["first"]
    n = pos.shape[0]
    a = box.pair_counts(pos, edges=case["edges"])
    same = box.pair_counts(pos, second=pos, edges=case["edges"])
    copy = box.pair_counts(pos, second=pos.copy(), edges=case["edges"])
    assert a.auto and same.auto and not copy.auto and (copy.n1, copy.n2) == (n, n)
    np.testing.assert_array_equal(a.npairs, ref[0])
    np.testing.assert_array_equal(same.npairs, ref[0])
    np.testing.assert_array_equal(copy.npairs - a.npairs, [n, 0, 0])
    assert abs(a.rr[0] * n / (n - 1.) / copy.rr[0] - 1.) < 1e-14          # P = n (n - 1) against n n


@pytest.mark.parametrize("prec", PRECS)
def test_cross_counts_are_symmetric_in_1d(prec):
    case, ref = pc.reference(pc.index_of("6 unequal 300 x 4096"))
    ab, ba = _count(case, prec, dict(mode='1d')), _count(case, prec, dict(mode='1d'), swap=True)
    assert (ab.n1, ab.n2, ba.n1, ba.n2) == (300, 4096, 4096, 300)
    np.testing.assert_array_equal(ab.npairs, ba.npairs)
    np.testing.assert_array_equal(ab.npairs, ref[0])
    np.testing.assert_array_equal(ab.rr, ba.rr)


@pytest.mark.parametrize("prec", PRECS)
def test_bad_and_tiny_inputs(prec):
    box = _box((32., 32., 32.), prec)
    edges = np.array(pc.OUTSIDE_EDGES)
    good = fc.case_f_outside()["pos"]
    for value in (np.nan, np.inf, 2. ** 52 * 32., -2. ** 52 * 32.):
        pos = good.copy()
        pos[3, 1] = value
        with pytest.raises(ValueError, match="not finite, or too large"):
            box.pair_counts(pos, edges=edges)
        with pytest.raises(ValueError, match="not finite, or too large"):
            box.pair_counts(good, second=pos, edges=edges, mode='2d')
    pos = good.copy()
    pos[3, 1] = 2. ** 51 * 32.                                         # still wraps
    assert box.pair_counts(pos, edges=edges).npairs.sum() > 0
    for n in (0, 1):
        tiny = fc.case_f_tiny(n)["pos"]
        for kw in (dict(mode='1d'), dict(mode='2d', Nmu=4), dict(mode='projected', pimax=3)):
            p = box.pair_counts(tiny, edges=edges, **kw)
            assert p.npairs.sum() == 0 and np.all(np.isnan(p.xi)) and p.npairs.shape[0] == edges.size - 1
            x = box.pair_counts(tiny, second=good, edges=edges, **kw)
            y = box.pair_counts(good, second=tiny, edges=edges, **kw)
            np.testing.assert_array_equal(x.npairs, pn.counts(tiny, good, (32.,) * 3, edges, **kw))
            np.testing.assert_array_equal(y.npairs, pn.counts(good, tiny, (32.,) * 3, edges, **kw))
            assert (n == 0) == bool(np.all(np.isnan(x.xi)))
    empty = np.zeros((0, 3))
    assert box.pair_counts(empty, second=empty.copy(), edges=edges).npairs.sum() == 0


@pytest.mark.parametrize("prec", PRECS)
def test_device_catalogues_count_as_their_host_copies(prec):
    """The ColaParticles of a 16^3 COLA run and the FoFHalos found in it, passed as device objects and as host arrays."""
    box = CosmoBox(cosmo=default_cosmo, box_scale=64., nsamp=16, realise_now=False, precision=prec, rng="device", seed=3)
    _, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    halos = box.find_halos(particles, linking_length=0.4, nmin=2)
    assert isinstance(particles, ColaParticles) and isinstance(halos, FoFHalos) and len(particles) == 4096 and len(halos) >= 2
    hp, hh = np.asarray(particles).copy(), np.asarray(halos).copy()
    edges = np.geomspace(1., 20., 9)
    for kw in (dict(mode='1d'), dict(mode='2d', Nmu=6, poles=(0, 2)), dict(mode='projected', pimax=12)):
        for dev, host in (((particles, None), (hp, None)), ((halos, None), (hh, None)), ((halos, particles), (hh, hp)),
                          ((halos, particles), (halos, hp)), ((particles, halos), (hp, halos))):
            a = box.pair_counts(dev[0], second=dev[1], edges=edges, **kw)
            b = box.pair_counts(host[0], second=host[1], edges=edges, **kw)
            np.testing.assert_array_equal(a.npairs, b.npairs)
            assert (a.npairs.sum() > 0 or (dev[0] is halos and dev[1] is None)) and a.auto == (dev[1] is None)
            np.testing.assert_array_equal(a.xi, b.xi)
        want = pn.counts(hh, hp, (64.,) * 3, edges, **{k: v for k, v in kw.items() if k != 'poles'})
        np.testing.assert_array_equal(box.pair_counts(halos, second=particles, edges=edges, **kw).npairs, want)
    other = _box((64., 64., 64.), prec)
    with pytest.raises(ValueError, match="of this box"):
        other.pair_counts(particles, edges=edges)
    default = box.pair_counts(particles)                                 # 20 logarithmic bins from L / N to L / 8
    assert default.npairs.shape == (20,) and abs(default.edges[0] - 4.) < 1e-12 and abs(default.edges[-1] - 8.) < 1e-12


@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_are_bit_identical(prec):
    case, ref = pc.reference(pc.index_of("2 cuboid blobs"))
    n = case["first"].shape[0]
    for kw in case["runs"]:
        a, b = _count(case, prec, kw), _count(case, prec, kw)
        assert a.npairs.tobytes() == b.npairs.tobytes() and a.xi.tobytes() == b.xi.tobytes()
        assert np.all(a.npairs % 2 == 0) and 0 < a.npairs.sum() <= n * (n - 1)


def test_timings_and_memory_guard(monkeypatch):
    """The stage timings; MemoryError before any kernel when the work memory does not fit (not provoked on the device)."""
    from fastbox_amd import halos
    case, ref = pc.reference(pc.index_of("1 uniform half shell"))
    box = _box(case["L"], "f64")
    t = {}
    p = halos.pair_counts(box, case["first"], edges=case["edges"], timings=t)
    np.testing.assert_array_equal(p.npairs, ref[0])
    assert t["cells"] == (4, 4, 4) and t["bin_ms"] > 0. and t["count_ms"] > 0. and t["count_crowded_ms"] > 0.
    calls = []
    real_call = halos._lib.call
    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 20)
    monkeypatch.setattr(halos._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    with pytest.raises(MemoryError, match="work memory"):
        box.pair_counts(np.zeros((200000, 3)), edges=case["edges"])
    assert calls == []
    monkeypatch.undo()
    n = 1024 ** 3
    assert 28 * n < halos.pair_device_bytes(n, 0, (64, 64, 64)) < 32 * n < 2 * 28 * n < halos.pair_device_bytes(n, n, (64, 64, 64))


@pytest.mark.parametrize("prec", PRECS)
def test_flush_inside_the_sweep_changes_nothing(prec):
    """A workgroup flushes its 32-bit LDS histogram before it has tested 2^31 + 2^14 pairs, which no small input reaches: with
    the threshold lowered to 4096 pair tests every workgroup flushes between its tiles, and the counts are the same."""
    from fastbox_amd import _lib
    try:
        _lib.call("fb_debug_pair_flush", 4096)
        for name in ("1 uniform half shell", "3 crowded L=8 rmax=3.9 auto", "6 unequal 300 x 4096", "2 cuboid blobs"):
            case, ref = pc.reference(pc.index_of(name))
            for kw, want in zip(case["runs"], ref):
                np.testing.assert_array_equal(_count(case, prec, kw).npairs, want)
    finally:
        _lib.call("fb_debug_pair_flush", 0)
