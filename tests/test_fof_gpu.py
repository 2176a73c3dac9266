"""GPU: friends-of-friends halo finding (fb_fof.hip, fastbox_amd.halos.find_halos_fof) on the constructed cases of
tests/fof_cases.py in both plan precisions, against the host reference tests/fof_numpy.py: group membership, roots, counts
and the number of groups exactly; centres of mass to 1e-10 L and mean velocities to 1e-10 max |v| (the fp64 reference itself
rounds at about 1e-12 L; the device sums are fixed-point).  What each case is for is asserted on the CPU by
tests/test_fof_cases_cpu.py.  The largest input is the 64^3 particles of a COLA run."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, _lib, default_cosmo, halos
from fastbox_amd.halos import FoFHalos, HaloCatalogue
from tests import fof_cases as fc
from tests import fof_numpy as fn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
NCASES = len(fc.all_cases())
IDS = [c["name"] for c in fc.all_cases()]


@functools.lru_cache(maxsize=None)
def _box(L, prec, N=16):
    scale = L[0] if L[0] == L[1] == L[2] else tuple(L)
    box = CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, realise_now=False, precision=prec, rng="device", seed=7)
    assert (box.Lx, box.Ly, box.Lz) == tuple(L)
    return box


def _find(case, prec, **kw):
    return _box(case["L"], prec).find_halos(case["pos"], linking_length=case["ell"], nmin=case["nmin"],
                                            absolute=case["absolute"], velocities=case["vel"], **kw)


def _check(h, case, cat):
    L = np.array(case["L"])
    assert isinstance(h, FoFHalos) and isinstance(h, HaloCatalogue)
    assert h.linking_length == fc.length(case)
    assert h.n_groups_all == cat["n_groups_all"]
    np.testing.assert_array_equal(h.roots, cat["roots"])
    np.testing.assert_array_equal(h.count, cat["count"])
    lab = np.asarray(h.labels)
    assert lab.dtype == np.int32
    np.testing.assert_array_equal(lab, cat["labels"])
    assert len(h) == cat["count"].size and h.mass.shape == h.count.shape
    np.testing.assert_array_equal(h.mass, h.count * h.particle_mass)
    if len(h):
        pos = np.asarray(h)
        assert np.all(pos >= 0.) and np.all(pos < L)
        dpos = np.max(np.abs(fn.min_image(pos - cat["position"], L)) / L)
        print("%s: %d groups kept of %d; centre of mass off by %.3g L" % (case["name"], len(h), h.n_groups_all, dpos))
        assert dpos <= 1e-10
    if case["vel"] is None:
        assert h.velocities is None
    else:
        assert len(h.velocities) == len(h)
        if len(h):
            dv = np.max(np.abs(np.asarray(h.velocities) - cat["velocity"])) / np.max(np.abs(case["vel"]))
            print("%s: mean velocity off by %.3g max |v|" % (case["name"], dv))
            assert dv <= 1e-10


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("index", range(NCASES), ids=IDS)
def test_constructed_cases_equal_the_reference(index, prec):
    case, cat = fc.reference(index)
    _check(_find(case, prec), case, cat)


@pytest.mark.parametrize("prec", PRECS)
def test_many_cells_scan_carries_across_rounds(prec):
    """fb_fof_link itself on 128 x 128 x 64 cells of the unit box: the scan of the cell histogram writes 2^20 + 1 offsets, 257
    chunks of 4096, so the one workgroup that scans the chunk sums takes a second round of 256 and carries the running sum
    into it -- the offsets of the last cell, and start[ncells] = n, come from that round.  Roots and group sizes equal the
    definition's exactly (what the case holds is asserted by tests/test_fof_cases_cpu.py)."""
    import ctypes
    pos, L, ell, roots = fc.case_g_many_cells()
    n, ncells = pos.shape[0], fc.G_CELLS[0] * fc.G_CELLS[1] * fc.G_CELLS[2]
    box = _box(L, prec)
    eng = box.engine
    wbytes = int(eng.lib.fb_fof_work_bytes(n, ncells))
    assert 8 * ncells < wbytes < 8 * ncells + (1 << 20)              # about 8 MiB: the cell table and its cursors
    pbuf, work, root = eng.upload_raw(pos), eng._alloc_bytes(wbytes), eng._alloc_bytes(4 * n)
    bad = ctypes.c_int32(0)
    _lib.call("fb_fof_link", eng._plan, pbuf.ptr, n, ell, (ctypes.c_int32 * 3)(*fc.G_CELLS), work.ptr, wbytes, root.ptr,
              ctypes.byref(bad), None, eng.stream)
    assert not bad.value
    count, small, kept = eng._alloc_bytes(4 * n), eng._alloc_bytes(256), eng._alloc_bytes(8 * n)
    out = (ctypes.c_int64 * 2)()
    _lib.call("fb_fof_sizes", eng._plan, root.ptr, n, 1, small.ptr, count.ptr, kept.ptr, out, eng.stream)
    got = np.empty(n, dtype=np.uint32)
    pairs = np.empty((n, 2), dtype=np.uint32)
    _lib.call("fb_memcpy_d2h", got.ctypes.data_as(ctypes.c_void_p), root.ptr, got.nbytes, eng.stream)
    _lib.call("fb_memcpy_d2h", pairs.ctypes.data_as(ctypes.c_void_p), kept.ptr, pairs.nbytes, eng.stream)
    eng.sync()
    np.testing.assert_array_equal(got, roots)
    uniq, cnt = np.unique(roots, return_counts=True)
    assert (int(out[0]), int(out[1])) == (uniq.size, uniq.size)
    pairs = pairs[:uniq.size]
    pairs = pairs[np.argsort(pairs[:, 0])]
    np.testing.assert_array_equal(pairs[:, 0], uniq)
    np.testing.assert_array_equal(pairs[:, 1], cnt)


def test_default_particle_mass():
    case, _ = fc.reference(0)
    h = _find(case, "f64")
    V, n = 100. ** 3, case["pos"].shape[0]
    om = default_cosmo['Omega_c'] + default_cosmo['Omega_b']
    assert abs(h.particle_mass / (om * 2.77536627e11 * default_cosmo['h'] ** 2 * V / n) - 1.) < 1e-14
    box = _box(case["L"], "f64")
    h2 = box.find_halos(case["pos"], linking_length=0.6, nmin=5, particle_mass=2.5)
    np.testing.assert_array_equal(h2.mass, 2.5 * h2.count)


@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_are_bit_identical(prec):
    case, _ = fc.reference(1)
    a, b = _find(case, prec), _find(case, prec)
    assert len(a) > 10
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.asarray(a.velocities).tobytes() == np.asarray(b.velocities).tobytes()
    assert np.asarray(a.labels).tobytes() == np.asarray(b.labels).tobytes()


def test_shuffled_particles_give_the_same_groups():
    case, cat = fc.reference(1)
    n = case["pos"].shape[0]
    perm = np.random.RandomState(99).permutation(n)
    box = _box(case["L"], "f64")
    h = box.find_halos(case["pos"][perm], linking_length=case["ell"], nmin=case["nmin"], absolute=True)
    np.testing.assert_array_equal(h.count, cat["count"])
    assert h.n_groups_all == cat["n_groups_all"] and h.velocities is None
    lab = np.asarray(h.labels)

    def partition(labels, orig):
        """per original particle: the least original index of its kept group, -1 if none"""
        least = np.full(labels.max() + 1, n, dtype=np.int64)
        kept = labels >= 0
        np.minimum.at(least, labels[kept], orig[kept])
        out = np.full(n, -1, dtype=np.int64)
        out[orig[kept]] = least[labels[kept]]
        return out

    np.testing.assert_array_equal(partition(lab, perm), partition(cat["labels"], np.arange(n)))


@pytest.mark.parametrize("prec", PRECS)
def test_paint_catalogue_takes_the_halos(prec):
    case, _ = fc.reference(1)
    box = _box(case["L"], prec)
    h = _find(case, prec)
    mesh = np.asarray(box.paint_catalogue(h, window='cic'))
    assert abs(mesh.sum() - len(h)) <= 1e-5 * len(h)


def test_device_catalogues_as_input():
    """A HaloCatalogue carries no velocities; a FoFHalos or ColaParticles carries its own."""
    case, cat = fc.reference(1)
    box = _box(case["L"], "f64")
    eng = box.engine
    hc = HaloCatalogue(eng, eng.upload_raw(case["pos"]), case["pos"].shape[0])
    h = box.find_halos(hc, linking_length=case["ell"], nmin=case["nmin"], absolute=True)
    assert h.velocities is None
    np.testing.assert_array_equal(np.asarray(h.labels), cat["labels"])
    with pytest.raises(ValueError, match="velocities"):
        box.find_halos(hc, linking_length=case["ell"], absolute=True, velocities=case["vel"])
    other = _box(case["L"], "f32")
    with pytest.raises(ValueError, match="this box"):
        other.find_halos(hc, linking_length=case["ell"], absolute=True)


@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_inputs(prec):
    box = _box((32., 32., 32.), prec)
    for n in (0, 1):
        t = fc.case_f_tiny(n)
        h = box.find_halos(t["pos"], linking_length=0.5, nmin=2, absolute=True)
        assert len(h) == 0 and np.asarray(h).shape == (0, 3) and h.velocities is None and h.n_groups_all == n
        assert np.asarray(h.labels).tolist() == [-1] * n and h.count.size == 0
    h = box.find_halos(np.zeros((0, 3)))                         # no particles: no mean spacing either
    assert len(h) == 0 and np.isnan(h.linking_length)
    h = box.find_halos(np.full((1, 3), 3.), nmin=1)              # the default relative length of one particle
    assert len(h) == 1 and h.count.tolist() == [1] and np.array_equal(np.asarray(h), [[3., 3., 3.]])
    bad = fc.case_f_outside()["pos"].copy()
    # not finite, or |x| >= 2^52 L, where x - L floor(x / L) is off by units of ulp(x) >= L and lands on 0 or far outside
    # the box: refused, and the particle enters no cell
    for v in (np.nan, np.inf, -np.inf, 1e20 * 32., -1e20 * 32., -1.2345678e21, 3.3e300, 2. ** 52 * 32., -2. ** 52 * 32.):
        bad[4, 1] = v
        with pytest.raises(ValueError, match="not finite, or too large"):
            box.find_halos(bad, linking_length=0.5, nmin=2, absolute=True)
    huge = np.random.RandomState(4).uniform(1e18, 1e22, (4096, 3)) * np.array([1., -1., 1.])
    assert np.abs(huge).min() >= 2. ** 52 * 32.                 # garbage such as np.empty's: every coordinate past the limit
    with pytest.raises(ValueError, match="too large"):
        box.find_halos(huge, linking_length=0.5, nmin=2, absolute=True)
    far = fc.case_f_outside()
    moved = far["pos"] + 32. * 2. ** 20                          # a million boxes away still wraps: same groups
    h = box.find_halos(moved, linking_length=0.5, nmin=2, absolute=True)
    np.testing.assert_array_equal(np.asarray(h.labels), fn.catalogue(moved, None, fn.groups_loop(moved, far["L"], 0.5)[0],
                                                                     far["L"], 2)["labels"])
    good = fc.case_f_outside()
    vel = good["vel"].copy()
    vel[2, 0] = np.nan
    with pytest.raises(ValueError, match="velocity is not finite"):
        box.find_halos(good["pos"], linking_length=0.5, nmin=2, absolute=True, velocities=vel)
    vel[2, 0] = 1e308                                            # finite, but n max |v| is not: no bound for the fixed point
    with pytest.raises(ValueError, match="overflows"):
        box.find_halos(good["pos"], linking_length=0.5, nmin=2, absolute=True, velocities=vel)
    vel[2, 0] = 1e300                                            # large and fine
    h = box.find_halos(good["pos"], linking_length=0.5, nmin=2, absolute=True, velocities=vel)
    ref = fn.catalogue(good["pos"], vel, fn.groups_loop(good["pos"], good["L"], 0.5)[0], good["L"], 2)
    assert np.max(np.abs(np.asarray(h.velocities) - ref["velocity"])) <= 1e-10 * 1e300
    with pytest.raises(ValueError, match="linking length"):
        _box((8., 8., 8.), "f64").find_halos(fc.case_c(2.5)["pos"], linking_length=4.0, absolute=True)


def test_error_paths_through_their_host_checks(monkeypatch):
    """MemoryError before any kernel when the work memory does not fit; RuntimeError when the library reports that a
    union-find loop hit its iteration cap.  Neither is provoked on the device."""
    case, _ = fc.reference(0)
    box = _box(case["L"], "f64")
    calls = []
    real_call = _lib.call

    def spy(name, *a):
        calls.append(name)
        return real_call(name, *a)

    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 20)
    monkeypatch.setattr(halos._lib, "call", spy)
    with pytest.raises(MemoryError, match="work memory"):
        big = np.zeros((200000, 3))
        box.find_halos(big, linking_length=1., absolute=True)
    assert calls == []
    monkeypatch.undo()
    n, cells = 1024 ** 3, halos.fof_cells(case["L"], 0.2 * 100. / 1024, 1024 ** 3)
    assert 40 * n < halos.fof_device_bytes(n, cells, 20) < 64 * n

    def capped(name, *a):
        if name == "fb_fof_link":
            raise _lib.FastBoxError(name, -5, "friends-of-friends: a find or union loop hit its iteration cap")
        return real_call(name, *a)

    monkeypatch.setattr(halos._lib, "call", capped)
    with pytest.raises(RuntimeError, match="iteration cap"):
        _find(case, "f64")


def test_cola_particles_end_to_end():
    """COLA at 64^3, default b = 0.2: labels and counts equal the periodic k-d tree's on the downloaded particles."""
    N, Lbox = 64, 200.
    box = CosmoBox(cosmo=default_cosmo, box_scale=Lbox, nsamp=N, realise_now=False, precision="f32", rng="device", seed=5)
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, n_steps=8, seed=12, return_particles=True,
                                        inplace=False)
    pos, vel = np.asarray(parts), np.asarray(parts.velocities)
    L = (box.Lx,) * 3
    ell = halos.fof_linking_length(L, N ** 3, 0.2)
    lo, hi = fn.tree_pairs(pos, L, ell * (1. - 1e-9)), fn.tree_pairs(pos, L, ell * (1. + 1e-9))
    if lo.shape != hi.shape:
        pytest.skip("a pair of this COLA run lies within 1e-9 of the linking length")
    roots = fn._roots(N ** 3, lo[:, 0], lo[:, 1])
    uniq, cnt = np.unique(roots, return_counts=True)
    keep = cnt >= 20
    order = np.lexsort((uniq[keep], -cnt[keep]))
    kroots, kcount = uniq[keep][order], cnt[keep][order]
    rank = np.full(N ** 3, -1, dtype=np.int32)
    rank[kroots] = np.arange(kroots.size)
    h = box.find_halos(parts)
    print("COLA 64^3: l = %.4f Mpc, %d groups, %d kept, largest %d" % (ell, uniq.size, kroots.size, kcount[0]))
    assert h.linking_length == ell and kroots.size > 50 and kcount[0] > 100
    assert h.n_groups_all == uniq.size
    np.testing.assert_array_equal(h.count, kcount)
    np.testing.assert_array_equal(h.roots, kroots)
    np.testing.assert_array_equal(np.asarray(h.labels), rank[roots])
    vm = np.asarray(h.velocities)
    for g in range(5):
        ref = np.mean(vel[roots == kroots[g]], axis=0)
        assert np.max(np.abs(vm[g] - ref)) <= 1e-10 * np.max(np.abs(vel))
    mesh = np.asarray(box.paint_catalogue(h, weights=h.mass))
    assert abs(mesh.sum() / h.mass.sum() - 1.) < 1e-5
