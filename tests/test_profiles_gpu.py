"""GPU: halo profiles, aperture moments and spherical-overdensity masses (fb_profiles.hip; fastbox_amd.halos.halo_profiles,
halo_apertures, spherical_overdensity) on the constructed cases of tests/profiles_cases.py in both plan precisions: the
counts are exactly those of the numpy statement tests/profiles_numpy.py, the moments agree with its correctly rounded sums to
the fixed-point step, and the radii come from identical integers.  What each case is for is asserted on the CPU by
tests/test_profiles_cases_cpu.py.  The largest input is the 6,046 points of the blobs."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, halos
from fastbox_amd.halos import ColaParticles, FoFHalos, HaloCatalogue, HaloProfiles, SOHalos
from tests import profiles_cases as pc
from tests import profiles_numpy as pf
from tests.fof_numpy import min_image

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
NCASES = len(pc.NAMES)


@functools.lru_cache(maxsize=None)
def _box(L, prec, N=16):
    scale = L[0] if L[0] == L[1] == L[2] else tuple(L)
    box = CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, realise_now=False, precision=prec, rng="device", seed=7)
    assert (box.Lx, box.Ly, box.Lz) == tuple(L)
    return box


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("index", range(NCASES), ids=pc.NAMES)
def test_counts_equal_the_statement(index, prec):
    case, inner, counts = pc.reference(index)
    box = _box(case["L"], prec)
    p = box.halo_profiles(case["centres"], case["pos"], case["edges"], particle_mass=2.)
    assert isinstance(p, HaloProfiles) and p.counts.dtype == np.int64 and p.inner.dtype == np.int64 and p.particle_mass == 2.
    print("%s: %d particles in the bins, %d inside the first edge" % (case["name"], p.counts.sum(), p.inner.sum()))
    np.testing.assert_array_equal(p.inner, inner)
    np.testing.assert_array_equal(p.counts, counts)
    np.testing.assert_array_equal(p.edges, case["edges"])
    np.testing.assert_array_equal(p.enclosed[:, 0], inner)
    np.testing.assert_array_equal(np.diff(p.enclosed, axis=1), counts)
    assert p.density.shape == counts.shape and p.enclosed_density.shape == p.enclosed.shape and p.r.shape == (counts.shape[1],)
    if case["expect_counts"] is not None:
        np.testing.assert_array_equal(p.counts, case["expect_counts"])
        np.testing.assert_array_equal(p.inner, case["expect_inner"])
    if case["name"] in ("2 seam", "5 many centres"):
        np.testing.assert_array_equal(p.counts[0], p.counts[1])
        assert p.inner[0] == p.inner[1]
    # the existing pair counts test the same pairs and sum them over the centres
    pairs = box.pair_counts(case["centres"], second=case["pos"], edges=case["edges"])
    np.testing.assert_array_equal(p.counts.sum(axis=0), pairs.npairs)


def _check_apertures(case, ref, got, vel):
    count, com, vmean, sigma = got
    n, L = case["pos"].shape[0], np.array(case["L"])
    np.testing.assert_array_equal(count, ref["count"])
    empty = ref["count"] == 0
    assert np.all(np.isnan(com[empty])) and np.all(np.isfinite(com[~empty]))
    if vel:
        assert np.all(np.isnan(vmean[empty])) and np.all(np.isnan(sigma[empty]))
    if empty.all():
        return
    m = ref["count"][~empty].astype(np.float64)
    # Every term enters its sum rounded to a multiple of 2^-F, F = 93 - e with (n x bound of a term) < 2^e: the sum of m
    # terms is within m 2^-F of the exact one (half of that, in fact).  The statement's sum is the correctly rounded exact
    # one.  Joining the two words, dividing by m, adding the centre (a value below 2 L: one rounding of at most ulp(L)) and
    # wrapping round the device's result at most four times at the magnitude of L, and the statement's as often.
    Fp = pf.fx_bits(n * 0.5 * L.max())
    err = np.abs(min_image(com[~empty] - ref["com"][~empty], L))
    tol = m[:, None] * 2. ** -Fp + 4. * np.spacing(L)[None, :]
    print("com: largest error %.3e, bound %.3e (F = %d)" % (err.max(), tol.min(), Fp))
    assert np.all(err <= tol)
    if not vel:
        assert vmean is None and sigma is None
        return
    vmax = np.abs(case["vel"]).max()
    Fv = pf.fx_bits(n * vmax)
    err = np.abs(vmean[~empty] - ref["vmean"][~empty])
    tol = m[:, None] * 2. ** -Fv + 2. * np.spacing(np.abs(ref["vmean"][~empty]))
    print("vmean: largest error %.3e, bound %.3e (F = %d)" % (err.max(), tol.min(), Fv))
    assert np.all(err <= tol) and np.all(np.isnan(vmean[empty])) and np.all(np.isnan(sigma[empty]))
    err = np.abs(sigma[~empty] ** 2 - ref["sigma_v"][~empty] ** 2)
    print("sigma_v^2: largest error %.3e of %.3e, bound %.3e" % (err.max(), (ref["sigma_v"][~empty] ** 2).max(), 1e-12 * ref["svv"][~empty].min()))
    assert np.all(err <= 1e-12 * ref["svv"][~empty])


@pytest.mark.parametrize("prec", PRECS)
def test_apertures_against_correctly_rounded_sums(prec):
    index = pc.index_of("8 apertures")
    case, ref = pc.all_cases()[index], pc.aperture_reference(index)
    box = _box(case["L"], prec)
    t = {}
    got = halos.halo_apertures(box, case["centres"], case["pos"], case["r2"], velocities=case["vel"], timings=t)
    _check_apertures(case, ref, got, True)
    assert got[0][0] == 0 and got[0][1] >= 2 and t["bin_ms"] > 0. and t["aperture_ms"] > 0. and t["cells"] == (4, 4, 4)
    _check_apertures(case, ref, halos.halo_apertures(box, case["centres"], case["pos"], case["r2"]), False)
    # the crowded cell: 1025 members through the strided loop of every thread
    case = pc.all_cases()[pc.index_of("4 crowded cell of 1025")]
    r2 = np.array([3.9 ** 2, 1., 3.5 ** 2])
    ref = pf.apertures(case["centres"], case["pos"], case["L"], r2)
    assert ref["count"][0] == 1025 and 0 < ref["count"][1] < ref["count"][2] < 1025
    _check_apertures(case, ref, halos.halo_apertures(_box(case["L"], prec), case["centres"], case["pos"], r2), False)


def _so_fields(s):
    out = [s.radius, s.mass, s.status, s.count, np.asarray(s.com), s.profiles.counts, s.profiles.inner]
    if s.velocities is not None:
        out += [np.asarray(s.velocities), s.sigma_v]
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_spherical_overdensity_equals_the_statement_and_repeats(prec):
    """status and count exact, radius and mass at rtol 1e-12 (fp64 numpy on both sides from identical integers); a second call
    and a random permutation of the particles give the same bits, the fixed-point moments included."""
    rs = np.random.RandomState(5)
    for name, want in (("7 blobs rmax=4", [0, 0, 0, 1]), ("7 blobs rmax=0.3", [2, 2, 2, 1])):
        case, inner, counts = pc.reference(pc.index_of(name))
        box, so = _box(case["L"], prec), case["so"]
        vel = np.array([300., -200., 100.]) + 50. * np.random.RandomState(6).standard_normal(case["pos"].shape)
        for delta in so["deltas"]:
            kw = dict(delta=delta, reference=so["rho_ref"], edges=case["edges"], particle_mass=so["particle_mass"])
            s = box.spherical_overdensity(case["centres"], case["pos"], velocities=vel, **kw)
            assert isinstance(s, SOHalos) and isinstance(s, HaloCatalogue) and isinstance(s.com, HaloCatalogue) and len(s) == 4
            r, m, st = pf.so_statement(case["edges"], inner, counts, so["particle_mass"], so["rho_ref"], delta)
            print("%s, Delta = %g: R = %s, members %s" % (name, delta, s.radius, s.count))
            np.testing.assert_array_equal(s.status, want)
            np.testing.assert_array_equal(s.status, st)
            np.testing.assert_allclose(s.radius, r, rtol=1e-12)
            np.testing.assert_allclose(s.mass, m, rtol=1e-12)
            np.testing.assert_array_equal(s.profiles.counts, counts)
            np.testing.assert_array_equal(np.asarray(s), case["centres"])
            assert (s.delta, s.rho_ref, s.particle_mass) == (delta, so["rho_ref"], so["particle_mass"])
            ref = pf.apertures(case["centres"], case["pos"], case["L"], np.where(s.status == 0, s.radius * s.radius, 0.), vel)
            _check_apertures(dict(case, vel=vel), ref, (s.count, np.asarray(s.com), np.asarray(s.velocities), s.sigma_v), True)
            assert np.all((s.count > 0) == (s.status == 0))
            # a second call, and the particles in another order
            again = box.spherical_overdensity(case["centres"], case["pos"], velocities=vel, **kw)
            order = rs.permutation(case["pos"].shape[0])
            shuffled = box.spherical_overdensity(case["centres"], case["pos"][order], velocities=vel[order], **kw)
            for a, b, c in zip(_so_fields(s), _so_fields(again), _so_fields(shuffled)):
                assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
            assert s.sigma_v.tobytes() == shuffled.sigma_v.tobytes() and np.asarray(s.com).tobytes() == np.asarray(shuffled.com).tobytes()
    # the catalogue goes where a HaloCatalogue goes
    mesh = box.paint_catalogue(s, window='cic')
    assert abs(float(np.asarray(mesh).sum()) - 4.) < 1e-4
    assert box.pair_counts(s, second=case["pos"], edges=case["edges"]).npairs.sum() == counts.sum()


@pytest.mark.parametrize("prec", PRECS)
def test_device_objects_match_their_host_copies(prec):
    """The ColaParticles of a 16^3 COLA run and the FoFHalos found in it, passed as device objects and as host arrays; no
    particle, no centre, one centre; the defaults."""
    box = CosmoBox(cosmo=default_cosmo, box_scale=64., nsamp=16, realise_now=False, precision=prec, rng="device", seed=3)
    _, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    fof = box.find_halos(particles, linking_length=0.4, nmin=2)
    assert isinstance(particles, ColaParticles) and isinstance(fof, FoFHalos) and len(particles) == 4096 and len(fof) >= 2
    hp, hv, hh = np.asarray(particles).copy(), np.asarray(particles.velocities).copy(), np.asarray(fof).copy()
    kw = dict(delta=50., rmax=12., nbins=16)
    dev = box.spherical_overdensity(fof, particles, **kw)
    host = box.spherical_overdensity(hh, hp, velocities=hv, **kw)
    mixed = box.spherical_overdensity(fof, hp, velocities=hv, **kw)
    for a, b, c in zip(_so_fields(dev), _so_fields(host), _so_fields(mixed)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert dev.velocities is not None and np.count_nonzero(dev.status == 0) >= 1 and dev.particle_mass == fof.particle_mass
    assert abs(dev.profiles.edges[0] - 1.) < 1e-12 and abs(dev.profiles.edges[-1] - 12.) < 1e-12      # a quarter of the 4 Mpc spacing
    inner, counts = pf.profiles(hh, hp, (64.,) * 3, dev.profiles.edges)
    np.testing.assert_array_equal(dev.profiles.counts, counts)
    np.testing.assert_array_equal(dev.profiles.inner, inner)
    novel = box.spherical_overdensity(fof, hp, **kw)                     # host positions without velocities
    assert novel.velocities is None and novel.sigma_v is None
    np.testing.assert_array_equal(novel.count, dev.count)
    np.testing.assert_array_equal(box.halo_profiles(fof, particles, dev.profiles.edges).counts, counts)
    # rho_ref at z = 0: E = a = 1
    h2 = default_cosmo['h'] ** 2
    assert abs(halos.so_reference_density(box, 'crit') / (halos.RHO_CRIT * h2) - 1.) < 1e-12
    assert abs(dev.rho_ref / ((default_cosmo['Omega_c'] + default_cosmo['Omega_b']) * halos.RHO_CRIT * h2) - 1.) < 1e-12
    assert default_cosmo['Omega_c'] + default_cosmo['Omega_b'] < 1. and halos.so_reference_density(box, 3.5) == 3.5
    with pytest.raises(ValueError, match="reference"):
        halos.so_reference_density(box, 'virial')
    default = box.spherical_overdensity(fof, particles)                  # 32 bins from 1 Mpc to 5 Mpc
    assert default.profiles.counts.shape == (len(fof), 32) and default.profiles.edges[-1] == 5. and default.delta == 200.
    other = _box((64., 64., 64.), prec)
    with pytest.raises(ValueError, match="of this box"):
        other.spherical_overdensity(fof, hp, **kw)
    with pytest.raises(ValueError, match="of this box"):
        other.halo_profiles(hh, particles, dev.profiles.edges)
    # no particle, no centre, one centre
    none = np.zeros((0, 3))
    s = box.spherical_overdensity(hh, none, velocities=none.copy(), **kw)
    assert s.profiles.counts.sum() == 0 and np.all(s.status == 1) and np.all(s.count == 0) and np.all(np.isnan(np.asarray(s.com)))
    assert np.all(np.isnan(np.asarray(s.velocities))) and np.all(np.isnan(s.sigma_v))
    s = box.spherical_overdensity(none, particles, **kw)
    assert len(s) == 0 and s.radius.shape == (0,) and s.profiles.counts.shape == (0, 16) and np.asarray(s.com).shape == (0, 3)
    assert box.halo_profiles(none, hp, [1., 2.]).counts.shape == (0, 1)
    s = box.spherical_overdensity(hh[:1], particles, **kw)
    for a, b in zip(_so_fields(s), _so_fields(dev)):
        np.testing.assert_array_equal(a, b[:1])


@pytest.mark.parametrize("prec", PRECS)
def test_bad_inputs(prec):
    box = _box((32., 32., 32.), prec)
    good = np.random.RandomState(9).uniform(-40., 70., (300, 3))        # outside [0, L) as well: wrapped on read
    centres = np.array([[1., 2., 3.], [31., 30., -1.]])
    edges = np.array([0., 0.5, 2., 5.])
    want = pf.profiles(centres, good, (32.,) * 3, edges)[1]
    np.testing.assert_array_equal(box.halo_profiles(centres, good, edges).counts, want)
    assert want.sum() > 0
    for value in (np.nan, np.inf, -np.inf, 2. ** 52 * 32., -2. ** 52 * 32.):
        pos, cen = good.copy(), centres.copy()
        pos[3, 1] = value
        cen[1, 2] = value
        for fn in (lambda c, p: box.halo_profiles(c, p, edges), lambda c, p: box.spherical_overdensity(c, p, edges=edges),
                   lambda c, p: halos.halo_apertures(box, c, p, [1., 4.])):
            with pytest.raises(ValueError, match="not finite, or too large"):
                fn(centres, pos)
            with pytest.raises(ValueError, match="not finite, or too large"):
                fn(cen, good)
    pos, cen = good.copy(), centres.copy()
    pos[3, 1] = 2. ** 51 * 32.                                         # still wraps
    cen[1, 2] = 2. ** 51 * 32.
    np.testing.assert_array_equal(box.halo_profiles(cen, pos, edges).counts, pf.profiles(cen, pos, (32.,) * 3, edges)[1])
    vel = np.zeros_like(good)
    for value in (np.nan, np.inf, 1e200):                              # 3 n v^2 overflows for the last
        vel[7, 0] = value
        with pytest.raises(ValueError, match="velocity is not finite"):
            box.spherical_overdensity(centres, good, edges=edges, velocities=vel)
    for bad_edges in ([1., 3., 2.], [1., 1.], np.linspace(0., 5., 258), [1., 16.], [1., 20.], [-1., 2.], [1., np.nan]):
        with pytest.raises(ValueError, match="edges"):
            box.halo_profiles(centres, good, bad_edges)
        with pytest.raises(ValueError, match="edges"):
            box.spherical_overdensity(centres, good, edges=bad_edges)
    with pytest.raises(ValueError, match="radius2"):
        halos.halo_apertures(box, centres, good, [1., 16. ** 2])
    with pytest.raises(ValueError, match="radius2"):
        halos.halo_apertures(box, centres, good, [1.])


def test_timings_and_memory_guard(monkeypatch):
    """The stage timings; MemoryError before any kernel when the work memory does not fit (not provoked on the device)."""
    case, inner, counts = pc.reference(pc.index_of("6 nr=1"))
    box = _box(case["L"], "f64")
    t = {}
    p = halos.halo_profiles(box, case["centres"], case["pos"], case["edges"], timings=t)
    np.testing.assert_array_equal(p.counts, counts)
    assert t["cells"] == (5, 5, 5) and t["bin_ms"] > 0. and t["profile_ms"] > 0.
    calls = []
    real_call = halos._lib.call
    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 20)
    monkeypatch.setattr(halos._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    with pytest.raises(MemoryError, match="work memory"):
        box.halo_profiles(case["centres"], np.zeros((200000, 3)), case["edges"])
    with pytest.raises(MemoryError, match="work memory"):
        box.spherical_overdensity(case["centres"], np.zeros((200000, 3)), edges=case["edges"])
    assert calls == []
    monkeypatch.undo()
    n, nh = 1024 ** 3, 10 ** 6
    plain = halos.profile_device_bytes(n, nh, (64, 64, 64), 32)
    assert 28 * n < plain < 29 * n and 56 * n < halos.profile_device_bytes(n, nh, (64, 64, 64), 32, velocities=True) < 57 * n
    assert halos.profile_device_bytes(n, nh, (64, 64, 64), 32, host_particles=True) > 52 * n
