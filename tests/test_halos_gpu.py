"""GPU: halo tracers (fastbox_amd/halos.py; fb_halo_lambda, fb_halo_counts, fb_halo_catalogue*, fb_paint*) against the
reference's golden draws (tests/golden/halos_n*.npz), the host model of the device streams (fastbox_amd/rng.py) and the numpy
statements of tests/halos_numpy.py, in both precisions."""
import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, rng
from fastbox_amd.halos import HaloDistribution
from tests import halos_numpy as hn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")


def _box(N, L, prec, rng_="device", seed=7):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng=rng_, seed=seed)


def _stored(x, prec):
    return np.asarray(x, dtype=np.float64).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)


# ---- 1. rng='numpy' against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [16, 32])
def test_numpy_rng_matches_reference(golden_dir, prec, N):
    g = np.load("%s/halos_n%d.npz" % (golden_dir, N))
    box = _box(N, tuple(g["L"]), prec, rng_="numpy")
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    np.random.seed(int(g["seed_counts"]))
    c = hd.halo_count_field(g["delta"].astype(np.float64), g["nbar_z"], float(g["bias"]))
    ch = np.asarray(c)
    if prec == "f64":
        np.testing.assert_array_equal(ch, g["counts"])
    else:
        assert np.mean(ch != g["counts"]) <= 1e-4
    np.random.seed(int(g["seed_counts_ln"]))
    cl = np.asarray(hd.halo_count_field(g["delta"].astype(np.float64), g["nbar_z"], float(g["bias"]), lognormal=True))
    assert np.mean(cl != g["counts_ln"]) <= 1e-4
    # catalogues: bitwise where the counts are the reference's
    if np.array_equal(ch, g["counts"]):
        cat = hd.realise_halo_catalogue(c)
        assert len(cat) == g["cat"].shape[0]
        np.testing.assert_array_equal(np.asarray(cat), g["cat"])
        np.random.seed(int(g["seed_cat"]))
        cs = hd.realise_halo_catalogue(c, scatter=True)
        np.testing.assert_array_equal(np.asarray(cs), g["cat_scatter"])
    # a host integer array is accepted as well
    np.testing.assert_array_equal(np.asarray(hd.realise_halo_catalogue(g["counts"])), g["cat"])


# ---- 2. rng='device' against the host model ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [64, 256])
def test_device_counts_match_host_model(prec, N):
    L = (float(N) * 4., float(N) * 4.5, float(N) * 5.)
    box = _box(N, L, prec, seed=11 + N)
    delta = box.realise_density()
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    vv = L[0] * L[1] * L[2] / N ** 3.
    nbar_z = np.linspace(0.3, 3.0, N) / vv
    c = hd.halo_count_field(delta, nbar_z, 1.3)
    lam = hn.expected_counts(_stored(delta, prec), nbar_z, 1.3, L)
    ref = rng.stream_poisson(lam, box.seed, hd.last_realisation)
    got = np.asarray(c).astype(np.int64)
    diff = got != ref
    assert diff.mean() <= 1e-6 and np.all(np.abs(got - ref)[diff] == 1), diff.sum()
    # mean and variance per lam class
    cls = np.digitize(lam, [0.5, 1., 2., 4.])
    for q in range(5):
        m = cls == q
        if m.sum() < 1000:
            continue
        l = lam[m]
        assert abs(got[m].mean() - l.mean()) < 6 * np.sqrt(l.mean() / m.sum()) + 1e-12
        assert abs((got[m] - l).var() / l.mean() - 1.) < 0.1
    # determinism in (seed, realisation, voxel)
    c2 = hd.halo_count_field(delta, nbar_z, 1.3, realisation=hd.last_realisation)
    np.testing.assert_array_equal(np.asarray(c2), np.asarray(c))


@pytest.mark.parametrize("prec", PRECS)
def test_param_forms_agree(prec):
    N, L = 32, (200., 200., 200.)
    box = _box(N, L, prec)
    delta = box.realise_density()
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    vv = L[0] * L[1] * L[2] / N ** 3.
    nb, bs = 1.7 / vv, 1.2
    ref = np.asarray(hd.halo_count_field(delta, nb, bs, realisation=5))
    prof = np.full(N, nb)
    for a, b in ((prof, bs), (nb, np.full(N, bs)), (np.full((N, N, N), nb), bs), (nb, np.full((N, N, N), bs)),
                 (nb, box.engine.upload(np.full((N, N, N), bs), "real"))):
        np.testing.assert_array_equal(np.asarray(hd.halo_count_field(delta, a, b, realisation=5)), ref)
    for ln in (False, True):
        np.testing.assert_array_equal(np.asarray(hd.halo_count_field(delta, prof, bs, lognormal=ln, realisation=6)),
                                      np.asarray(hd.halo_count_field(delta, nb, np.full((N, N, N), bs), lognormal=ln,
                                                                     realisation=6)))


@pytest.mark.parametrize("prec", PRECS)
def test_negative_and_nan_lambda_give_zero(prec):
    N, L = 16, (100., 100., 100.)
    box = _box(N, L, prec)
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    d = np.full((N, N, N), 0.5)
    d[0] = -5.                   # 1 + delta < 0
    d[1] = np.nan
    vv = L[0] * L[1] * L[2] / N ** 3.
    c = np.asarray(hd.halo_count_field(d, 4. / vv, 1.))
    assert np.all(c[0] == 0) and np.all(c[1] == 0) and c[2:].sum() > 0
    with pytest.raises(ValueError):
        hd.halo_count_field(np.zeros((N, N, N)), 2. ** 25 / vv, 1.)
    with pytest.raises(ValueError):
        hd.realise_halo_catalogue(c, scatter=True, scatter_type="gaussian")
    empty = hd.realise_halo_catalogue(np.zeros((N, N, N), dtype=np.int64))
    assert len(empty) == 0 and np.asarray(empty).shape == (0, 3)


@pytest.mark.parametrize("prec", PRECS)
def test_device_catalogue_order_and_scatter(prec):
    N, L = 32, (300., 310., 320.)
    box = _box(N, L, prec, seed=99)
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    c = hd.halo_count_field(box.realise_density(), 2.5 / (L[0] * L[1] * L[2] / N ** 3.), 2.0)
    ch = np.asarray(c)
    cat = hd.realise_halo_catalogue(c)
    np.testing.assert_array_equal(np.asarray(cat), hn.catalogue(ch, L))
    cs = hd.realise_halo_catalogue(c, scatter=True)
    u = rng.scatter_uniforms(len(cs), box.seed, hd.last_realisation)
    np.testing.assert_array_equal(np.asarray(cs), hn.catalogue(ch, L, u))


@pytest.mark.parametrize("prec", PRECS)
def test_catalogue_with_large_counts(prec):
    N, L = 16, (160., 170., 180.)
    box = _box(N, L, prec)
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    rs = np.random.RandomState(8)
    c = rs.poisson(0.7, (N, N, N))
    c[3, 4, 5], c[0, 0, 1], c[15, 15, 15], c[7, 0, 0] = 5000, 4095, 12345, 5000      # past the LDS histogram
    cat = hd.realise_halo_catalogue(c)
    assert len(cat) == c.sum()
    np.testing.assert_array_equal(np.asarray(cat), hn.catalogue(c, L))


@pytest.mark.parametrize("prec", PRECS)
def test_catalogue_table_scan_carries_across_rounds(prec):
    """A count of 16384 at 64^3 (64 tiles of 4096 voxels): the (count, tile) table has 16385 x 64 = 1048640 entries, 257 chunks
    of 4096, so the one workgroup that scans the chunk sums takes a second round of 256 and carries the running sum into it.
    The entries of count 16384 are the ones of chunk 256: their halos start after everything else, the second voxel's after
    the first's."""
    N, L = 64, (640., 650., 660.)
    box = _box(N, L, prec)
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    c = np.zeros((N, N, N), dtype=np.int64)
    c[0, 0, 5], c[2, 3, 4], c[63, 63, 63] = 1, 3, 2                     # tiles 0, 2 and 63
    c[20, 1, 1], c[40, 40, 40] = 4097, 9000                             # past the LDS histogram, chunks 64 and 140
    c[3, 10, 7], c[60, 2, 9] = 16384, 16384                             # chunk 256, tiles 3 and 60
    assert (c.max() + 1) * (N ** 3 // 4096) == 1048640 and -(-1048641 // 4096) == 257
    cat = hd.realise_halo_catalogue(c)
    assert len(cat) == c.sum()
    np.testing.assert_array_equal(np.asarray(cat), hn.catalogue(c, L))


# ---- 3. painting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", ["ngp", "cic", "tsc"])
def test_paint_matches_oracle(prec, window):
    N, L = 32, (100., 120., 140.)
    box = _box(N, L, prec)
    rs = np.random.RandomState(5)
    pos = rs.uniform(-0.3, 1.3, (20000, 3)) * np.array(L)          # wrapped across the box edges
    w = rs.uniform(-0.5, 2.0, pos.shape[0])
    tol = 1e-12 if prec == "f64" else 1e-5
    for weights in (None, w):
        for comp in (False, True):
            m = box.paint_catalogue(pos, weights=weights, window=window, compensated=comp)
            got = np.asarray(m)
            ref = hn.paint(pos, N, L, window, weights, comp)
            assert np.max(np.abs(got - ref)) <= tol * np.max(np.abs(ref)), (weights is None, comp)
            if not comp:
                tot = pos.shape[0] if weights is None else w.sum()
                assert abs(got.sum() - tot) <= (1e-10 if prec == "f64" else 1e-4) * np.abs(w).sum()
            again = np.asarray(box.paint_catalogue(pos, weights=weights, window=window, compensated=comp))
            assert np.array_equal(got, again)


@pytest.mark.parametrize("prec", PRECS)
def test_paint_catalogue_roundtrip(prec):
    N, L = 32, (250., 250., 250.)
    box = _box(N, L, prec, seed=3)
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    c = hd.halo_count_field(box.realise_density(), 3. / (L[0] * L[1] * L[2] / N ** 3.), 1.)
    ch = np.asarray(c)
    cat = hd.realise_halo_catalogue(c)
    np.testing.assert_array_equal(np.asarray(box.paint_catalogue(cat, window="ngp")), ch)
    cic = np.asarray(box.paint_catalogue(cat, window="cic"))
    assert np.max(np.abs(cic - ch)) <= 1e-12 * ch.max() * (1e6 if prec == "f32" else 1.)


# ---- 4. the whole chain at 512^3 -------------------------------------------------------------------------------------
def test_chain_512_f32():
    N, L = 512, (1000., 1000., 1000.)
    box = _box(N, L, "f32", seed=21)
    delta = box.realise_density()
    hd = HaloDistribution(box, (1e12, 1e15), 10)
    vv = L[0] * L[1] * L[2] / N ** 3.
    c = hd.halo_count_field(delta, 1. / vv, 1.5)
    rc = hd.last_realisation
    cat = hd.realise_halo_catalogue(c, scatter=True)
    mesh = box.paint_catalogue(cat, window="tsc", compensated=True)
    kc, pk, err = box.binned_power_spectrum(delta_x=mesh)
    kd, pd, ed = box.binned_power_spectrum(delta_x=delta)
    ok = ~np.isnan(pd)                          # empty bins are NaN, as in the reference
    assert np.array_equal(np.isnan(pk), ~ok) and np.all(np.isfinite(pk[ok])) and np.all(pk[ok] > 0)
    for ix in (0, 137, 511):
        plane = box.engine.download_plane(c, ix).astype(np.float64)
        dpl = box.engine.download_plane(delta, ix).astype(np.float64)
        lam = hn.expected_counts(dpl[None], 1. / vv, 1.5, L)[0]
        u = rng.poisson_uniforms(N * N, box.seed, rc, first=ix * N * N)
        ref = rng.poisson_inverse(lam.reshape(-1), u).reshape(N, N)
        assert np.mean(plane != ref) <= 1e-5
    total = float(np.sum(np.asarray(c), dtype=np.float64))
    assert len(cat) == int(total)
