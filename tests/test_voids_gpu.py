"""GPU: void finding (fastbox_amd/voids.py; fb_watershed, fb_region_stats, fb_merge_regions, fb_stack_voids) against the numpy
statement of tests/voids_numpy.py, in both precisions: labels, counts and arg-mins exactly, sums to 1e-10 and the same bit for bit
from call to call, merged labels exactly, the catalogue functions and the stacked mean."""
import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, voids
from fastbox_amd.device import REAL
from tests import voids_numpy as vn

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
CUBE, CUBOID = (1e3, 1e3, 1e3), (1e3, 7e2, 1.3e3)


def _box(N, prec, scale=CUBE, seed=11):
    return CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, realise_now=False, precision=prec, rng="device", seed=seed)


def _stored(box, a):
    return np.asarray(a, dtype=np.float64).astype(box.engine.rdtype).astype(np.float64)


def _check_labels(lab, ref, n):
    assert lab.n_labels == n
    np.testing.assert_array_equal(np.asarray(lab), ref)


def _check_stats(st, rs, f):
    np.testing.assert_array_equal(st.count, rs["count"])
    np.testing.assert_array_equal(st.index_sum, rs["index_sum"])
    if "sum" not in rs:
        return
    np.testing.assert_array_equal(st.argmin, rs["argmin"])
    # per label: within 1e-10 of the oracle's value, or of the label's own sum of |f| where the sum cancels
    l = st.labels.host().reshape(-1).astype(np.int64)
    fa = np.abs(np.where(np.isfinite(f), f, 0.)).reshape(-1)
    absum = np.bincount(l, weights=fa, minlength=st.count.size)
    N = f.shape[0]

    def close(a, b, s):
        bad = np.abs(a - b) > 1e-10 * np.maximum(np.abs(b), 1e-3 * s)
        assert not bad.any(), (np.nonzero(bad), a[bad], b[bad])

    close(st.sum, rs["sum"], absum)
    close(st.weight_sum, rs["weight_sum"], absum)
    close(st.weighted_index_sum, rs["weighted_index_sum"], absum[:, None] * N)
    ok = rs["count"] > 0
    close(st.mean[ok], rs["mean"][ok], absum[ok] / rs["count"][ok])


def _same_bits(a, b):
    for k in ("sum", "weight_sum", "weighted_index_sum", "mean", "argmin", "count"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def _check_chain(box, d, f, scale, grid_pixes=(15,)):
    """Watershed, statistics, catalogue and stacking of the field d (a device field of the box, or a host array), whose stored
    values are f, against the numpy statement."""
    lab = voids.watershed(d, markers=None, box=box)
    ref, n = vn.watershed(f, vn.inside(f))
    _check_labels(lab, ref, n)
    st = voids.region_statistics(lab, d)
    rs = vn.region_stats(ref, n, f)
    _check_stats(st, rs, f)
    _same_bits(st, voids.region_statistics(lab, d))
    # catalogue
    cat = vn.trim(rs, 3, 10 ** 9)
    np.testing.assert_array_equal(voids.trim_by_volume(lab, 3, 10 ** 9), cat)
    L = max(scale)
    for kind in voids.KINDS:
        c = voids.void_centroids(cat, lab, box, d, kind)
        np.testing.assert_allclose(c, vn.centroids(rs, box, kind)[cat], rtol=0, atol=1e-12 * L)
    np.testing.assert_allclose(voids.void_radii_array(cat, lab, box), vn.radii(rs, box)[cat], rtol=1e-14)
    dc = voids.void_centroid(cat[:3], lab, box, d, kind="minimum")
    assert sorted(dc) == sorted(cat[:3].tolist())
    dr = voids.void_radii(cat[:3], np.asarray(lab), box)           # a host label array works as well
    np.testing.assert_allclose([dr[k] for k in cat[:3]], vn.radii(rs, box)[cat[:3]], rtol=1e-14)
    # stacking, on the device's own centres and radii
    cen = voids.void_centroids(cat, lab, box)
    rad = voids.void_radii_array(cat, lab, box)
    for pix in grid_pixes:
        stk, fail, cnt = voids.stack_voids_at(cat, lab, box, d, cen, rad, grid_pix=pix)
        o, ofail, ocnt = vn.stack(ref, f, cat, cen, rad, box, 1., pix)
        _check_stack(stk, fail, cnt, o, ofail, ocnt)
        assert (~np.ma.getmaskarray(o)).any()
        s2, f2 = voids.stack_voids(cat, lab, box, d, grid_pix=pix)
        assert s2.data.tobytes() == stk.data.tobytes() and f2 == fail
    return n


def _check_stack(stk, fail, cnt, o, ofail, ocnt):
    np.testing.assert_array_equal(cnt, ocnt)
    np.testing.assert_array_equal(np.ma.getmaskarray(stk), np.ma.getmaskarray(o))
    assert [int(x) for x in fail] == [int(x) for x in ofail]
    m = ~np.ma.getmaskarray(o)
    np.testing.assert_allclose(stk.data[m], o.data[m], rtol=1e-10, atol=1e-12)


def _check_apply_merge(box, d, f):
    """apply_watershed at a merge threshold of 0.3 sigma against the numpy statement; returns (regions, merged regions)."""
    mth = 0.3 * float(np.std(f))
    out = voids.apply_watershed(d, mask_threshold=0., merge_threshold=mth, verbose=False, box=box)
    ref, n = vn.watershed(f, vn.inside(f, threshold=0.))
    rs = vn.region_stats(ref, n, f)
    mref, M = vn.merge(ref, n, rs["mean"], mth, margin=1e-6)
    assert 0 < M < n
    _check_labels(out, mref, M)
    return n, M


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,scale", [(16, CUBE), (32, CUBE), (48, CUBE), (64, CUBE), (64, CUBOID)])
def test_watershed_statistics_catalogue_stacking(prec, N, scale):
    box = _box(N, prec, scale)
    d = box.realise_density()
    _check_chain(box, d, _stored(box, d), scale)


@pytest.mark.parametrize("prec", PRECS)
def test_plateaus_masks_nans(prec):
    N = 32
    box = _box(N, prec, seed=5)
    d = box.realise_density()
    f = _stored(box, d)
    sd = np.std(f)
    # plateaus: quantised values from the host, ties broken by the index
    q = _stored(box, np.round(f / sd * 2.) / 2.)
    lab = voids.watershed(q, box=box)
    ref, n = vn.watershed(q, vn.inside(q))
    _check_labels(lab, ref, n)
    _check_stats(voids.region_statistics(lab, q), vn.region_stats(ref, n, q), q)
    # a caller's mask, as a host array and as a device field
    m = f < 0.5 * sd
    ref, n = vn.watershed(f, vn.inside(f, mask=m))
    _check_labels(voids.watershed(d, mask=m), ref, n)
    lab = voids.watershed(d, mask=box.engine.upload(m.astype(np.float64), REAL))
    _check_labels(lab, ref, n)
    st = voids.region_statistics(lab, d)
    rs = vn.region_stats(ref, n, f)
    _check_stats(st, rs, f)
    cat = vn.trim(rs, 1, 10 ** 9)
    assert cat[0] == 0                                   # label 0 is present and qualifies
    np.testing.assert_array_equal(voids.trim_by_volume(lab, 1, 10 ** 9), cat)
    # the thresholded mask of apply_watershed, without merging
    ref, n = vn.watershed(f, vn.inside(f, threshold=0.))
    lab = voids.apply_watershed(d, mask_threshold=0., merge_threshold=0., verbose=False)
    _check_labels(lab, ref, n)
    # everything masked: no region
    lab = voids.watershed(d, mask=np.zeros((N, N, N), dtype=bool))
    assert lab.n_labels == 0 and not np.asarray(lab).any()
    st = voids.region_statistics(lab, d)
    assert st.count.tolist() == [N ** 3]
    assert voids.apply_watershed(d, mask_threshold=float(f.min()) - 1., verbose=False).n_labels == 0
    # NaNs are outside the mask; the statistics skip them in label 0 and refuse them in a region
    g = f.copy()
    g.flat[np.random.RandomState(3).choice(N ** 3, 300, replace=False)] = np.nan
    lab = voids.watershed(g, box=box)
    ref, n = vn.watershed(g, vn.inside(g))
    _check_labels(lab, ref, n)
    _check_stats(voids.region_statistics(lab, g), vn.region_stats(ref, n, g), g)
    with pytest.raises(ValueError):
        voids.region_statistics(voids.watershed(d), g, box=box)
    with pytest.raises(NotImplementedError):
        voids.watershed(d, markers=5)
    with pytest.raises(NotImplementedError):
        voids.apply_watershed(d, markers=np.zeros(4), verbose=False)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,scale", [(32, CUBE), (48, CUBOID), (64, CUBE)])
def test_apply_watershed_merges_as_the_oracle(prec, N, scale):
    box = _box(N, prec, scale, seed=2)
    d = box.realise_density()
    _check_apply_merge(box, d, _stored(box, d))


@pytest.mark.parametrize("prec", PRECS)
def test_256(prec):
    box = _box(256, prec, seed=4)
    d = box.realise_density()
    f = _stored(box, d)
    lab = voids.watershed(d)
    ref, n = vn.watershed(f, vn.inside(f))
    _check_labels(lab, ref, n)
    st = voids.region_statistics(lab, d)
    _check_stats(st, vn.region_stats(ref, n, f), f)
    _same_bits(st, voids.region_statistics(lab, d))
    mth = 0.3 * float(np.std(f))
    out = voids.apply_watershed(d, mask_threshold=0., merge_threshold=mth, verbose=False)
    ref, n = vn.watershed(f, vn.inside(f, threshold=0.))
    # about 10^6 adjacent pairs here: a margin of 1e-9 still leaves the device's means (1e-15 from the oracle's) on the same side
    mref, M = vn.merge(ref, n, vn.region_stats(ref, n, f)["mean"], mth, margin=1e-9)
    _check_labels(out, mref, M)
