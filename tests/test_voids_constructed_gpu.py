"""GPU: the void kernels (fb_voids.hip) on the constructed cases of tests/void_cases.py and on grids whose N^3 is no multiple of
256, in both precisions, against the numpy statement of tests/voids_numpy.py.  Fields and labels go in as host arrays; nothing
here depends on the generator.  What each case is for, and the properties that keep it from being vacuous, are asserted on the
CPU by tests/test_void_cases_cpu.py."""
import functools

import numpy as np
import pytest

from fastbox_amd import voids
from fastbox_amd.device import REAL
from tests import void_cases as vc
from tests import voids_numpy as vn
from tests.test_voids_gpu import (CUBE, CUBOID, PRECS, _box, _check_apply_merge, _check_chain, _check_labels, _check_stack,
                                  _check_stats, _same_bits, _stored)

pytestmark = pytest.mark.gpu
N0 = 32
NLAB = 7


@functools.lru_cache(maxsize=None)
def _cached_box(N, prec, scale=CUBE):
    return _box(N, prec, scale)


def _smooth_gaussian(N, seed, sigma=0.8):
    """A seeded host Gaussian field smoothed over ``sigma`` voxels, unit variance."""
    f = np.random.RandomState(seed).normal(size=(N, N, N))
    g = np.exp(-2. * np.pi ** 2 * sigma ** 2 * np.fft.fftfreq(N) ** 2)
    f = np.fft.ifftn(np.fft.fftn(f) * g[:, None, None] * g[None, :, None] * g[None, None, :]).real
    return f / np.std(f)


def _device_labels(box, lab, n_labels):
    return voids.VoidLabels(box.engine, box.engine.upload_raw(np.ascontiguousarray(lab, dtype=np.int32)), n_labels)


# ---- grids with N % 4 == 2: every tail guard and the x / y edges of the watershed tile ------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,scale", [(18, CUBE), (18, CUBOID), (30, CUBE), (30, CUBOID)])
def test_odd_sized_grid_chain_and_merge(prec, N, scale):
    assert N % 4 == 2 and N ** 3 % 256 != 0
    box = _cached_box(N, prec, scale)
    f = _stored(box, _smooth_gaussian(N, 100 + N))
    n = _check_chain(box, f, f, scale, grid_pixes=(7, 15))
    assert 5 <= N ** 3 / n <= 50                                    # regions of 5-50 voxels on average
    _check_apply_merge(box, f, f)


# ---- the watershed on the builders -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corridor_reference(N):
    f, ins, length = vc.corridor(N)
    ref, n = vn.watershed(f, vn.inside(f, mask=ins))
    ref.setflags(write=False)
    return f, ins, length, ref, n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [18, 32])
def test_watershed_corridor(prec, N):
    box = _cached_box(N, prec)
    f, ins, length, ref, n = _corridor_reference(N)
    assert n == 1 and int((ref == 1).sum()) == length
    outside = np.where(ins, f, np.nan)                              # no mask: NaN is outside
    for lab in (voids.watershed(outside, box=box), voids.watershed(f, mask=ins, box=box),
                voids.watershed(f, mask=box.engine.upload(ins.astype(np.float64), REAL), box=box)):
        _check_labels(lab, ref, n)
        assert lab.n_labels == 1 and int((np.asarray(lab) == 1).sum()) == length
    st = voids.region_statistics(voids.watershed(f, mask=ins, box=box), f)
    _check_stats(st, vn.region_stats(ref, n, f), f)
    assert st.argmin[1] == int(np.argmin(np.where(ins, f, np.inf)))  # the end of the corridor


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["checkerboard", "constant", "constant_zero", "signed_zeros", "ramp"])
def test_watershed_builders(prec, name):
    N = N0
    box = _cached_box(N, prec)
    f = {"checkerboard": vc.checkerboard, "constant": lambda n: vc.constant(n, -1.25), "constant_zero": lambda n: vc.constant(n, 0.),
         "signed_zeros": vc.signed_zeros, "ramp": vc.ramp}[name](N)
    ref, n = vn.watershed(f, vn.inside(f))
    assert n == (N ** 3 // 2 if name == "checkerboard" else 1)
    lab = voids.watershed(f, box=box)
    _check_labels(lab, ref, n)
    st = voids.region_statistics(lab, f)
    rs = vn.region_stats(ref, n, f)
    _check_stats(st, rs, f)
    np.testing.assert_array_equal(st.sum, rs["sum"])                 # small integers and quarters: exact
    if n == 1:
        assert st.argmin[1] == 0                                     # the least index of the plateau; -0 is +0


@pytest.mark.parametrize("prec", PRECS)
def test_watershed_masks(prec):
    N = N0
    box = _cached_box(N, prec)
    rs = np.random.RandomState(12)
    f = _stored(box, _smooth_gaussian(N, 3))
    # a device-field mask with -0.0 (outside) and NaN (inside, as != 0 says)
    m = rs.randint(0, 2, size=(N, N, N)).astype(np.float64)
    k = rs.permutation(N ** 3)
    m.flat[k[:2000]] = -0.0
    m.flat[k[2000:4000]] = np.nan
    ins = vn.inside(f, mask=m)
    assert not ins.flat[k[:2000]].any() and ins.flat[k[2000:4000]].all()
    ref, n = vn.watershed(f, ins)
    _check_labels(voids.watershed(f, mask=box.engine.upload(m, REAL), box=box), ref, n)
    # +inf, -inf and NaN side by side: all outside, whatever their order
    g = f.copy()
    for v, sel in zip((np.inf, -np.inf, np.nan), (k[4000:4500], k[4500:5000], k[5000:5500])):
        g.flat[sel] = v
    g[5, 5, 5:8] = (np.inf, np.nan, -np.inf)
    g[N - 1, N - 1, N - 3:] = (-np.inf, np.inf, np.nan)
    ref, n = vn.watershed(g, vn.inside(g))
    lab = voids.watershed(g, box=box)
    _check_labels(lab, ref, n)
    assert not np.asarray(lab)[~np.isfinite(g)].any()
    # the threshold is compared in fp64: float32(0.1) lies above 0.1 and is outside, its predecessor is inside
    above = np.float32(0.1)
    below = np.nextafter(above, np.float32(0.))
    assert float(above) > 0.1 > float(below)
    h = f.copy()
    h.flat[k[6000:7000]] = float(above)
    h.flat[k[7000:8000]] = float(below)
    assert np.array_equal(_stored(box, h), h)
    ref, n = vn.watershed(h, vn.inside(h, threshold=0.1))
    assert not ref.flat[k[6000:7000]].any() and ref.flat[k[7000:8000]].all()
    out = voids.apply_watershed(h, mask_threshold=0.1, merge_threshold=0., verbose=False, box=box)
    _check_labels(out, ref, n)
    # f == t exactly is inside
    h.flat[k[6000:8000]] = 0.5
    ref, n = vn.watershed(h, vn.inside(h, threshold=0.5))
    assert ref.flat[k[6000:8000]].all() and (ref == 0).any()
    _check_labels(voids.apply_watershed(h, mask_threshold=0.5, merge_threshold=0., verbose=False, box=box), ref, n)


# ---- statistics on striped labels ------------------------------------------------------------------------------------------------
def _check_exact(st, rs):
    for k in ("sum", "weight_sum", "weighted_index_sum", "mean"):     # assert_array_equal: NaN equals NaN in the same place
        np.testing.assert_array_equal(getattr(st, k), rs[k], err_msg=k)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [18, 32])
@pytest.mark.parametrize("run", vc.RUNS)
def test_statistics_on_striped_labels(prec, N, run):
    box = _cached_box(N, prec)
    for zeros, gaps in ((False, False), (True, False), (True, True)):
        lab, nl = vc.striped_labels(N, run, NLAB, zeros=zeros, gaps=gaps)
        dl = _device_labels(box, lab, nl)
        cancel = 11 if gaps else 4
        absent = np.setdiff1d(np.arange(nl + 1), np.unique(lab))
        assert (absent.size > 0) == (gaps or not zeros) and (0 in absent) == (not zeros)
        for field in (vc.dyadic_field(N, run, lab, cancel), np.zeros((N, N, N)), None):
            st = voids.region_statistics(dl, field)
            rs = vn.region_stats(lab, nl, field)
            _check_stats(st, rs, field)
            _same_bits(st, voids.region_statistics(dl, field))
            assert np.all(st.count[absent] == 0)
            if field is None:
                continue
            _check_exact(st, rs)
            assert np.all(st.argmin[absent] == -1) and np.all(np.isnan(st.mean[absent]))
            if field.any():
                assert st.sum[cancel] == 0. and st.weight_sum[cancel] > 0. and (st.sum < 0).any() and (st.sum > 0).any()
                ex = vc.exact_sums(lab, nl, field)
                for k in ex:
                    np.testing.assert_array_equal(getattr(st, k), ex[k], err_msg=k)


@pytest.mark.parametrize("prec", PRECS)
def test_statistics_spike(prec):
    """2^40 beside unit values: the bound's exponent is 41, one fixed-point unit 2^-52, a label's error at most count 2^-52."""
    N = N0
    box = _cached_box(N, prec)
    f, index = vc.spike_field(N, 5)
    lab, nl = vc.striped_labels(N, 65, NLAB)
    lab = lab.copy()
    lab.flat[index] = nl + 1
    nl += 1
    st = voids.region_statistics(lab, f, box=box)
    rs = vn.region_stats(lab, nl, f)
    _check_stats(st, rs, f)
    assert st.sum[nl] == 2.0 ** 40 and st.count[nl] == 1 and st.argmin[nl] == index
    absum = np.bincount(lab.reshape(-1), weights=np.abs(f).reshape(-1), minlength=nl + 1)
    worst = 0.
    for a, b, s in ((st.sum, rs["sum"], absum), (st.weight_sum, rs["weight_sum"], absum),
                    (st.weighted_index_sum, rs["weighted_index_sum"], absum[:, None] * N)):
        with np.errstate(invalid="ignore"):                          # 0 / 0 for the absent label 0
            worst = max(worst, float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * s))))
    print("spike field, %s: largest relative error of a label's sums %.3e" % (prec, worst))


@pytest.mark.parametrize("prec", PRECS)
def test_statistics_error_word(prec):
    """A label below 0 or above n_labels is skipped by every kernel and reported: ValueError, nothing written out of range."""
    N = N0
    box = _cached_box(N, prec)
    lab, nl = vc.striped_labels(N, 65, NLAB)
    f = vc.dyadic_field(N, 1)
    for bad in (-1, nl + 1, 2 ** 31 - 1):
        b = lab.copy()
        b[N // 2, 3, N - 1] = bad
        b[N - 1, N - 1, N - 1] = bad
        for field in (f, None):
            with pytest.raises(ValueError, match="labels outside"):
                voids.region_statistics(_device_labels(box, b, nl), field)
    st = voids.region_statistics(_device_labels(box, lab, nl), f)    # and the next call is sound
    _check_stats(st, vn.region_stats(lab, nl, f), f)


# ---- merging -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("order", vc.ORDERS)
def test_merge_chain(prec, order):
    N = N0
    box = _cached_box(N, prec)
    lab, f, n = vc.chain_labels(N, order)
    mean = vn.region_stats(lab, n, f)["mean"]
    for thr, want in ((1.5, 1), (0., n), (np.inf, 1)):
        ref, M = vn.merge(lab, n, mean, thr)
        assert M == want
        _check_labels(voids.merge_regions(lab, f, thr, box=box), ref, M)
    lab, f, n = vc.chain_labels(N, order, equal_at=n // 2 + 5)       # one interface with |d mean| == threshold: strict <
    mean = vn.region_stats(lab, n, f)["mean"]
    np.testing.assert_array_equal(voids.region_statistics(lab, f, box=box).mean[1:], mean[1:])
    ref, M = vn.merge(lab, n, mean, 1.5)
    assert M == 2
    _check_labels(voids.merge_regions(lab, f, 1.5, box=box), ref, M)


@pytest.mark.parametrize("prec", PRECS)
def test_merge_adjacency(prec):
    """Face neighbours only, no wrap from the end of a row or a plane to the next, no periodic box, and label 0 joins nothing."""
    N = N0
    box = _cached_box(N, prec)
    one = np.ones((N, N, N))
    for lab in (vc.diagonal_labels(N), vc.face_labels(N, 0), vc.face_labels(N, 1), vc.face_labels(N, 2), vc.sheet_labels(N)):
        for thr in (0.5, np.inf):
            _check_labels(voids.merge_regions(lab, one, thr, box=box), lab, 2)
    # the same sheet with a region in place of the 0 does merge
    ref, M = vn.merge(vc.sheet_labels(N) + 1, 3, np.array([np.nan, 1., 1., 1.]), np.inf)
    assert M == 1
    _check_labels(voids.merge_regions(vc.sheet_labels(N) + 1, one, np.inf, box=box), ref, 1)
    # absent labels (count 0, NaN mean) merge with nothing and are counted, as the numpy statement counts them
    lab, nl = vc.striped_labels(N, 65, NLAB, zeros=True, gaps=True)
    f = vc.dyadic_field(N, 2)
    st = voids.region_statistics(_device_labels(box, lab, nl), f)
    mean = vn.region_stats(lab, nl, f)["mean"]
    for thr in (0., np.inf):
        ref, M = vn.merge(lab, nl, mean, thr)
        assert M == (nl if thr == 0. else nl - NLAB + 1)
        _check_labels(voids.merge_regions(st, None, thr), ref, M)


# ---- stacking ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_stacking_linear_field(prec):
    """Label 1 everywhere and f = a x + b y + c z + d: the stacked value is the field at c_v + R (grid[b], grid[a], grid[c])."""
    N = N0
    box = _cached_box(N, prec, CUBOID)
    coef = (3., -5., 7., 11.)
    f = _stored(box, vc.linear_field(coef, box))
    lab = np.ones((N, N, N), dtype=np.int32)
    cen = np.array([[400., 0., 0.], [450., -200., 100.], [300., 0., 600.]])
    rad = np.array([200., 150., 300.])
    scale = np.max(np.abs(f))
    tol = (1e-12 + (2. ** -24 if prec == "f32" else 0.)) * scale
    for pix in (1, 7):
        stk, fail, cnt = voids.stack_voids_at([1, 1, 1], lab, box, f, cen, rad, grid_pix=pix)
        want, wcnt = vc.linear_stack(coef, cen, rad, box, 1., pix)
        np.testing.assert_array_equal(cnt, wcnt)
        assert fail == []
        m = cnt > 0
        assert m.any() and np.array_equal(np.ma.getmaskarray(stk), ~m)
        assert np.max(np.abs(stk.data[m] - want[m])) <= tol
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 3).any()


@pytest.mark.parametrize("prec", PRECS)
def test_stacking_cases(prec):
    N = N0
    box = _cached_box(N, prec, CUBOID)
    f = _stored(box, vc.linear_field((3., -5., 7., 11.), box) + _smooth_gaussian(N, 8))
    lab = np.ones((N, N, N), dtype=np.int32)
    lab[N - 1, N - 1, N - 1] = 3                                     # label 2 is absent, label 3 has no whole cell
    rs = np.random.RandomState(21)
    nv = 130
    half = 0.5 * np.array(CUBOID)
    cen = rs.uniform(-1.1, 1.1, size=(nv, 3)) * half                 # some outside the box, many with part of the grid outside
    rad = rs.uniform(0., 300., size=nv)
    cat = np.ones(nv, dtype=np.int64)
    cat[3], cat[70] = 2, 3                                           # absent, and present without a valid point: failures
    cen[5] = cen[4]                                                  # a void listed twice
    rad[5] = rad[4]
    cen[6, 1] = np.nan                                               # a NaN centre: a failure
    cen[7], rad[7] = (10., 20., 30.), 0.                             # R = 0: every grid point is the centre
    x0, dx = vn.axes(box)
    edges = []                                                       # (void, valid): u == N - 2 and the double below N - 1 are
    for axis in range(3):                                            # valid, u == N - 1 is not
        for k in (N - 2, N - 1):
            below, at = vc.edge_u(box, axis, k)
            assert (at - x0[axis]) / dx[axis] == k or axis == 1      # exact on x and z; on y the least u above N - 1
            for coord, valid in ((at, k == N - 2), (below, True)):
                v = 8 + len(edges)
                cen[v], rad[v] = (0., 0., 0.), 0.
                cen[v, axis] = coord
                edges.append((v, valid))
    cen[64:66] = cen[8:10]                                           # and again where a chunk of voids ends
    rad[64:66] = 0.
    for n in (0, 65, 130):
        for pix in (1, 7):
            stk, fail, cnt = voids.stack_voids_at(cat[:n], lab, box, f, cen[:n], rad[:n], grid_pix=pix)
            o, ofail, ocnt = vn.stack(lab, f, cat[:n], cen[:n], rad[:n], box, 1., pix)
            _check_stack(stk, fail, cnt, o, ofail, ocnt)
            if n == 0:
                assert fail == [] and np.ma.getmaskarray(stk).all()
            else:
                assert {1, 2} <= set(ofail) and len(ofail) >= 5 and (ocnt > 0).any() and ocnt.max() < n
    # the single voids: exactly at the last cell, exactly past it, just before it; the repeated one
    for v, valid in edges:
        _, fail, cnt = voids.stack_voids_at([1], lab, box, f, cen[v:v + 1], rad[v:v + 1], grid_pix=1)
        assert int(cnt[0, 0, 0]) == (1 if valid else 0) and fail == ([] if valid else [1]), v
    a, _, ca = voids.stack_voids_at([1], lab, box, f, cen[4:5], rad[4:5], grid_pix=7)
    b, _, cb = voids.stack_voids_at([1, 1], lab, box, f, cen[4:6], rad[4:6], grid_pix=7)
    np.testing.assert_array_equal(cb, 2 * ca)
    np.testing.assert_array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b))
    np.testing.assert_allclose(b.compressed(), a.compressed(), rtol=1e-15)
