"""GPU: every instance of the PCA kernels on the constructed cases of tests/pca_cases.py, through the C entries.

The exact cases carry no tolerance: every sum is exact in any order, so the device must give the bits of the numpy value.
Outputs are pre-filled with NaN, so an element that is not written shows.  The real-valued cases at the end follow the rule of
tests/test_cleaning_gpu.py (device deviation <= 10 delta_ref, floor 1e-12, delta_ref = the reference's own deviation under a
fixed permutation of the pixels), per element of the covariance relative to sqrt(cov_aa cov_bb)."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, _lib
from tests import pca_cases as pc

pytestmark = pytest.mark.gpu
FLOOR = 1e-12


def _box(N, prec):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec)


@functools.lru_cache(maxsize=None)
def _num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _up(eng, x):
    """(npix, N) host matrix -> the device cube in the plan's precision."""
    N = eng.N
    return eng.upload(np.asarray(x).reshape(N, N, N).astype(eng.rdtype), "real")


def _dl(eng, buf, shape, dtype=np.float64):
    h = np.empty(shape, dtype=dtype)
    _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), buf.ptr, h.nbytes, eng.stream)
    eng.sync()
    return h


def _nan(eng, count):
    return eng.upload_raw(np.full(count, np.nan))


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d differ, first at %s: device %r, expected %r" % (
            what, len(bad), got.size, i, got[i], want[i]))


def _cov(eng, cube, mean_buf):
    N = eng.N
    cov_dev = _nan(eng, N * N)
    _lib.call("fb_channel_covariance", eng._plan, cube.ptr, mean_buf.ptr, cov_dev.ptr, eng.stream)
    return _dl(eng, cov_dev, (N, N))


def _set_row(eng, cube, p, spectrum):
    row = np.ascontiguousarray(spectrum, dtype=eng.rdtype)
    _lib.call("fb_memcpy_h2d", cube.ptr + p * row.nbytes, row.ctypes.data_as(ctypes.c_void_p), row.nbytes, eng.stream)
    eng.sync()                                                       # `row` is this call's


def _cases(table, only_f32=(), prec_of=None):
    out = []
    for key, sizes in table.items():
        for N in sizes:
            precs = (prec_of or {}).get(N, ("f32",) if N in only_f32 else ("f64", "f32"))
            out += [pytest.param(key, N, prec, id="%s-%d-%s" % (str(key).replace(" ", "_"), N, prec)) for prec in precs]
    return out


@functools.lru_cache(maxsize=1)
def _cov_expected(N):
    x = pc.int_cube(N)
    return {name: pc.expected_cov(x, mean) for name, mean in pc.mean_vectors(N, x).items()}


# ---- means -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instance,N,prec", _cases(dict(pc.COV_SIZES, large=(512,)), only_f32=pc.F32_ONLY))
def test_channel_means_are_exact(instance, N, prec):
    eng = _box(N, prec).engine
    x = pc.int_cube(N)
    mean_dev, cube = _nan(eng, N), _up(eng, x)
    _lib.call("fb_channel_means", eng._plan, cube.ptr, mean_dev.ptr, eng.stream)
    _same("means", _dl(eng, mean_dev, (N,)), pc.expected_means(x))
    if N <= 160:                                                     # one hot pixel at either end of the cube
        cube = _up(eng, np.zeros((N * N, N)))
        for p in (0, N * N - 1):
            _set_row(eng, cube, p, pc.hot_spectrum(N))
            _lib.call("fb_channel_means", eng._plan, cube.ptr, mean_dev.ptr, eng.stream)
            _same("means, hot pixel %d" % p, _dl(eng, mean_dev, (N,)), pc.hot_spectrum(N) * (1.0 / (N * N)))
            _set_row(eng, cube, p, np.zeros(N))


# ---- covariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instance,N,prec", _cases(pc.COV_SIZES, only_f32=pc.F32_ONLY))
def test_channel_covariance_is_exact(instance, N, prec):
    eng = _box(N, prec).engine
    x = pc.int_cube(N)
    cube = _up(eng, x)
    want = _cov_expected(N)
    for name, mean in pc.mean_vectors(N, x).items():
        mean_buf = eng.upload_raw(mean)
        cov = _cov(eng, cube, mean_buf)
        _same("cov about %s" % name, cov, want[name])
        _same("cov about %s against its transpose" % name, cov, cov.T)
    mean_dev = _nan(eng, N)                                          # the chain as pca_filter runs it
    _lib.call("fb_channel_means", eng._plan, cube.ptr, mean_dev.ptr, eng.stream)
    _same("cov about the device's means", _cov(eng, cube, mean_dev), want["own"])


@pytest.mark.parametrize("instance,N,prec", _cases(pc.COV_SIZES, only_f32=pc.F32_ONLY))
def test_channel_covariance_of_one_hot_pixel(instance, N, prec):
    """cov (npix - 1) = v v^T about zero, wherever the pixel lies in the slices and pipeline groups of the plan."""
    eng = _box(N, prec).engine
    slices, rows = pc.plan(N, _num_cu())
    cube = _up(eng, np.zeros((N * N, N)))
    means = {name: (eng.upload_raw(mean), pc.expected_cov_one_hot(N, mean)) for name, mean in pc.mean_vectors(N).items()}
    positions = pc.hot_positions(N, slices, rows)
    assert len(positions) >= 7 and all(0 <= p < N * N for p in positions.values())
    for where, p in positions.items():
        _set_row(eng, cube, p, pc.hot_spectrum(N))
        for name, (mean_buf, want) in means.items():
            cov = _cov(eng, cube, mean_buf)
            _same("hot pixel %d (%s; %d slices of %d) about %s" % (p, where, slices, rows, name), cov, want)
        _set_row(eng, cube, p, np.zeros(N))


# ---- projection ------------------------------------------------------------------------------------------------------------
def _clean_combos(N):
    names = ("own", "zeros", "quarters")
    if N >= 384:
        return [(0, "own"), (8, "quarters")]
    nms = (0, 1, 3, 8) + ((N,) if N <= 18 else ())
    if N >= 160:
        return [(nm, names[i % 3]) for i, nm in enumerate(nms)]
    return [(nm, name) for nm in nms for name in names]


@pytest.mark.parametrize("cpl,N,prec", _cases(pc.CLEAN_SIZES, prec_of=pc.CLEAN_PREC))
def test_pca_clean_is_exact(cpl, N, prec):
    lanes = 1
    while 64 * lanes < N:
        lanes *= 2
    assert lanes == cpl
    eng = _box(N, prec).engine
    npix = N * N
    x = pc.int_cube(N)
    cube = _up(eng, x)
    means = pc.mean_vectors(N, x)
    for nm, name in _clean_combos(N):
        U = pc.modes(N, nm)
        want, want_amps = pc.expected_clean(x, means[name], U, out_dtype=eng.rdtype)
        mean_buf = eng.upload_raw(means[name])
        U_buf = eng.upload_raw(U) if nm else None                    # nm = 0: a null U
        for with_amps in (True, False):
            out = eng.empty("real")
            if N <= 256:
                blank = np.full(npix * N, np.nan, dtype=eng.rdtype)
                _lib.call("fb_memcpy_h2d", out.ptr, blank.ctypes.data_as(ctypes.c_void_p), blank.nbytes, eng.stream)
                eng.sync()                                           # `blank` is this block's
            amps = _nan(eng, max(1, nm) * npix) if with_amps else None
            _lib.call("fb_pca_clean", eng._plan, cube.ptr, mean_buf.ptr, U_buf.ptr if nm else None, nm, out.ptr,
                      amps.ptr if with_amps else None, eng.stream)
            what = "%d modes about %s, amps %s" % (nm, name, "given" if with_amps else "NULL")
            _same("cleaned, " + what, _dl(eng, out, (npix, N), eng.rdtype), want)
            if with_amps and nm:
                _same("amps, " + what, _dl(eng, amps, (nm, npix)), want_amps)
            del out


# ---- rotated covariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec", [(N, prec) for N in pc.ROTATED_SIZES for prec in pc.ROTATED_PREC.get(N, ("f64", "f32"))])
def test_rotated_covariance_is_exact(N, prec):
    """k_rotate_spectra, then the fp64 covariance about a mean of zeros (the fp64 instance serves both plans)."""
    eng = _box(N, prec).engine
    x = pc.int_cube(N)
    Vt = pc.rotation(N)
    work = eng._alloc_bytes((N * N * N + N) * 8)
    cov_dev, cube, Vt_buf = _nan(eng, N * N), _up(eng, x), eng.upload_raw(Vt)
    _lib.call("fb_rotated_covariance", eng._plan, cube.ptr, Vt_buf.ptr, work.ptr, cov_dev.ptr, eng.stream)
    cov = _dl(eng, cov_dev, (N, N))
    _same("rotated covariance", cov, _rotated_expected(N))
    _same("rotated covariance against its transpose", cov, cov.T)


@functools.lru_cache(maxsize=1)
def _rotated_expected(N):
    return pc.expected_rotated(pc.int_cube(N), pc.rotation(N))


# ---- NNDSVD rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", pc.NNDSVD_SIZES)
def test_nndsvd_norms_and_fill_are_exact(N, prec):
    eng = _box(N, prec).engine
    npix = N * N
    fill = -3.5
    for k in (1, 5, 16):
        W = pc.nndsvd_rows(k, npix)
        norms = np.full(2 * k, np.nan)
        W_buf = eng.upload_raw(W)
        _lib.call("fb_nndsvd_norms", eng._plan, W_buf.ptr, k, norms.ctypes.data_as(_lib.P_double), eng.stream)
        _same("norms, k = %d" % k, norms, pc.expected_norms(W))
        W2, coef = pc.nndsvd_fill_rows(k, npix), pc.nndsvd_coef(k)
        for abs_first in (0, 1):
            buf = eng.upload_raw(W2)
            _lib.call("fb_nndsvd_fill", eng._plan, buf.ptr, k, coef.ctypes.data_as(_lib.P_double), abs_first, pc.EPS, fill,
                      eng.stream)
            _same("fill, k = %d, abs_first = %d" % (k, abs_first), _dl(eng, buf, (k, npix)),
                  pc.expected_fill(W2, coef, abs_first, pc.EPS, fill))


# ---- real-valued data ------------------------------------------------------------------------------------------------------
def _foreground_cube(N):
    """The foreground-plus-noise cube of tests/test_generic_grid_gpu.py."""
    rs = np.random.RandomState(N)
    nu = np.linspace(1., 2., N)
    return (40. * nu ** -2.7) * (1. + 0.2 * rs.normal(size=(N, N, 1))) + (3. * nu ** -2.0) * rs.normal(size=(N, N, 1)) \
        + 0.02 * rs.normal(size=(N, N, N))


def _perm(npix):
    return np.random.RandomState(99).permutation(npix)


def _held(eng, N):
    cube = eng.upload(_foreground_cube(N), "real")
    return cube, _dl(eng, cube, (N * N, N), eng.rdtype).astype(np.float64)


@pytest.mark.parametrize("instance,N,prec", [("MA=1", 48, "f64"), ("MA=1 edge", 18, "f32"), ("MA=1 edge, once empty slices", 50, "f64"),
                                             ("MA=2", 96, "f32"), ("MA=4", 128, "f64")])
def test_channel_covariance_on_foreground_data(instance, N, prec):
    eng = _box(N, prec).engine
    cube, held = _held(eng, N)
    npix = N * N
    mean = held.mean(axis=0)

    def ref(h):
        d = h - mean
        return (d.T @ d) / (npix - 1.)
    want, alt = ref(held), ref(held[_perm(npix)])
    mean_buf = eng.upload_raw(mean)
    got = _cov(eng, cube, mean_buf)
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))          # per element: its two rows' scale
    dev, dref = float(np.max(np.abs(got - want) / scale)), float(np.max(np.abs(alt - want) / scale))
    print("covariance %s N = %d %s: device deviation %.3e, delta_ref %.3e" % (instance, N, prec, dev, dref))
    assert dev <= max(10. * dref, FLOOR), "device deviation %.3e, delta_ref %.3e" % (dev, dref)
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("cpl,N,prec", [(1, 18, "f64"), (2, 80, "f32"), (4, 160, "f64"), (8, 384, "f32")])
def test_pca_clean_on_foreground_data(cpl, N, prec):
    eng = _box(N, prec).engine
    cube, held = _held(eng, N)
    npix, nm = N * N, 3
    mean = held.mean(axis=0)
    d = held - mean
    U = np.ascontiguousarray(np.linalg.eigh((d.T @ d) / (npix - 1.))[1][:, ::-1][:, :nm])

    def ref(dd):
        A = dd @ U
        return dd - A @ U.T, A.T
    want, want_amps = ref(d)
    pm = _perm(npix)
    alt, alt_amps = ref(d[pm])
    inv = np.argsort(pm)
    alt, alt_amps = alt[inv], alt_amps[:, inv]
    out, amps, mean_buf, U_buf = eng.empty("real"), eng._alloc_bytes(nm * npix * 8), eng.upload_raw(mean), eng.upload_raw(U)
    _lib.call("fb_pca_clean", eng._plan, cube.ptr, mean_buf.ptr, U_buf.ptr, nm, out.ptr, amps.ptr, eng.stream)
    got, got_amps = _dl(eng, out, (npix, N), eng.rdtype).astype(np.float64), _dl(eng, amps, (nm, npix))
    xmax = float(np.max(np.abs(held)))
    dref = float(np.max(np.abs(alt - want)) / xmax)
    bound = 10. * max(dref, FLOOR / 10.) * xmax + (4. * 2. ** -24 * np.abs(want) if prec == "f32" else 0.)
    err = np.abs(got - want)
    print("pca_clean cpl = %d N = %d %s: device deviation %.3e (relative to max|X|), delta_ref %.3e" % (
        cpl, N, prec, float(err.max()) / xmax, dref))
    assert np.all(err <= bound), "cleaned: device deviation %.3e (relative to max|X|), delta_ref %.3e, largest excess %.3e" % (
        float(err.max()) / xmax, dref, float((err - bound).max()))
    amax = float(np.max(np.abs(want_amps)))
    adev, adref = float(np.max(np.abs(got_amps - want_amps)) / amax), float(np.max(np.abs(alt_amps - want_amps)) / amax)
    print("pca_clean amps: device deviation %.3e, delta_ref %.3e" % (adev, adref))
    assert adev <= max(10. * adref, FLOOR), "amps: device deviation %.3e, delta_ref %.3e" % (adev, adref)
