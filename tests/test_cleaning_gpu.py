"""GPU: filters.nmf_filter, ica_filter and bandpower_pca_filter against their numpy statements (tests/cleaning_numpy.py).

Tolerances of the fp64 quantities are not fixed in advance: the statement is run on the pixels in natural order and on a fixed
permutation of them, which changes the summation order only; that deviation is delta_ref, and the device (whose tree sums are
one more reordering) must lie within 10 delta_ref, with a floor of 1e-12, all relative to the largest magnitude of the
quantity.  A cube stored in fp32 has the bound 4 2^-24 |cleaned| + 10 delta_ref max|X| per element.  Every assertion message
carries the measured deviation."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, filters
from tests import cleaning_numpy as cn

pytestmark = pytest.mark.gpu
FLOOR = 1e-12


@functools.lru_cache(maxsize=None)
def _host_cube(N, prec, ncomp=3):
    c = cn.build_cube(N, ncomp=ncomp)
    if prec == "f32":
        c = c.astype(np.float32).astype(np.float64)          # what the device stores
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _perm(npix):
    return np.random.RandomState(99).permutation(npix)


def _box(N, prec):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _within(what, got, want, alt):
    """got against want, given the statement's own reordering deviation |alt - want|."""
    dref, dev = _rel(alt, want), _rel(got, want)
    assert dev <= max(10. * dref, FLOOR), "%s: device deviation %.3e, delta_ref %.3e" % (what, dev, dref)


def _cube_within(what, got, want, alt, xmax, prec):
    dref = float(np.max(np.abs(alt - want)) / xmax)
    bound = 10. * max(dref, FLOOR / 10.) * xmax + (4. * 2. ** -24 * np.abs(want) if prec == "f32" else 0.)
    err = np.abs(np.asarray(got) - want)
    assert np.all(err <= bound), "%s: device deviation %.3e (relative to max|X|), delta_ref %.3e, largest excess %.3e" % (
        what, float(err.max()) / xmax, dref, float((err - bound).max()))


def _nmf_init(N, k):
    rs = np.random.RandomState(5)
    return rs.uniform(0.1, 1., size=(N * N, k)), rs.uniform(0.1, 1., size=(k, N))


@functools.lru_cache(maxsize=None)
def _nmf_ref(N, k, prec, ncomp, custom, tol, max_iter):
    """The statement in natural order and on permuted pixels (W un-permuted, cleaned un-permuted)."""
    X = cn.as_matrix(_host_cube(N, prec, ncomp))
    W0, H0 = _nmf_init(N, k) if custom else (None, None)
    a = cn.nmf(X, k, W0, H0, tol, max_iter)
    pm = _perm(N * N)
    b = cn.nmf(X[pm], k, None if W0 is None else W0[pm], H0, tol, max_iter)
    inv = np.argsort(pm)
    b["W"], b["cleaned"] = b["W"][inv], b["cleaned"][inv]
    return a, b


# 128: two channels per lane, the first size at which the kernels that hold a spectrum in registers take another instance
NMF_FIXED = [(16, 3, "f64", 3), (16, 1, "f32", 3), (24, 5, "f64", 5), (32, 16, "f32", 16), (64, 3, "f32", 3), (64, 16, "f64", 3),
             (128, 3, "f32", 3), (128, 5, "f64", 5)]


@pytest.mark.parametrize("N,k,prec,ncomp", NMF_FIXED)
def test_nmf_five_iterations_match_the_statement(N, k, prec, ncomp):
    a, b = _nmf_ref(N, k, prec, ncomp, True, 0., 5)
    box = _box(N, prec)
    W0, H0 = _nmf_init(N, k)
    cleaned, res = filters.nmf_filter(_host_cube(N, prec, ncomp), k, return_filter=True, box=box, init="custom", W=W0, H=H0,
                                      tol=0., max_iter=5)
    assert res.n_iter_ == 5 == a["n_iter"]
    _within("W", res.W_host(), a["W"], b["W"])
    _within("H", res.components_, a["H"], b["H"])
    va = np.array(a["viols"])                                   # every iteration's pair relative to itself
    _within("violations", np.array(res.violations) / va, np.ones_like(va), np.array(b["viols"]) / va)
    _within("reconstruction_err_", res.reconstruction_err_, a["err"], b["err"])
    X = cn.as_matrix(_host_cube(N, prec, ncomp))
    _cube_within("cleaned", np.asarray(cleaned).reshape(X.shape), a["cleaned"], b["cleaned"], X.max(), prec)


NMF_CONVERGED = [(16, 3, "f64", 3, True), (24, 1, "f32", 3, True), (32, 3, "f32", 3, True), (64, 3, "f64", 3, True),
                 (24, 5, "f64", 5, False), (32, 5, "f32", 5, False), (64, 5, "f32", 5, False), (32, 4, "f64", 5, False),
                 (128, 5, "f64", 5, False)]


@pytest.mark.parametrize("N,k,prec,ncomp,custom", NMF_CONVERGED)
def test_nmf_default_tolerances(N, k, prec, ncomp, custom):
    """custom: a given start; otherwise the default initialisation against the statement's exact-SVD NNDSVDA.

    The fourth and fifth singular directions of the five-component cubes lie in the noise and are nearly degenerate, so these
    cases hold only if the device's singular vectors are as good as those of a decomposition of X itself: with V taken from
    the Gram matrix X^T X alone W deviated by 6e-6 .. 5e-1.  Measured on the MI355X with the corrected V (fb_rotated_covariance):
    DESIGN.md section 4."""
    a, b = _nmf_ref(N, k, prec, ncomp, custom, 1e-4, 200)
    ratio = sum(a["viols"][-1]) / sum(a["viols"][0])
    assert a["n_iter"] < 200 and ratio <= 0.5e-4, "the statement's stop is borderline (%.3e): n_iter_ is not comparable" % ratio
    box = _box(N, prec)
    kw = {}
    if custom:
        W0, H0 = _nmf_init(N, k)
        kw = dict(init="custom", W=W0, H=H0)
    cleaned, res = filters.nmf_filter(_host_cube(N, prec, ncomp), k, return_filter=True, box=box, **kw)
    assert res.n_iter_ == a["n_iter"], (res.n_iter_, a["n_iter"], res.violations, a["viols"])
    W, H = res.W_host(), res.components_
    assert W.min() >= 0. and H.min() >= 0.
    _within("W", W, a["W"], b["W"])
    _within("H", H, a["H"], b["H"])
    X = cn.as_matrix(_host_cube(N, prec, ncomp))
    _cube_within("cleaned", np.asarray(cleaned).reshape(X.shape), a["cleaned"], b["cleaned"], X.max(), prec)
    only = filters.nmf_filter(_host_cube(N, prec, ncomp), k, box=box, **kw)
    assert np.array_equal(np.asarray(only), np.asarray(cleaned))


@pytest.mark.parametrize("N,k,prec", [(24, 3, "f64"), (64, 5, "f32")])
def test_nmf_error_does_not_increase_and_runs_repeat_bitwise(N, k, prec):
    box = _box(N, prec)
    cube = box.engine.upload(_host_cube(N, prec), "real")
    W0, H0 = _nmf_init(N, k)
    errs, last, seen = [], None, set()
    for it in (1, 2, 3, 4, 4):
        cleaned, res = filters.nmf_filter(cube, k, return_filter=True, init="custom", W=W0, H=H0, tol=0., max_iter=it)
        errs.append(res.reconstruction_err_)
        state = (np.asarray(cleaned).tobytes(), res.W_host().tobytes(), res.components_.tobytes(), res.reconstruction_err_,
                 tuple(res.violations))
        if it in seen:                                          # the second run of four iterations
            assert state == last, "two runs differ"
        seen.add(it)
        last = state
    assert all(errs[i + 1] <= errs[i] * (1. + 1e-14) for i in range(3)), errs
    r1 = filters.nmf_filter(cube, k, return_filter=True)
    r2 = filters.nmf_filter(cube, k, return_filter=True)
    assert np.asarray(r1[0]).tobytes() == np.asarray(r2[0]).tobytes() and r1[1].W_host().tobytes() == r2[1].W_host().tobytes()
    assert r1[1].n_iter_ == r2[1].n_iter_ and r1[1].components_.tobytes() == r2[1].components_.tobytes()


def test_nmf_refuses_bad_input():
    N = 16
    box = _box(N, "f32")
    good = np.array(_host_cube(N, "f32"))
    for k in (0, 17):
        with pytest.raises(ValueError):
            filters.nmf_filter(good, k, box=box)
    bad = good.copy()
    bad[3, 5, 7] = -1e-3
    with pytest.raises(ValueError):
        filters.nmf_filter(bad, 3, box=box)
    for v in (np.nan, np.inf):
        bad = good.copy()
        bad[N - 1, N - 1, N - 1] = v
        with pytest.raises(ValueError):
            filters.nmf_filter(bad, 3, box=box)
    with pytest.raises(ValueError):
        filters.nmf_filter(good, 3, box=box, init="nndsvd")
    W0, H0 = _nmf_init(N, 3)
    with pytest.raises(ValueError):
        filters.nmf_filter(good, 3, box=box, init="custom", W=W0)
    with pytest.raises(ValueError):
        filters.nmf_filter(good, 3, box=box, init="custom", W=W0[:-1], H=H0)
    from fastbox_amd import _lib
    eng = box.engine
    cube = eng.upload(good, "real")
    buf = eng._alloc_bytes(17 * N * N * 8)
    v = np.empty(2)
    with pytest.raises(_lib.FastBoxError) as e:
        _lib.call("fb_nmf_sweep", eng._plan, cube.ptr, buf.ptr, buf.ptr, 17, v.ctypes.data_as(_lib.P_double), eng.stream)
    assert e.value.code == -1                                  # FB_ERR_INVALID


# ---- ICA ----------------------------------------------------------------------------------------------------------------------
def _w_init(n):
    return np.random.RandomState(3).normal(size=(n, n))


@functools.lru_cache(maxsize=None)
def _ica_ref(N, n, prec, ncomp, fun, tol, max_iter):
    X = cn.as_matrix(_host_cube(N, prec, ncomp))
    a = cn.fastica(X, n, fun=fun, w_init=_w_init(n), tol=tol, max_iter=max_iter)
    pm = _perm(N * N)
    b = cn.fastica(X[pm], n, fun=fun, w_init=_w_init(n), tol=tol, max_iter=max_iter)
    b["sources"] = b["sources"][:, np.argsort(pm)]
    return a, b


ICA_FIXED = [(16, 1, "f64", 3, "logcosh"), (24, 5, "f32", 5, "exp"), (32, 16, "f64", 16, "cube"), (64, 3, "f32", 3, "logcosh"),
             (64, 16, "f64", 16, "logcosh")]


@pytest.mark.parametrize("N,n,prec,ncomp,fun", ICA_FIXED)
def test_ica_five_iterations_match_the_statement(N, n, prec, ncomp, fun):
    a, b = _ica_ref(N, n, prec, ncomp, fun, 0., 5)
    box = _box(N, prec)
    _, res = filters.ica_filter(_host_cube(N, prec, ncomp), n, return_filter=True, box=box, fun=fun, w_init=_w_init(n), tol=0.,
                                max_iter=5)
    assert res.n_iter_ == 5 == a["n_iter_"]
    _within("W K", res.unmixing_, a["unmixing"], b["unmixing"])
    _within("whitening_", res.whitening_, a["whitening_"], b["whitening_"])


ICA_CONVERGED = [(32, 3, "f64", 3, "logcosh"), (32, 3, "f64", 3, "exp"), (32, 3, "f64", 3, "cube"), (16, 3, "f32", 3, "logcosh"),
                 (64, 3, "f32", 3, "logcosh"), (64, 5, "f64", 5, "exp"), (24, 5, "f64", 5, "cube")]


@pytest.mark.parametrize("N,n,prec,ncomp,fun", ICA_CONVERGED)
def test_ica_default_settings(N, n, prec, ncomp, fun):
    a, b = _ica_ref(N, n, prec, ncomp, fun, 1e-4, 200)
    assert a["n_iter_"] < 200 and a["lims"][-1] <= 0.5e-4, "the statement's stop is borderline (%.3e)" % a["lims"][-1]
    box = _box(N, prec)
    cube = box.engine.upload(_host_cube(N, prec, ncomp), "real")
    cleaned, res = filters.ica_filter(cube, n, return_filter=True, fun=fun, w_init=_w_init(n))
    assert res.n_iter_ == a["n_iter_"], (res.n_iter_, a["n_iter_"], res.lims, a["lims"])
    _within("components_", res.components_, a["components_"], b["components_"])
    _within("mixing_", res.mixing_, a["mixing_"], b["mixing_"])
    _within("mean_", res.mean_, a["mean_"], b["mean_"])
    _within("sources", res.sources_host().T, a["sources"], b["sources"])
    # the cleaned cube is pca_filter's: the same kernel on the same modes
    pca = np.asarray(filters.pca_filter(cube, n))
    assert np.array_equal(np.asarray(cleaned), pca)
    assert np.array_equal(np.asarray(filters.ica_filter(cube, n, fun=fun)), pca)
    # two runs repeat bitwise
    _, again = filters.ica_filter(cube, n, return_filter=True, fun=fun, w_init=_w_init(n))
    assert again.components_.tobytes() == res.components_.tobytes() and again.n_iter_ == res.n_iter_
    assert again.sources_host().tobytes() == res.sources_host().tobytes()


def test_ica_random_state_draws_w_init_as_scikit_learn_does():
    N, n = 16, 3
    box = _box(N, "f64")
    cube = box.engine.upload(_host_cube(N, "f64"), "real")
    _, r1 = filters.ica_filter(cube, n, return_filter=True, random_state=3)
    _, r2 = filters.ica_filter(cube, n, return_filter=True, w_init=_w_init(n))
    assert r1.components_.tobytes() == r2.components_.tobytes()
    with pytest.raises(ValueError):
        filters.ica_filter(cube, n, return_filter=True, w_init=np.eye(4))


# ---- band-power PCA -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bandpower_ref(N, prec, nbands, modes):
    """The statement on the cube as it is, and on the cube with x and y exchanged and both reversed (undone afterwards): a fixed
    permutation of the pixels under which the filter is unchanged in exact arithmetic -- the mask depends on |k| alone, the PCA on
    no order of the pixels -- so the two differ by the order of the transforms' and the sums' operations only.  The transforms are
    taken in the plan's precision, as the device takes them: for an f32 plan delta_ref is that of fp32 transforms."""
    host = _host_cube(N, prec)
    dtype = np.float32 if prec == "f32" else np.float64
    modes = list(modes) if isinstance(modes, tuple) else modes
    want = cn.bandpower_pca(host, nbands, modes, dtype=dtype)
    turned = np.ascontiguousarray(host.transpose(1, 0, 2)[::-1, ::-1])
    alt = cn.bandpower_pca(turned, nbands, modes, dtype=dtype)[::-1, ::-1].transpose(1, 0, 2)
    return want, alt


@pytest.mark.parametrize("N,prec", [(16, "f64"), (32, "f32"), (24, "f64")])
@pytest.mark.parametrize("nbands,modes", [(1, 2), (3, 2), (3, (3, 2, 1))])
def test_bandpower_pca_filter(N, prec, nbands, modes):
    """Within 10 delta_ref of the statement (floor 1e-12, relative to max|X|), an fp32 cube with 4 2^-24 |cleaned| besides."""
    box = _box(N, prec)
    host = _host_cube(N, prec)
    cube = box.engine.upload(host, "real")
    want, alt = _bandpower_ref(N, prec, nbands, modes)
    modes = list(modes) if isinstance(modes, tuple) else modes
    got = filters.bandpower_pca_filter(cube, nbands, modes)
    _cube_within("band-power cleaned", np.asarray(got), want, alt, host.max(), prec)
    if nbands == 1:
        _, edges = cn.band_edges(N, 1)
        band = filters.angular_bandpass_filter(filters.mean_spectrum_filter(cube), edges[0], edges[1])
        real = box.engine.upload(np.asarray(band).real, "real")
        direct = filters.pca_filter(real, modes)
        assert np.array_equal(np.asarray(got), np.asarray(direct))
    with pytest.raises(AssertionError):
        filters.bandpower_pca_filter(cube, nbands, [1] * (nbands + 1))
