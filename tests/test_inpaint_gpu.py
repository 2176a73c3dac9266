"""GPU: fastbox_amd.inpaint and analysis.replace_nan_with_channel_mean against their numpy statements (tests/inpaint_numpy.py).

Tolerances are not fixed in advance.  The statement is evaluated with np.linalg.solve and through eigh of A_p; that deviation,
relative to the largest magnitude of the realisation, is delta_ref.  A device value may differ from the statement by
10 delta_ref (floor 1e-12) times that magnitude, plus the solver's term: the loop stops a line of sight at a residual of
tol |b|, A >= I gives |x - x_exact|_2 <= |b - A x|_2, and s = S^(1/2) x, so every element of that line of sight may be off by
|S^(1/2)|_2 tol |b_p|_2; plus 4 2^-24 |s| per element stored in fp32.  Every assertion message carries the measured deviation.

The statement costs one dense N x N solve per line of sight, so from N = 64 up it is evaluated on the four constructed lines of
sight and a fixed stride of the others (_rows); finiteness, the reported residual and the iteration counts cover the whole
cube."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

from fastbox_amd import CosmoBox, analysis, default_cosmo, inpaint, rng, _lib
from fastbox_amd.device import REAL
from tests import inpaint_numpy as inp

pytestmark = pytest.mark.gpu
FLOOR = 1e-12
TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inpaint_n16.npz")


def _box(N, prec, rng_="numpy", seed=0):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec, rng=rng_, seed=seed)


def _stored(a, prec):
    """what the device holds of a host array"""
    return a.astype(np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _rows(N):
    npix = N * N
    if N < 64:
        return np.arange(npix)
    return np.unique(np.concatenate([np.arange(8), np.arange(8, npix, npix // 248)]))


@functools.lru_cache(maxsize=None)
def _wiener_ref(N, prec, per_voxel=False, max_flags=None):
    """(rows, statement by solve, delta_ref, |b_p|_2, |S^(1/2)|_2) of a case's Wiener mean on the data the device stores"""
    c = inp.build_case(N, per_voxel, max_flags)
    rows = _rows(N)
    d = np.where(c["w"][rows] != 0., _stored(c["d"][rows], prec), 0.)
    var = _stored(c["var"][rows], prec) if per_voxel else c["var"]
    a = inp.statement(d, c["w"][rows], c["S"], var)
    b = inp.statement(d, c["w"][rows], c["S"], var, via="eigh")
    bnorm = np.linalg.norm(inp.rhs(d, c["w"][rows], c["S"], var)[0], axis=1)
    dref = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
    return rows, a, dref, bnorm, float(np.linalg.norm(inp.sqrt_psd(c["S"]), 2))


def _check(what, got, want, dref, bnorm, snorm, prec, tol=TOL):
    """got, want: (rows, N)"""
    big = float(np.max(np.abs(want)))
    bound = 10. * max(dref, FLOOR / 10.) * big + (snorm * tol * bnorm)[:, None] + (4. * 2. ** -24 * np.abs(want) if prec == "f32" else 0.)
    err = np.abs(got - want)
    assert np.all(err <= bound), "%s: device deviation %.3e (relative to max|s|), delta_ref %.3e, solver term %.3e, largest excess %.3e" % (
        what, float(err.max()) / big, dref, float((snorm * tol * bnorm).max()) / big, float((err - bound).max()))


# ---- 1. the product ---------------------------------------------------------------------------------------------------------------
def _matmul(eng, M, X_dev_ptr, kind, pre, post, add):
    N = eng.N
    bufs = [eng.upload_raw(np.ascontiguousarray(a)) if a is not None else None for a in (pre, post, add)]
    Y, Mbuf = eng._alloc_bytes(N ** 3 * 8), eng.upload_raw(np.ascontiguousarray(M))
    _lib.call("fb_los_matmul", eng._plan, Mbuf.ptr, X_dev_ptr, kind,
              *[b.ptr if b is not None else None for b in bufs], Y.ptr, eng.stream)
    h = np.empty((N * N, N))
    _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), Y.ptr, h.nbytes, eng.stream)
    return h


# 18: a remainder of 2 in the sum; 24: a partial channel tile; 64: the first size without edges; 128: several channel tiles per row
@pytest.mark.parametrize("N,xmode", list(itertools.product((16, 18, 24, 64, 128), ("plan_f32", "plan_f64", "fp64_on_f32"))))
def test_los_matmul_matches_numpy(N, xmode):
    rs = np.random.RandomState(N)
    prec = "f64" if xmode == "plan_f64" else "f32"
    eng = _box(N, prec).engine
    M = rs.standard_normal((N, N))                                   # not symmetric: a transposed operand fails
    X = rs.standard_normal((N * N, N))
    if xmode == "fp64_on_f32":
        xbuf, kind = eng.upload_raw(X), 1
        xptr = xbuf.ptr
    else:
        X = _stored(X, prec)
        xdev, kind = eng.upload(X.reshape(N, N, N), REAL), 0
        xptr = xdev.ptr
    opt = dict(pre=rs.uniform(0.5, 2., size=X.shape), post=rs.uniform(-2., 2., size=X.shape), add=rs.standard_normal(X.shape))
    for use in itertools.product((False, True), repeat=3):
        pre, post, add = [opt[k] if u else None for k, u in zip(("pre", "post", "add"), use)]
        got = _matmul(eng, M, xptr, kind, pre, post, add)
        px = X if pre is None else pre * X
        want = px @ M.T
        bound = 2. * N * 2. ** -53 * (np.abs(px) @ np.abs(M).T)
        if post is not None:
            want, bound = post * want, np.abs(post) * bound
        if add is not None:
            want, bound = want + add, bound + 2. ** -53 * np.abs(add)
        err = np.abs(got - want)
        assert np.all(err <= bound), "pre, post, add = %s: largest error %.3e, largest error / bound %.3f" % (
            use, float(err.max()), float(np.max(err / np.maximum(bound, 1e-300))))


# ---- 2. the Wiener mean ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec,per_voxel", [(16, "f64", False), (18, "f64", False), (24, "f32", False), (64, "f32", False),
                                              (128, "f64", False), (16, "f64", True), (24, "f32", True)])
def test_wiener_mean_matches_the_statement(N, prec, per_voxel):
    c = inp.build_case(N, per_voxel)
    rows, want, dref, bnorm, snorm = _wiener_ref(N, prec, per_voxel)
    box = _box(N, prec)
    noise = c["var"].reshape(N, N, N) if per_voxel else c["var"]
    mean, info = inpaint.wiener_filter_1d(c["d_nan"], c["w"], c["S"], noise, box=box, tol=TOL, return_info=True)
    got = np.asarray(mean).reshape(N * N, N)
    assert np.all(np.isfinite(got)), "%d values are not finite" % int((~np.isfinite(got)).sum())
    assert info.residual <= TOL, "residual %.3e" % info.residual
    assert info.converged == N * N, "%d of %d converged" % (info.converged, N * N)
    _check("Wiener mean", got[rows], want, dref, bnorm, snorm, prec)
    assert np.array_equal(got[3], np.zeros(N))                       # the fully flagged line of sight: the prior mean


# ---- 3. iteration counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,max_flags", [(64, 8), (128, 20)])
def test_iteration_counts_follow_the_number_of_flags(N, max_flags):
    c = inp.build_case(N, False, max_flags)
    rows, want, dref, bnorm, snorm = _wiener_ref(N, "f64", False, max_flags)
    box = _box(N, "f64")
    mean, info = inpaint.wiener_filter_1d(c["d_nan"], c["w"], c["S"], c["var"], box=box, tol=TOL, return_info=True)
    n_iter = info.n_iter_host().reshape(-1)
    k = c["nflag"]
    excess = n_iter - (k + 1)
    assert np.all(excess[k < N] <= 2), "largest n_iter - (k + 1): %d" % int(excess[k < N].max())
    assert np.all(n_iter[k == 0] == 1), "unflagged lines of sight took %s iterations" % np.unique(n_iter[k == 0])
    assert n_iter[3] == 0 and np.array_equal(np.asarray(mean).reshape(N * N, N)[3], np.zeros(N))
    assert info.max_iter_ == n_iter.max() and info.converged == N * N and info.residual <= TOL, (info.max_iter_, info.converged, info.residual)
    _check("preconditioned", np.asarray(mean).reshape(N * N, N)[rows], want, dref, bnorm, snorm, "f64")
    plain, info2 = inpaint.wiener_filter_1d(c["d_nan"], c["w"], c["S"], c["var"], box=box, tol=TOL, precondition=False, return_info=True)
    _check("plain CG", np.asarray(plain).reshape(N * N, N)[rows], want, dref, bnorm, snorm, "f64")
    assert info2.residual <= TOL and info2.converged == N * N, (info2.residual, info2.converged)
    assert info2.max_iter_ > info.max_iter_, "plain CG %d iterations, preconditioned %d" % (info2.max_iter_, info.max_iter_)


# ---- 4. draw parity with the reference ---------------------------------------------------------------------------------------------
def test_numpy_draws_reproduce_the_reference():
    g = np.load(GOLDEN)
    N = 16
    d, w, S, var, cr = g["d"], g["w"].astype(np.float64), g["S"], g["var"], g["cr"]
    np.random.seed(int(g["seed"]))
    om = np.random.randn(N * N, 2, 2, N)
    box = _box(N, "f64", "numpy")
    np.random.seed(int(g["seed"]))
    out = inpaint.gaussian_cr_1d(d, w, S, np.diag(var), realisations=2, add_noise=False, verbose=False, box=box, tol=TOL)
    assert len(out) == 2
    snorm = float(np.linalg.norm(inp.sqrt_psd(S), 2))
    for i in range(2):
        a = inp.statement(d, w, S, var, om[:, i, 0], om[:, i, 1])
        b = inp.statement(d, w, S, var, om[:, i, 0], om[:, i, 1], via="eigh")
        dref = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        bnorm = np.linalg.norm(inp.rhs(d, w, S, var, om[:, i, 0], om[:, i, 1])[0], axis=1)
        _check("realisation %d against the reference" % i, np.asarray(out[i]).reshape(N * N, N), cr[i], dref, bnorm, snorm, "f64")


# ---- 5. the device generator -------------------------------------------------------------------------------------------------------
def _device_seed(box_seed, call):
    return (box_seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * call) & (2 ** 64 - 1)


@pytest.mark.parametrize("N,prec", [(16, "f64"), (24, "f32")])
def test_device_draws_match_the_host_model(N, prec):
    c = inp.build_case(N)
    d = np.where(c["w"] != 0., _stored(c["d"], prec), 0.)
    w, S, var = c["w"], c["S"], c["var"]
    box = _box(N, prec, "device", seed=77)
    out = inpaint.gaussian_cr_1d(c["d_nan"], w, S, var, realisations=2, add_noise=False, verbose=False, box=box, tol=TOL)
    seed = _device_seed(77, 1)
    snorm = float(np.linalg.norm(inp.sqrt_psd(S), 2))
    for i in range(2):
        om1, om2 = rng.gcr_normals(N, 1, seed, i), rng.gcr_normals(N, 2, seed, i)
        a = inp.statement(d, w, S, var, om1, om2)
        b = inp.statement(d, w, S, var, om1, om2, via="eigh")
        dref = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        bnorm = np.linalg.norm(inp.rhs(d, w, S, var, om1, om2)[0], axis=1)
        _check("realisation %d" % i, np.asarray(out[i]).reshape(N * N, N), a, dref, bnorm, snorm, prec)
    assert not np.array_equal(np.asarray(out[0]), np.asarray(out[1]))
    # the same seed again: bitwise the same cubes
    box2 = _box(N, prec, "device", seed=77)
    again = inpaint.gaussian_cr_1d(c["d_nan"], w, S, var, realisations=2, add_noise=False, verbose=False, box=box2, tol=TOL)
    for i in range(2):
        assert np.array_equal(np.asarray(out[i]), np.asarray(again[i])), "realisation %d is not repeatable" % i
    # add_noise: the difference is sigma omega3 of the host model, to 2 ulp of the larger term (of the stored precision)
    box3 = _box(N, prec, "device", seed=77)
    noisy = inpaint.gaussian_cr_1d(c["d_nan"], w, S, var, realisations=2, add_noise=True, verbose=False, box=box3, tol=TOL)
    ulp = 2. ** -23 if prec == "f32" else 2. ** -52
    for i in range(2):
        s, sn = np.asarray(out[i]).reshape(N * N, N), np.asarray(noisy[i]).reshape(N * N, N)
        want = np.sqrt(var) * rng.gcr_normals(N, 3, seed, i)
        err = np.abs((sn - s) - want)
        bound = 2. * ulp * np.maximum(np.abs(s), np.abs(want))
        assert np.all(err <= bound), "realisation %d: sigma omega3 off by %.3e, largest error / bound %.3f" % (
            i, float(err.max()), float(np.max(err / bound)))


# ---- 6. in-painting ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec", [(16, "f64"), (24, "f32")])
def test_inpaint_cube_keeps_the_data_and_fills_the_holes(N, prec):
    c = inp.build_case(N)
    w = c["w"]
    box = _box(N, prec, "device", seed=5)
    d_dev = box.engine.upload(c["d_nan"].reshape(N, N, N), REAL)
    full = np.asarray(inpaint.inpaint_cube(d_dev, w, c["S"], c["var"], box=box, tol=TOL)).reshape(N * N, N)
    box2 = _box(N, prec, "device", seed=5)
    cr = np.asarray(inpaint.gaussian_cr_1d(c["d_nan"], w, c["S"], c["var"], add_noise=False, verbose=False, box=box2, tol=TOL)[0]).reshape(N * N, N)
    stored = np.asarray(d_dev).reshape(N * N, N)
    assert np.array_equal(full[w != 0.], stored[w != 0.])
    assert np.array_equal(full[w == 0.], cr[w == 0.])
    assert np.all(np.isfinite(full)) and np.isnan(stored).any()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    N = 16
    c = inp.build_case(N)
    box = _box(N, "f64")
    d, w, S, var = c["d"], c["w"], c["S"], c["var"]
    dense = np.diag(var).copy()
    dense[0, 1] = dense[1, 0] = 1e-5
    with pytest.raises(NotImplementedError):
        inpaint.wiener_filter_1d(d, w, S, dense, box=box)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d[:, :8], w, S, var, box=box)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w[:100], S, var, box=box)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, S[:8, :8], var, box=box)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, S, var[:8], box=box)
    asym = S.copy()
    asym[0, 1] += 1e-3
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, asym, var, box=box)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, S, var, box=box, tol=0.)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, S, var, box=box, tol=-1e-3)
    with pytest.raises(ValueError):
        inpaint.wiener_filter_1d(d, w, S, var, box=box, cg_maxiter=0)
    with pytest.raises(TypeError):
        inpaint.wiener_filter_1d(d, w, S, var)
    # a flag per channel is accepted and equals the same flags as a cube
    wc = np.ones(N)
    wc[[2, 9]] = 0.
    a = np.asarray(inpaint.wiener_filter_1d(d, wc, S, var, box=box))
    b = np.asarray(inpaint.wiener_filter_1d(d, np.broadcast_to(wc, (N * N, N)), S, np.diag(var), box=box))
    assert np.array_equal(a, b)


# ---- 8. replace_nan_with_channel_mean ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec", list(itertools.product((16, 18, 64), ("f32", "f64"))))
def test_replace_nan_with_channel_mean(N, prec):
    rs = np.random.RandomState(40 + N)
    cube = _stored(5. + rs.standard_normal((N * N, N)), prec)
    cube[rs.uniform(size=cube.shape) < 0.1] = np.nan
    cube[:, 3] = np.nan                                              # a channel without a value stays NaN
    cube[:, 5] = _stored(rs.standard_normal(N * N), prec)            # a channel without a NaN is untouched
    want, means = inp.nan_channel_mean(cube)
    pm = np.random.RandomState(99).permutation(N * N)
    means_alt = inp.nan_channel_mean(cube[pm])[1]
    box = _box(N, prec)
    got = np.asarray(analysis.replace_nan_with_channel_mean(cube.reshape(N, N, N), box=box)).reshape(N * N, N)
    keep = ~np.isnan(cube)
    assert np.array_equal(got[keep], cube[keep])
    assert np.all(np.isnan(got[:, 3])) and not np.isnan(np.delete(got, 3, axis=1)).any()
    ok = ~np.isnan(means)
    big = np.max(np.abs(means[ok]))
    dref = float(np.max(np.abs(means_alt[ok] - means[ok])) / big)
    for j in np.nonzero(ok)[0]:
        filled = got[np.isnan(cube[:, j]), j]
        if filled.size:
            assert np.all(filled == filled[0])
            dev = abs(filled[0] - means[j]) / big
            bound = max(10. * dref, FLOOR) + (2. ** -24 if prec == "f32" else 0.)
            assert dev <= bound, "channel %d: mean off by %.3e (relative), delta_ref %.3e" % (j, dev, dref)
