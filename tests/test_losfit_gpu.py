"""GPU: filters.polynomial_filter, LSQfitting.run_fit and gpr_filter against their statements (tests/losfit_numpy.py).

Tolerances are not fixed in advance.  Every statement is evaluated twice (lstsq and QR; trf and dogbox; Cholesky and eigh); the
deviation of the two, relative to the largest magnitude of the quantity, is delta_ref, and the device must lie within 10
delta_ref (floor 1e-12) of the first.  A cube stored in fp32 gets 4 2^-24 |value| per element besides.  The statements are fed
the data as the device stores them.  Every assertion message carries the measured deviation and delta_ref.

Sizes: 16; 18 (N % 4 = 2, not a power of two); 24; 64 (the largest with one channel per lane); 72 (the smallest grid the plans
accept above 64: four channels per lane, the last of them partly past the end); 270 (the smallest above 256: sixteen channels per
lane).  A plan's N is even, so N^2 is always a multiple of the four rows of a workgroup and no size leaves a workgroup partly
filled.  From N = 64 up the
statements run on the four constructed lines of sight and a fixed stride of the others (_rows); statuses, NaN rows and the zeros
under flags are checked on the whole cube."""
import functools
import itertools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, filters, losfit
from fastbox_amd.device import REAL
from tests import losfit_numpy as ln

pytestmark = pytest.mark.gpu
FLOOR = 1e-12
EPS = 2. ** -52
SPACES = ("loglog", "semilog", "linear")
MODES = ("none", "chan", "voxel")


def _box(N, prec):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec)


def _stored(a, prec):
    """what the device holds of a host array"""
    return a.astype(np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _rows(N):
    npix = N * N
    if N <= 24:
        return np.arange(npix)
    return np.unique(np.concatenate([np.arange(8), np.arange(8, npix, npix // 88)]))


def _aux(c, name, mode, prec):
    """weights or sigma of a case -> (the argument of the call, the (N^2, N) array of the statement)"""
    N = c["N"]
    if mode == "none":
        return None, np.ones((N * N, N))
    if mode == "chan":
        v = c[name + "_chan"]
        return v, np.broadcast_to(v, (N * N, N))
    return c[name].reshape(N, N, N), _stored(c[name], prec)


def _within(what, got, want, alt):
    big = float(np.max(np.abs(want)))
    dref, dev = float(np.max(np.abs(alt - want))) / big, float(np.max(np.abs(got - want))) / big
    assert dev <= max(10. * dref, FLOOR), "%s: device deviation %.3e, delta_ref %.3e" % (what, dev, dref)


def _cube_within(what, got, want, alt, prec):
    big = float(np.max(np.abs(want)))
    dref = float(np.max(np.abs(alt - want))) / big
    bound = 10. * max(dref, FLOOR / 10.) * big + (4. * 2. ** -24 * np.abs(want) if prec == "f32" else 0.)
    err = np.abs(got - want)
    assert np.all(err <= bound), "%s: device deviation %.3e (relative to the largest value), delta_ref %.3e, largest excess %.3e" % (
        what, float(err.max()) / big, dref, float((err - bound).max()))


def _host(dev_cube, N):
    return np.asarray(dev_cube).reshape(N * N, N).astype(np.float64)


# ---- 1. the polynomial fit ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poly_ref(N, prec, order, space, mode):
    c = ln.build_case(N)
    rows = _rows(N)
    T = _stored(c["d_nan"], prec)
    w = _aux(c, "w", mode, prec)[1]
    a = ln.poly_statement(T[rows], w[rows], c["freqs"], order, space, via="lstsq")
    b = ln.poly_statement(T[rows], w[rows], c["freqs"], order, space, via="qr")
    return rows, a, b, ln.poly_status_rows(T, w, order, space)


POLY = [(16, "f64", o, s, m) for o, s, m in itertools.product((0, 1, 3, 7), SPACES, MODES)]
POLY += [(16, "f32", 3, "loglog", "voxel"), (16, "f32", 7, "semilog", "chan"), (16, "f32", 1, "linear", "none")]
for _N in (18, 24, 64, 72):
    POLY += [(_N, "f64", 3, "loglog", "voxel"), (_N, "f32", 7, "semilog", "voxel"), (_N, "f64", 7, "linear", "chan"),
             (_N, "f32", 1, "loglog", "none")]
POLY += [(270, "f32", 3, "loglog", "voxel"), (270, "f64", 7, "semilog", "chan")]


@pytest.mark.parametrize("N,prec,order,space,mode", POLY)
def test_polynomial_filter_matches_the_statement(N, prec, order, space, mode):
    c = ln.build_case(N)
    rows, a, b, want_status = _poly_ref(N, prec, order, space, mode)
    warg, w = _aux(c, "w", mode, prec)
    box = _box(N, prec)
    cube = box.engine.upload(c["d_nan"].reshape(N, N, N), REAL)
    out, fit = filters.polynomial_filter(cube, order=order, space=space, freqs=c["freqs"], weights=warg, return_filter=True, box=box)
    got, model, status, coeffs = _host(out, N), _host(fit.model, N), fit.status_host(), fit.coeffs_host()
    assert np.array_equal(status, want_status), "rows with another status: %s" % np.flatnonzero(status != want_status)[:10]
    assert np.array_equal(a["status"], want_status[rows]) and np.array_equal(b["status"], want_status[rows])
    bad = want_status != 0
    assert fit.n_failed == int(bad.sum())
    expected = {ln.ROW_EMPTY: ln.TOO_FEW} if mode == "voxel" else ({ln.ROW_NAN: ln.NONFINITE} if mode == "none" else {})
    if space == "loglog":
        expected[ln.ROW_NEGATIVE] = ln.NONPOSITIVE
    for r, s in expected.items():
        assert status[r] == s, "constructed row %d: status %d, expected %d" % (r, status[r], s)
    assert set(np.flatnonzero(status != 0)) - set(expected) <= set(np.flatnonzero(want_status == ln.TOO_FEW))
    assert np.isnan(got[bad]).all() and np.isnan(model[bad]).all() and np.isnan(coeffs[:, bad]).all()
    assert np.isfinite(got[~bad]).all() and np.isfinite(model[~bad]).all()
    assert np.all(got[~bad][w[~bad] == 0.] == 0.), "a flagged voxel is not exactly 0"
    ok = a["status"] == 0
    sub = rows[ok]
    _within("coeffs", coeffs[:, sub], a["coeffs"][:, ok], b["coeffs"][:, ok])
    _cube_within("cleaned", got[sub], a["cleaned"][ok], b["cleaned"][ok], prec)
    _cube_within("model", model[sub], a["model"][ok], b["model"][ok], prec)
    flagged = w[sub] == 0.
    if flagged.any():
        _cube_within("model at flagged channels", np.where(flagged, model[sub], 0.), np.where(flagged, a["model"][ok], 0.),
                     np.where(flagged, b["model"][ok], 0.), prec)
    # chi2 from the device's own coefficients: y - fit cancels |y| / |y - fit| <= 1e5 digits' worth, so 1e-9 relative
    V = ln.legendre_design(c["freqs"], order, space)
    T = _stored(c["d_nan"], prec)[sub]
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.where(w[sub] != 0., np.log(T) if space == "loglog" else T, 0.)
    chi = np.sum(np.where(w[sub] != 0., w[sub] * (y - coeffs[:, sub].T @ V.T), 0.) ** 2, axis=1)
    got_chi = fit.chi2_host()
    assert np.all(np.abs(got_chi[sub] - chi) <= 1e-9 * np.max(chi)), "chi2 off by %.3e (relative)" % (np.max(np.abs(got_chi[sub] - chi)) / np.max(chi))
    assert np.isnan(got_chi[bad]).all()
    # without return_filter, and a second call: the same bits
    again = filters.polynomial_filter(cube, order=order, space=space, freqs=c["freqs"], weights=warg, box=box)
    assert np.array_equal(np.asarray(again), np.asarray(out), equal_nan=True)


def test_per_channel_weights_take_both_paths():
    """per-channel weights through the shared pseudo-inverse, and the same weights as a cube through the per-row Cholesky"""
    N, order = 24, 7
    c = ln.build_case(N)
    box = _box(N, "f64")
    shared = _host(filters.polynomial_filter(c["d"].reshape(N, N, N), order, "semilog", c["freqs"], c["w_chan"], box=box), N)
    cube_w = np.broadcast_to(c["w_chan"], (N, N, N))
    own = _host(filters.polynomial_filter(c["d"].reshape(N, N, N), order, "semilog", c["freqs"], cube_w, box=box), N)
    ref = ln.poly_statement(c["d"], np.broadcast_to(c["w_chan"], (N * N, N)), c["freqs"], order, "semilog")
    alt = ln.poly_statement(c["d"], np.broadcast_to(c["w_chan"], (N * N, N)), c["freqs"], order, "semilog", via="qr")
    _cube_within("shared pseudo-inverse", shared, ref["cleaned"], alt["cleaned"], "f64")
    _cube_within("per-row Cholesky", own, ref["cleaned"], alt["cleaned"], "f64")


def test_polynomial_filter_arguments_and_memory_guard(monkeypatch):
    N = 16
    c = ln.build_case(N)
    box = _box(N, "f64")
    cube = box.engine.upload(c["d"].reshape(N, N, N), REAL)
    for kw in (dict(order=8), dict(order=-1), dict(space="log"), dict(freqs=c["freqs"][:8]), dict(freqs=-c["freqs"]),
               dict(weights=-np.ones(N)), dict(weights=np.ones((N, N)))):
        with pytest.raises(ValueError):
            filters.polynomial_filter(cube, box=box, **kw)
    with pytest.raises(TypeError):
        filters.polynomial_filter(c["d"].reshape(N, N, N))
    # the default frequencies follow the box (decreasing) or, without one, linspace(1, 10, N)
    a = np.asarray(filters.polynomial_filter(cube, box=box))
    b = np.asarray(filters.polynomial_filter(cube, freqs=box.freq_array()))
    assert np.array_equal(a, b, equal_nan=True) and np.isnan(a).sum() == N          # (the negative datum: one NaN row in ln T)
    calls = []
    real_call = losfit._lib.call
    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 10)
    monkeypatch.setattr(losfit._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    with pytest.raises(MemoryError, match="work memory"):
        filters.polynomial_filter(cube, box=box)
    with pytest.raises(MemoryError, match="work memory"):
        filters.LSQfitting(box).run_fit(cube, freqs=c["freqs"])
    with pytest.raises(MemoryError, match="work memory"):
        filters.gpr_filter(cube, optimize=False, noise_variance=1e-3)
    assert calls == []


# ---- 2. the power-law fit -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plaw_ref(N, prec, smode, wmode, tps):
    c = ln.build_case(N)
    rows = _rows(N)
    tpsmean = c["tpsmean"] if tps else None
    maps = _stored(c["d_nan"] + (c["tpsmean"] if tps else 0.), prec)
    sigma, w = _aux(c, "sigma", smode, prec)[1], _aux(c, "w", wmode, prec)[1]
    a = ln.plaw_statement(maps[rows], c["freqs"], sigma[rows], w[rows], tpsmean, method="trf")
    b = ln.plaw_statement(maps[rows], c["freqs"], sigma[rows], w[rows], tpsmean, method="dogbox")
    d = maps - (c["tpsmean"] if tps else 0.)
    return rows, a, b, ln.plaw_status_rows(d, w), maps


PLAW = [(16, "f64", "none", "none", False), (16, "f64", "chan", "chan", True), (16, "f64", "voxel", "voxel", False),
        (16, "f64", "voxel", "chan", True), (16, "f64", "none", "voxel", True), (16, "f32", "voxel", "voxel", True),
        (16, "f32", "chan", "none", False)]
for _N in (18, 24, 64, 72):
    PLAW += [(_N, "f64", "voxel", "voxel", True), (_N, "f32", "chan", "voxel", False)]
PLAW += [(270, "f32", "voxel", "voxel", True), (270, "f64", "chan", "chan", False)]


@pytest.mark.parametrize("N,prec,smode,wmode,tps", PLAW)
def test_run_fit_matches_the_statement(N, prec, smode, wmode, tps):
    c = ln.build_case(N)
    rows, a, b, want_status, maps = _plaw_ref(N, prec, smode, wmode, tps)
    sarg, sigma = _aux(c, "sigma", smode, prec)
    warg, w = _aux(c, "w", wmode, prec)
    box = _box(N, prec)
    cube = box.engine.upload(maps.reshape(N, N, N), REAL)
    kw = dict(freqs=c["freqs"], sigma=sarg, weights=warg, tpsmean=c["tpsmean"] if tps else None, freeind=ln.FREEIND)
    resid, bsval, res = filters.LSQfitting(box).run_fit(cube, return_filter=True, **kw)
    got = _host(resid, N)
    assert np.array_equal(res.status, want_status), "rows with another status: %s" % np.flatnonzero(res.status != want_status)[:10]
    assert np.array_equal(a["status"], want_status[rows]) and np.array_equal(b["status"], want_status[rows])
    expected = {ln.ROW_NEGATIVE: ln.NONPOSITIVE}
    if wmode == "voxel":
        expected[ln.ROW_EMPTY] = ln.TOO_FEW
    if wmode == "none":
        expected[ln.ROW_NAN] = ln.NONFINITE
    assert {int(r): int(res.status[r]) for r in np.flatnonzero(res.status)} == expected, "only the constructed failures may fail"
    bad = want_status != 0
    assert res.n_failed == int(bad.sum()) and np.isnan(got[bad]).all() and np.isnan(bsval[bad]).all() and np.isnan(_host(res.model, N)[bad]).all()
    assert np.isfinite(got[~bad]).all() and np.all(got[~bad][w[~bad] == 0.] == 0.)
    assert np.all(res.n_iter[~bad] >= 1) and np.all(res.n_iter[~bad] <= 50)
    ok = a["status"] == 0
    sub = rows[ok]
    _within("ampS", res.ampS[sub], a["ampS"][ok], b["ampS"][ok])
    _within("betaS", bsval[sub], a["bsval"][ok], b["bsval"][ok])
    assert np.array_equal(bsval, res.bsval, equal_nan=True)
    # the device's parameters through the statement's cost function
    x = c["freqs"] / c["freqs"][0]
    spread, worst = 0., 0.
    for i, p in zip(np.flatnonzero(ok), sub):
        good = w[p] != 0.
        d = np.where(good, maps[p] - (c["tpsmean"] if tps else 0.), 0.)
        q = np.where(good, w[p] / sigma[p], 0.)
        cmin = min(a["cost"][i], b["cost"][i])
        spread = max(spread, abs(a["cost"][i] - b["cost"][i]) / cmin)
        worst = max(worst, (ln.plaw_cost(res.ampS[p], bsval[p], d, x, q) - cmin) / cmin)
    assert worst <= max(10. * spread, FLOOR), "cost above the smaller scipy cost by %.3e (relative), scipy's spread %.3e" % (worst, spread)
    # the constructed row ends on its bound 1.1 b
    i = int(np.flatnonzero(rows == ln.ROW_BOUND)[0])
    dref = max(abs(a["bsval"][i] - b["bsval"][i]) / abs(a["bsval"][i]), FLOOR / 10.)
    off = abs(bsval[ln.ROW_BOUND] - a["bounds"][i, 0]) / abs(a["bounds"][i, 0])
    assert off <= 10. * dref, "the bound row is %.3e (relative) off its bound, delta_ref %.3e" % (off, dref)
    _within("syamp", res.syamp[sub], a["syamp"][ok], b["syamp"][ok])
    _within("ffamp", res.ffamp[sub], a["ffamp"][ok], b["ffamp"][ok])
    _cube_within("residual", got[sub], a["residual"][ok], b["residual"][ok], prec)
    _cube_within("model", _host(res.model, N)[sub], a["model"][ok], b["model"][ok], prec)
    # without return_filter, and a second call: the same bits
    resid2, bsval2 = filters.LSQfitting(box).run_fit(cube, **kw)
    assert np.array_equal(np.asarray(resid2), np.asarray(resid), equal_nan=True) and np.array_equal(bsval2, bsval, equal_nan=True)


def test_run_fit_guess_iteration_limit_and_arguments():
    N = 16
    c = ln.build_case(N)
    rows, a, b, want_status, maps = _plaw_ref(N, "f64", "voxel", "voxel", False)
    box = _box(N, "f64")
    fitter = filters.LSQfitting(box)
    kw = dict(freqs=c["freqs"], sigma=c["sigma"].reshape(N, N, N), weights=c["w"].reshape(N, N, N))
    # the statement's guess handed in: the same fit
    guess = np.where(np.isfinite(a["guess"]), a["guess"], -2.7)
    _, bsval = fitter.run_fit(maps.reshape(N, N, N), beta_guess=guess, **kw)
    ok = a["status"] == 0
    _within("betaS from beta_guess", bsval[ok], a["bsval"][ok], b["bsval"][ok])
    assert np.isnan(bsval[ln.ROW_EMPTY]) and np.isnan(bsval[ln.ROW_NEGATIVE])
    # one step is not enough: the status says so and the row is NaN; nothing spins
    resid, bsval, res = fitter.run_fit(maps.reshape(N, N, N), max_iter=1, return_filter=True, **kw)
    assert np.all(res.status[ok] == ln.MAXITER) and np.isnan(bsval).all() and np.isnan(_host(resid, N)).all() and res.n_failed == N * N
    assert np.all(res.n_iter <= 1)
    for bad in (dict(max_iter=0), dict(tol=0.), dict(sigma=np.zeros(N)), dict(weights=-np.ones(N)), dict(tpsmean=np.ones(3)),
                dict(beta_guess=np.ones(5)), dict(freqs=c["freqs"][::2])):
        with pytest.raises(ValueError):
            fitter.run_fit(maps.reshape(N, N, N), **bad)


# ---- 3. Gaussian-process regression ---------------------------------------------------------------------------------------------------
GPR_FIXED = np.log([4.0, 0.3, 0.05, 0.02, 1e-3])


@functools.lru_cache(maxsize=None)
def _gpr_cube(N, prec, kinds=("rbf", "exponential")):
    x = _stored(ln.gpr_draw(N, kinds, GPR_FIXED, seed=N), prec)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("N,prec,kinds", [(16, "f64", ("rbf", "exponential")), (16, "f32", ("rbf", "matern32")), (18, "f64", ("matern52", "exponential")),
                                          (24, "f32", ("rbf", "exponential")), (64, "f64", ("rbf", "exponential")), (72, "f32", ("rbf", "exponential")),
                                          (72, "f64", ("rbf", "matern32"))])
def test_gpr_filter_with_given_hyperparameters(N, prec, kinds):
    X = _gpr_cube(N, prec, kinds)
    x = X - X.mean(axis=0)
    par = np.exp(GPR_FIXED)
    kernels = [filters.GPRKernel(kinds[0], par[0], par[1]), filters.GPRKernel(kinds[1], par[2], par[3])]
    Ma, ca = ln.gpr_matrices(GPR_FIXED, kinds, N)
    Mb, cb = ln.gpr_matrices(GPR_FIXED, kinds, N, via="eigh")
    box = _box(N, prec)
    out, res = filters.gpr_filter(X.reshape(N, N, N), kernels=kernels, optimize=False, noise_variance=par[4], return_filter=True, box=box)
    _cube_within("cleaned", _host(out, N), x - x @ Ma.T, x - x @ Mb.T, prec)
    _within("fg_matrix", res.fg_matrix, Ma, Mb)
    kfg = float(np.max(np.abs(ln.kernel_matrix(kinds[0], par[0], par[1], N))))
    dref = float(np.max(np.abs(ca - cb))) / kfg
    dev = float(np.max(np.abs(res.cov_fg - ca))) / kfg
    assert dev <= max(10. * dref, FLOOR), "cov_fg: deviation %.3e (relative to |K_fg|), delta_ref %.3e" % (dev, dref)
    assert res.n_starts == 0 and res.noise_variance == par[4] and [k.kind for k in res.kernels] == list(kinds)
    # ln L from the device's Gram matrix against the statement's from numpy's: 10 cond(K) 2^-52 of the summed terms
    gram = x.T @ x
    lnL = ln.gpr_lml(GPR_FIXED, gram, N * N, kinds)[0]
    K = ln.gpr_parts(GPR_FIXED, kinds, N)[0]
    scale = abs(np.sum(np.linalg.inv(K) * gram)) + N * N * abs(np.linalg.slogdet(K)[1]) + N ** 3 * np.log(2. * np.pi)
    assert abs(res.log_marginal_likelihood - lnL) <= 10. * np.linalg.cond(K) * EPS * scale, "ln L %.12e, statement %.12e" % (
        res.log_marginal_likelihood, lnL)
    again = filters.gpr_filter(X.reshape(N, N, N), kernels=kernels, optimize=False, noise_variance=par[4], box=box)
    assert np.array_equal(np.asarray(again), np.asarray(out))


def test_gpr_filter_optimised():
    """A cube drawn from known hyperparameters inside the default bounds: ln L returned >= ln L at the generating
    hyperparameters, and not below scikit-learn's optimum of the same kernel and bounds by more than the spread of
    scikit-learn's own optima over two seeds of its restarts (floor: its L-BFGS-B ftol times |ln L|)."""
    N = 16
    X = ln.gpr_draw(N, ln.GPR_KINDS, ln.GPR_TRUTH, 0)
    x = X - X.mean(axis=0)
    box = _box(N, "f64")
    out, res = filters.gpr_filter(X.reshape(N, N, N), return_filter=True, opt_messages=False, box=box)
    assert res.n_starts == 11 == len(res.messages)
    gram = x.T @ x
    truth = ln.gpr_lml(ln.GPR_TRUTH, gram, N * N, ln.GPR_KINDS)[0]
    assert res.log_marginal_likelihood >= truth, "ln L %.10e at the optimum, %.10e at the generating hyperparameters" % (
        res.log_marginal_likelihood, truth)
    sk = ln.sklearn_optima(N)
    slack = max(abs(sk[0] - sk[1]), ln.SKLEARN_FTOL * abs(max(sk)))
    assert res.log_marginal_likelihood >= max(sk) - slack, "ln L %.10e, scikit-learn's optima %.10e and %.10e (slack %.3e)" % (
        res.log_marginal_likelihood, sk[0], sk[1], slack)
    # the cleaned cube is the projection with the optimised hyperparameters
    theta = np.log([res.kernels[0].variance, res.kernels[0].lengthscale, res.kernels[1].variance, res.kernels[1].lengthscale, res.noise_variance])
    bounds = ln.default_bounds(float(np.var(x)))
    assert all(lo * (1. - 1e-12) <= p <= hi * (1. + 1e-12) for p, (lo, hi) in zip(np.exp(theta), bounds))
    Ma, Mb = ln.gpr_matrices(theta, ln.GPR_KINDS, N)[0], ln.gpr_matrices(theta, ln.GPR_KINDS, N, via="eigh")[0]
    _cube_within("cleaned", _host(out, N), x - x @ Ma.T, x - x @ Mb.T, "f64")
    out2, res2 = filters.gpr_filter(X.reshape(N, N, N), return_filter=True, opt_messages=False, box=box)
    assert np.array_equal(np.asarray(out2), np.asarray(out)) and res2.log_marginal_likelihood == res.log_marginal_likelihood
