"""
Foreground fits along the line of sight, on the device: a low-order polynomial per line of sight (polynomial_filter), the
power-law least-squares fit of the reference's LSQfitting (fastbox/filters.py:598-664, made runnable) and Gaussian-process
regression (gpr_filter, filters.py:494-593, without GPy).  The names are exported from fastbox_amd.filters, where the reference
keeps them.  Definitions, the bytes every kernel moves and the differences from the reference: DESIGN.md section 4.

The two fits run one wave per line of sight in libfastbox_hip (fb_losfit.hip) and honour per-voxel flags: w = 0 takes a voxel
out of the fit, whatever it holds.  The Gaussian-process likelihood needs only the N x N Gram matrix G = x^T x of the
mean-subtracted cube (fb_channel_covariance), so its optimiser runs on the host at O(N^3) per step whatever the number of
pixels; the projection x - K_fg K^-1 x is one product on the matrix cores (fb_los_matmul) and one elementwise pass.
"""
import ctypes

import numpy as np

from . import _lib
from .device import REAL, DeviceArray
from .filters import _as_cube, _channel_means, _few_blas_threads

NMAX = 1024
_PER_CHANNEL, _PER_VOXEL = 0, 1                     # FB_GCR_PER_CHANNEL, FB_GCR_PER_VOXEL
_X_PLAN = 0                                         # FB_LOS_X_PLAN
# FB_LOSFIT_*: the status of a line of sight
OK, TOO_FEW, NONFINITE, NONPOSITIVE, SINGULAR, MAXITER = range(6)
_SPACES = ("loglog", "semilog", "linear")


def _frequencies(freqs, box, N):
    if freqs is None:
        freqs = box.freq_array() if box is not None else np.linspace(1., 10., N)
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    if freqs.shape != (N,):
        raise ValueError("freqs: expected %d values, got shape %s" % (N, freqs.shape))
    step = np.diff(freqs)
    if not np.all(np.isfinite(freqs)) or not np.all(freqs > 0.) or not (np.all(step > 0.) or np.all(step < 0.)):
        raise ValueError("freqs must be positive and strictly monotonic")
    return freqs


def _aux_kind(eng, a, what):
    """None, (N,) host values, or a cube -> the kind, without touching the device"""
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        if a.kind != REAL or a.engine is not eng:
            raise TypeError("%s: expected a real-space cube of the same box" % what)
        return _PER_VOXEL
    return _PER_CHANNEL if np.shape(a) == (eng.N,) else _PER_VOXEL


def _aux(eng, a, what, positive):
    """weights or sigma -> (device object or None, kind, host (N,) copy or None)"""
    kind = _aux_kind(eng, a, what)
    if kind is None:
        return None, _PER_CHANNEL, None
    if isinstance(a, DeviceArray):
        return a, _PER_VOXEL, None
    h = np.asarray(a, dtype=np.float64)
    good = np.all(h > 0.) if positive else np.all(h >= 0.)
    if not good:
        raise ValueError("%s must be %s" % (what, "positive" if positive else "non-negative"))
    N = eng.N
    if kind == _PER_CHANNEL:
        h = np.ascontiguousarray(h)
        return eng.upload_raw(h), _PER_CHANNEL, h
    if h.shape == (N * N, N):
        h = h.reshape(N, N, N)
    if h.shape != (N, N, N):
        raise ValueError("%s: expected shape %s, %s or %s, got %s" % (what, (N,), (N, N, N), (N * N, N), h.shape))
    return eng.upload(h, REAL), _PER_VOXEL, None


def _ptr(buf):
    return buf.ptr if buf is not None else None


def _cube_bytes(eng):
    return eng.N ** 3 * np.dtype(eng.rdtype).itemsize


# ---- 1. polynomial fit -----------------------------------------------------------------------------------------------------------
def legendre_basis(u, order):
    """P_k(t), k = 0 .. order, at t = 2 (u - u_min) / (u_max - u_min) - 1: (order + 1, N)"""
    u = np.asarray(u, dtype=np.float64)
    t = 2. * (u - u.min()) / (u.max() - u.min()) - 1.
    return np.ascontiguousarray(np.polynomial.legendre.legvander(t, int(order)).T)


class LOSFit(object):
    """What polynomial_filter fitted: coeffs ((order + 1) x Npix fp64 on the device, the layout of pca_filter's amplitudes, in
    the Legendre basis of the normalised abscissa; `coeffs_host()` downloads them), model (a device cube defined at every
    channel, flagged ones included), status (int32 per line of sight on the device; `status_host()`), chi2 (fp64 per line of
    sight on the device: sum_c w^2 (y - fit)^2; `chi2_host()`), n_failed, and order, space, freqs, basis."""

    def __init__(self, engine, coeffs, model, status, chi2, n_failed, order, space, freqs, basis):
        self.engine, self.coeffs, self.model, self.status, self.chi2, self.n_failed = engine, coeffs, model, status, chi2, n_failed
        self.order, self.space, self.freqs, self.basis = order, space, freqs, basis

    def coeffs_host(self):
        return self.engine.download_raw(self.coeffs, (self.order + 1, self.engine.N ** 2))

    def chi2_host(self):
        return self.engine.download_raw(self.chi2, (self.engine.N ** 2,))

    def status_host(self):
        return self.engine.download_raw(self.status, self.engine.N ** 2, np.int32)


def polynomial_filter(field, order=3, space="loglog", freqs=None, weights=None, return_filter=False, box=None):
    """Subtract a polynomial of the given order (0 .. 7) fitted to every line of sight: y = ln T against u = ln nu ('loglog'),
    T against ln nu ('semilog') or T against nu ('linear'), minimising sum_c w^2 (y - sum_k a_k P_k(t))^2 with the Legendre
    polynomials of t = 2 (u - u_min) / (u_max - u_min) - 1.

    freqs: (N,) positive and strictly monotonic; default box.freq_array() with box=, else np.linspace(1, 10, N).  weights: None,
    (N,) host values or a cube (device or host), non-negative; w = 0 flags a voxel, which may then hold anything.  Per-voxel
    weights give every line of sight its own normal matrix, accumulated and solved by Cholesky in the kernel; None and
    per-channel weights share one pseudo-inverse (numpy.linalg.pinv of the weighted design, on the host).

    Returns the cube T - model where w != 0 (model = exp(fit) for 'loglog') and exactly 0 where w = 0, in the plan's precision.
    A line of sight that cannot be fitted is NaN at every channel and has a status other than 0: 1 fewer unflagged channels
    than coefficients, 2 a non-finite unflagged datum, 3 a non-positive one in 'loglog', 4 a non-positive pivot.  With
    return_filter a LOSFit follows.  Work memory: the result, and with return_filter one more cube and (order + 2) Npix
    doubles; MemoryError before any kernel runs if that does not fit."""
    order = int(order)
    if not 0 <= order <= 7:
        raise ValueError("order must lie in 0 .. 7")
    if space not in _SPACES:
        raise ValueError("space: 'loglog', 'semilog' or 'linear'")
    cube = _as_cube(field, box)
    eng = cube.engine
    N = eng.N
    if N > NMAX:
        raise ValueError("polynomial_filter holds a line of sight in one wave's registers: N <= %d" % NMAX)
    npix = N * N
    freqs = _frequencies(freqs, box, N)
    kind = _aux_kind(eng, weights, "weights")
    need = _cube_bytes(eng) * (2 if return_filter else 1) + npix * 4 + (npix * 8 * (order + 2) if return_filter else 0)
    if kind == _PER_VOXEL and not isinstance(weights, DeviceArray):
        need += _cube_bytes(eng)
    eng.need_memory(need, "polynomial_filter:")
    w_dev, w_kind, w_host = _aux(eng, weights, "weights", positive=False)
    basis = legendre_basis(freqs if space == "linear" else np.log(freqs), order)
    pinv_dev = None
    if w_dev is None or w_kind == _PER_CHANNEL:
        wh = np.ones(N) if w_host is None else w_host
        with _few_blas_threads():
            pinv = np.linalg.pinv(wh[:, None] * basis.T)                # (order + 1, N): a = pinv (w y)
        pinv_dev = eng.upload_raw(np.ascontiguousarray(pinv * wh[None, :]))
    basis_dev = eng.upload_raw(basis)
    out = eng.empty(REAL)
    model = eng.empty(REAL) if return_filter else None
    coeffs = eng._alloc_bytes((order + 1) * npix * 8) if return_filter else None
    chi2 = eng._alloc_bytes(npix * 8) if return_filter else None
    status = eng._alloc_bytes(npix * 4)
    n_failed = ctypes.c_int32(0)
    _lib.call("fb_los_polyfit", eng._plan, cube.ptr, _ptr(w_dev), w_kind, basis_dev.ptr, _ptr(pinv_dev), order,
              1 if space == "loglog" else 0, out.ptr, _ptr(model), _ptr(coeffs), _ptr(chi2), status.ptr, ctypes.byref(n_failed),
              eng.stream)
    if not return_filter:
        return out
    return out, LOSFit(eng, coeffs, model, status, chi2, int(n_failed.value), order, space, freqs, basis)


# ---- 2. power-law least squares ----------------------------------------------------------------------------------------------------
class LSQResult(object):
    """What LSQfitting.run_fit found, per line of sight on the host: bsval (betaS), ampS, syamp and ffamp (the two amplitudes of
    the second stage), cost (half the weighted sum of squares of the first stage), n_iter, status (0 fitted; 1 fewer than four
    unflagged channels, 2 a non-finite unflagged datum, 3 d0 <= 0 or d3 / d0 <= 0, 4 a singular normal matrix, 5 max_iter
    reached); model (a device cube, defined at every channel) and n_failed."""

    def __init__(self, engine, rows, n_iter, status, model, n_failed):
        self.engine, self.model, self.n_failed = engine, model, n_failed
        self.bsval, self.ampS, self.syamp, self.ffamp, self.cost = rows
        self.n_iter, self.status = n_iter, status


class LSQfitting(object):
    """Least-squares fit of a synchrotron-like power law to every line of sight of a cube (filters.py:598-664)."""

    def __init__(self, box):
        self.box = box

    def run_fit(self, maps, freqs=None, sigma=None, weights=None, tpsmean=None, freeind=-2.1, beta_guess=None, max_iter=50,
                tol=1e-12, return_filter=False):
        """The reference's do_loop (filters.py:625-664) for all lines of sight at once.  With d = maps - tpsmean[c], x = nu /
        nu_0 and nu_0 = freqs[0]:

        stage 1 minimises sum_c (w_c (ampS x_c^betaS - d_c) / sigma_c)^2 over 0.5 d0 <= ampS <= 1.5 d0 and betaS between 0.9 b
        and 1.1 b, where d0 is the first unflagged datum and b = ln(d3 / d0) / ln(x3 / x0) from the first and fourth unflagged
        channels (the reference's `bput`), or beta_guess (Npix,).  Variable projection: for a given betaS the best ampS within
        its bounds is closed-form, and betaS takes clipped Gauss-Newton steps, halved while the cost rises, until a step is
        below tol max(1, |betaS|); at most max_iter steps and max_iter halvings of each.  (The reference's start ampS = 0.9 d0
        plays no part: ampS is always at its optimum for the current betaS.)
        stage 2 solves amps = (S^T S)^-1 S^T d on the unflagged channels, unweighted, with S = [x^betaS, x^freeind]; model = S
        amps; residual = d - model, exactly 0 under a flag.

        maps: a REAL DeviceArray of the box's engine or a host (N, N, N) array.  freqs: default box.freq_array().  sigma: None
        (1), (N,) or a cube of standard deviations.  weights: None, (N,) or a cube; w = 0 flags a voxel, which may hold
        anything.  tpsmean: (N,) or None.  Returns (residual, bsval): a device cube and a host (Npix,) array; with
        return_filter an LSQResult follows.  A line of sight that cannot be fitted is NaN with a status (LSQResult).  Work
        memory: the residual, with return_filter the model cube, and 7 Npix doubles; MemoryError before any kernel runs if
        that does not fit."""
        cube = _as_cube(maps, self.box)
        eng = cube.engine
        N = eng.N
        if N > NMAX:
            raise ValueError("run_fit holds a line of sight in one wave's registers: N <= %d" % NMAX)
        npix = N * N
        max_iter, tol, freeind = int(max_iter), float(tol), float(freeind)
        if max_iter < 1 or not tol > 0.:
            raise ValueError("max_iter must be at least 1 and tol positive")
        freqs = _frequencies(freqs, self.box, N)
        kinds = [_aux_kind(eng, a, what) for a, what in ((sigma, "sigma"), (weights, "weights"))]
        need = _cube_bytes(eng) * (2 if return_filter else 1) + npix * (5 * 8 + 2 * 4 + (8 if beta_guess is not None else 0))
        need += sum(_cube_bytes(eng) for a, k in zip((sigma, weights), kinds) if k == _PER_VOXEL and not isinstance(a, DeviceArray))
        eng.need_memory(need, "run_fit:")
        s_dev, s_kind, _ = _aux(eng, sigma, "sigma", positive=True)
        w_dev, w_kind, _ = _aux(eng, weights, "weights", positive=False)
        tps_dev = None
        if tpsmean is not None:
            tps = np.ascontiguousarray(tpsmean, dtype=np.float64).reshape(-1)
            if tps.shape != (N,):
                raise ValueError("tpsmean: expected %d values" % N)
            tps_dev = eng.upload_raw(tps)
        guess_dev = None
        if beta_guess is not None:
            g = np.ascontiguousarray(beta_guess, dtype=np.float64).reshape(-1)
            if g.shape != (npix,):
                raise ValueError("beta_guess: expected %d values" % npix)
            guess_dev = eng.upload_raw(g)
        lnx_dev = eng.upload_raw(np.ascontiguousarray(np.log(freqs / freqs[0])))
        resid = eng.empty(REAL)
        model = eng.empty(REAL) if return_filter else None
        rows_dev = eng._alloc_bytes(5 * npix * 8)
        n_iter_dev, status_dev = eng._alloc_bytes(npix * 4), eng._alloc_bytes(npix * 4)
        n_failed = ctypes.c_int32(0)
        _lib.call("fb_los_powerlaw", eng._plan, cube.ptr, _ptr(tps_dev), _ptr(s_dev), s_kind, _ptr(w_dev), w_kind, lnx_dev.ptr, freeind,
                  _ptr(guess_dev), max_iter, tol, resid.ptr, _ptr(model), rows_dev.ptr, n_iter_dev.ptr, status_dev.ptr,
                  ctypes.byref(n_failed), eng.stream)
        rows = eng.download_raw(rows_dev, (5, npix))
        if not return_filter:
            return resid, rows[0]
        return resid, rows[0], LSQResult(eng, rows, eng.download_raw(n_iter_dev, npix, np.int32),
                                         eng.download_raw(status_dev, npix, np.int32), model, int(n_failed.value))


# ---- 3. Gaussian-process regression --------------------------------------------------------------------------------------------------
_KINDS = ("rbf", "exponential", "matern32", "matern52")


class GPRKernel(object):
    """A stationary covariance function of nu in [0, 1]: variance * c(|nu - nu'| / lengthscale), c = exp(-r^2 / 2) ('rbf'),
    exp(-r) ('exponential'), (1 + sqrt(3) r) exp(-sqrt(3) r) ('matern32') or (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)
    ('matern52'), as GPy's and scikit-learn's kernels of those names.  variance_bounds, lengthscale_bounds: (low, high) for the
    optimiser, or None (1e-10 .. 1e10 times the start)."""

    def __init__(self, kind, variance=1., lengthscale=0.1, variance_bounds=None, lengthscale_bounds=None):
        if kind not in _KINDS:
            raise ValueError("kind: one of %s" % (_KINDS,))
        self.kind, self.variance, self.lengthscale = kind, float(variance), float(lengthscale)
        if not (self.variance > 0. and self.lengthscale > 0.):
            raise ValueError("variance and lengthscale must be positive")
        self.variance_bounds = self._bounds(variance_bounds, self.variance)
        self.lengthscale_bounds = self._bounds(lengthscale_bounds, self.lengthscale)

    @staticmethod
    def _bounds(b, start):
        if b is None:
            return (1e-10 * start, 1e10 * start)
        lo, hi = float(b[0]), float(b[1])
        if not 0. < lo < hi:
            raise ValueError("bounds: 0 < low < high")
        return (lo, hi)

    def copy(self, variance=None, lengthscale=None):
        return GPRKernel(self.kind, self.variance if variance is None else variance,
                         self.lengthscale if lengthscale is None else lengthscale, self.variance_bounds, self.lengthscale_bounds)

    def matrix(self, r, variance=None, lengthscale=None, gradient=False):
        """K at the separations r; with gradient also dK / d ln(lengthscale)  (dK / d ln(variance) is K itself)."""
        v = self.variance if variance is None else variance
        ell = self.lengthscale if lengthscale is None else lengthscale
        s = r / ell
        if self.kind == "rbf":
            K = v * np.exp(-0.5 * s * s)
            dK = K * s * s
        elif self.kind == "exponential":
            K = v * np.exp(-s)
            dK = K * s
        elif self.kind == "matern32":
            a = np.sqrt(3.) * s
            e = v * np.exp(-a)
            K, dK = (1. + a) * e, a * a * e
        else:
            a = np.sqrt(5.) * s
            e = v * np.exp(-a)
            K, dK = (1. + a + a * a / 3.) * e, (a * a / 3.) * (1. + a) * e
        return (K, dK) if gradient else K

    def __repr__(self):
        return "GPRKernel(%r, variance=%.6g, lengthscale=%.6g)" % (self.kind, self.variance, self.lengthscale)


def default_gpr_kernels(var):
    """The reference's model (filters.py:559-567): a smooth foreground (RBF) that holds most of the variance and a signal with
    a small variance and a short correlation length (exponential)."""
    return [GPRKernel("rbf", 1., 0.1, (1e-4 * var, 1e2 * var), (1e-3, 1e2)),
            GPRKernel("exponential", 1., 1., (1e-14 * var, 1e-4 * var), (1e-6, 1e-3))]


def _separations(N):
    nu = np.linspace(0., 1., N)
    return np.abs(nu[:, None] - nu[None, :])


def gpr_covariances(kernels, noise_variance, N, theta=None):
    """(K_fg, K) at the kernels' own hyperparameters or at theta = ln [v_1, l_1, v_2, l_2, ..., noise]: the first kernel alone
    and the sum of all plus noise_variance on the diagonal."""
    r = _separations(N)
    par = np.exp(theta) if theta is not None else None
    K = np.zeros((N, N))
    K_fg = None
    for i, k in enumerate(kernels):
        Ki = k.matrix(r) if par is None else k.matrix(r, par[2 * i], par[2 * i + 1])
        if i == 0:
            K_fg = Ki
        K = K + Ki
    nv = noise_variance if par is None else par[-1]
    return K_fg, K + nv * np.eye(N)


def gpr_log_likelihood(theta, gram, npix, kernels, eval_gradient=False):
    """ln L of the N x npix multi-target data with Gram matrix `gram` = x^T x under shared hyperparameters theta = ln [v_1,
    l_1, ..., noise]:  -1/2 [tr(K^-1 G) + npix ln det K + npix N ln 2 pi], and its gradient in theta, 1/2 tr[(K^-1 G K^-1 - npix
    K^-1) dK/dtheta].  A failed Cholesky counts as -inf (gradient 0)."""
    from scipy.linalg import cho_factor, cho_solve, LinAlgError
    theta = np.asarray(theta, dtype=np.float64)
    N = gram.shape[0]
    r = _separations(N)
    par = np.exp(theta)
    K = par[-1] * np.eye(N)
    parts = []
    for i, k in enumerate(kernels):
        Ki, dKi = k.matrix(r, par[2 * i], par[2 * i + 1], gradient=True)
        parts.append((Ki, dKi))
        K = K + Ki
    try:
        if not np.all(np.isfinite(K)):
            raise LinAlgError("K is not finite")
        cf = cho_factor(K, lower=True)
    except (LinAlgError, ValueError):
        return (-np.inf, np.zeros_like(theta)) if eval_gradient else -np.inf
    logdet = 2. * np.sum(np.log(np.diag(cf[0])))
    KiG = cho_solve(cf, gram)
    lnL = -0.5 * (np.trace(KiG) + npix * logdet + npix * N * np.log(2. * np.pi))
    if not eval_gradient:
        return lnL
    Kinv = cho_solve(cf, np.eye(N))
    A = cho_solve(cf, KiG.T).T - npix * Kinv                      # K^-1 G K^-1 - npix K^-1 (symmetric)
    grad = np.empty_like(theta)
    for i, (Ki, dKi) in enumerate(parts):
        grad[2 * i] = 0.5 * np.sum(A * Ki)
        grad[2 * i + 1] = 0.5 * np.sum(A * dKi)
    grad[-1] = 0.5 * par[-1] * np.trace(A)
    return lnL, grad


def gpr_optimize(gram, npix, kernels, noise_variance, noise_bounds, num_restarts=10, random_state=0, messages=False):
    """Maximise gpr_log_likelihood over the kernels' bounds with scipy's L-BFGS-B and the analytic gradient, in log-parameters:
    from the given start (a start outside its bounds moves to the bounds' geometric mean) and from num_restarts log-uniform
    draws of RandomState(random_state).  Pure host code on the N x N Gram matrix.  Returns (theta, ln L, n_starts, the list of
    one message per start)."""
    from scipy.optimize import minimize
    lo, hi, start = [], [], []
    for k in kernels:
        for value, b in ((k.variance, k.variance_bounds), (k.lengthscale, k.lengthscale_bounds)):
            lo.append(b[0]); hi.append(b[1]); start.append(value)
    lo.append(noise_bounds[0]); hi.append(noise_bounds[1]); start.append(noise_variance)
    lo, hi, start = np.log(lo), np.log(hi), np.log(start)
    outside = (start < lo) | (start > hi)
    start[outside] = 0.5 * (lo + hi)[outside]
    rs = np.random.RandomState(random_state)
    starts = [start] + [rs.uniform(lo, hi) for _ in range(int(num_restarts))]
    scale = float(npix) * gram.shape[0]

    def fun(theta):
        lnL, grad = gpr_log_likelihood(theta, gram, npix, kernels, eval_gradient=True)
        if not np.isfinite(lnL):
            return 1e300, np.zeros_like(theta)
        return -lnL / scale, -grad / scale

    best, log = None, []
    with _few_blas_threads():
        for i, t0 in enumerate(starts):
            res = minimize(fun, t0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                           options=dict(ftol=1e-13, gtol=1e-9, maxiter=500, maxcor=20))
            lnL = gpr_log_likelihood(res.x, gram, npix, kernels)
            msg = res.message.decode() if isinstance(res.message, bytes) else str(res.message)
            log.append("start %d: ln L = %.10e after %d iterations (%s)" % (i, lnL, res.nit, msg))
            if messages:
                print("    gpr_filter " + log[-1])
            if np.isfinite(lnL) and (best is None or lnL > best[1]):
                best = (res.x, float(lnL))
    if best is None:
        raise RuntimeError("gpr_filter: the covariance is not positive definite at any start")
    return best[0], best[1], len(starts), log


def gpr_projection(kernels, noise_variance, N):
    """(M, cov_fg, K): M = K_fg K^-1 by a solve, cov_fg = K_fg - M K_fg (the posterior covariance of the foreground part)."""
    from scipy.linalg import cho_factor, cho_solve
    K_fg, K = gpr_covariances(kernels, noise_variance, N)
    with _few_blas_threads():
        M = cho_solve(cho_factor(K, lower=True), K_fg).T             # K symmetric: K_fg K^-1 = (K^-1 K_fg)^T
        cov_fg = K_fg - M @ K_fg
    return np.ascontiguousarray(M), cov_fg, K


class GPRResult(object):
    """What gpr_filter found: kernels (GPRKernel with the optimised hyperparameters, foreground first), noise_variance,
    log_marginal_likelihood, fg_matrix (M = K_fg K^-1, host (N, N)), cov_fg (K_fg - M K_fg), n_starts, messages (one line per
    start of the optimiser), and timings (seconds: 'gram', 'optimise', 'project', each ended by a synchronisation)."""

    def __init__(self, kernels, noise_variance, lnL, M, cov_fg, n_starts, messages, timings):
        self.kernels, self.noise_variance, self.log_marginal_likelihood = kernels, noise_variance, lnL
        self.fg_matrix, self.cov_fg, self.n_starts, self.messages, self.timings = M, cov_fg, n_starts, messages, timings


def gpr_filter(field, kernels=None, return_filter=False, opt_messages=True, opt_num_restarts=10, box=None, optimize=True,
               noise_variance=None, random_state=0):
    """Gaussian-process regression along frequency (filters.py:494-593): the mean-subtracted cube x is modelled per line of
    sight as a draw from K = sum of the kernels + noise_variance I on nu = linspace(0, 1, N), with hyperparameters shared by
    all lines of sight; the cleaned cube is x - K_fg K^-1 x, K_fg the first kernel.

    kernels: a list of GPRKernel, the foreground first; default the reference's RBF + exponential with its bounds, var =
    np.var(x) taken from the trace of the channel covariance.  noise_variance: the start (or, with optimize=False, the value)
    of the Gaussian noise variance GPy's GPRegression adds; default 1.0 as GPy's, moved like every start to the geometric mean
    of its bounds (1e-12 var, var) when it lies outside.  optimize: maximise the marginal likelihood (gpr_optimize: from the
    start and opt_num_restarts log-uniform draws of RandomState(random_state); opt_messages prints a line per start);
    optimize=False applies the hyperparameters as given.

    The likelihood needs only the N x N matrix x^T x (fb_channel_means, fb_channel_covariance), so the optimiser never touches
    the cube.  Returns the cleaned cube (DeviceArray) and, with return_filter, a GPRResult.  Work memory: one fp64 cube, the
    result and N^2 + 2 N doubles; MemoryError before any kernel runs if that does not fit."""
    import time
    cube = _as_cube(field, box)
    eng = cube.engine
    N = eng.N
    if N > NMAX:
        raise ValueError("gpr_filter: N <= %d" % NMAX)
    npix = N * N
    if kernels is not None:
        kernels = list(kernels)
        if not kernels or not all(isinstance(k, GPRKernel) for k in kernels):
            raise TypeError("kernels: a list of GPRKernel")
    eng.need_memory(N ** 3 * 8 + _cube_bytes(eng) + (N * N + 2 * N) * 8, "gpr_filter:")
    t0 = time.perf_counter()
    mean_dev = _channel_means(eng, cube)
    cov_dev = eng._alloc_bytes(N * N * 8)
    _lib.call("fb_channel_covariance", eng._plan, cube.ptr, mean_dev.ptr, cov_dev.ptr, eng.stream)
    mean = eng.download_raw(mean_dev, (N,))
    gram = eng.download_raw(cov_dev, (N, N)) * (npix - 1.)           # x^T x
    gram = 0.5 * (gram + gram.T)
    t1 = time.perf_counter()
    var = float(np.trace(gram)) / (float(npix) * N)                # np.var(x): every channel of x has zero mean
    if kernels is None:
        kernels = default_gpr_kernels(var)
    noise_bounds = (1e-12 * var, var) if var > 0. else (1e-300, 1.)
    nv = 1.0 if noise_variance is None else float(noise_variance)
    if not nv > 0.:
        raise ValueError("noise_variance must be positive")
    lnL, n_starts, log = None, 0, []
    if optimize:
        theta, lnL, n_starts, log = gpr_optimize(gram, npix, kernels, nv, noise_bounds, opt_num_restarts, random_state,
                                                 messages=opt_messages)
        par = np.exp(theta)
        kernels = [k.copy(par[2 * i], par[2 * i + 1]) for i, k in enumerate(kernels)]
        nv = float(par[-1])
    M, cov_fg, _ = gpr_projection(kernels, nv, N)
    if lnL is None and return_filter:
        theta = np.log([p for k in kernels for p in (k.variance, k.lengthscale)] + [nv])
        with _few_blas_threads():
            lnL = float(gpr_log_likelihood(theta, gram, npix, kernels))
    t2 = time.perf_counter()
    Y = eng._alloc_bytes(N ** 3 * 8)
    _lib.call("fb_los_matmul", eng._plan, eng.upload_raw(M).ptr, cube.ptr, _X_PLAN, None, None, None, Y.ptr, eng.stream)
    out = eng.empty(REAL)
    shift = eng.upload_raw(np.ascontiguousarray(mean - M @ mean))
    _lib.call("fb_los_subtract", eng._plan, cube.ptr, Y.ptr, shift.ptr, out.ptr, eng.stream)
    eng.sync()
    t3 = time.perf_counter()
    if not return_filter:
        return out
    return out, GPRResult(kernels, nv, lnL, M, cov_fg, n_starts, log, dict(gram=t1 - t0, optimise=t2 - t1, project=t3 - t2))
