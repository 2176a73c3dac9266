"""numpy / scipy statements of fastbox_amd.losfit: the polynomial fit, the bounded power-law fit with its two-template solve, and
the Gaussian-process likelihood and projection through the Gram matrix.  Every statement has two evaluations (lstsq and QR; trf
and dogbox; Cholesky and eigh) whose deviation from each other is the yardstick delta_ref of the tests.  Nothing here imports
the product."""
import functools

import numpy as np

OK, TOO_FEW, NONFINITE, NONPOSITIVE, SINGULAR, MAXITER = range(6)
# the constructed lines of sight of build_case
ROW_EMPTY, ROW_NEGATIVE, ROW_NAN, ROW_BOUND = 0, 1, 2, 3
FLAGGED_CHANNELS = (5, 11)              # the per-channel flags; ROW_NAN holds its NaN in the first of them
FREEIND = -2.1


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def frequencies(N):
    return np.linspace(900., 1050., N)


@functools.lru_cache(maxsize=None)
def build_case(N, seed=0):
    """A power-law cube with per-pixel amplitude and index, a free-free term and noise, as (N^2, N) rows, with weights:

    d        the data without holes (every datum positive except ROW_NEGATIVE's first)
    d_nan    d with NaN under every per-voxel flag of ROW_NAN
    w        per-voxel weights in {0} + [0.5, 1.5], about 20 % flagged; FLAGGED_CHANNELS are flagged in every row
    w_chan   per-channel weights: FLAGGED_CHANNELS flagged
    sigma, sigma_chan   standard deviations per voxel and per channel
    tpsmean  a smooth mean spectrum to be added to d by the caller

    ROW_EMPTY is fully flagged in w.  ROW_NEGATIVE has a negative first datum (unflagged).  ROW_NAN has NaN at
    FLAGGED_CHANNELS[0].  ROW_BOUND has channels 0 .. 3 unflagged and channel 3 raised so that the guess of the index moves by
    0.3: the optimum of the bounded fit then sits on the bound 1.1 b."""
    rs = np.random.RandomState(1000 * seed + N)
    npix = N * N
    nu = frequencies(N)
    x = nu / nu[0]
    lever = np.log(x[3] / x[0])
    amp = rs.uniform(5., 20., size=npix)
    beta = rs.uniform(-2.9, -2.5, size=npix)
    beta[ROW_BOUND] = -2.6
    free = rs.uniform(0.02, 0.08, size=npix) * amp
    level = 0.02 * lever / np.sqrt(2.)                                  # the guess of the index scatters by 0.02
    sigma_chan = level * 10. * x ** -2.5 * (1. + 0.2 * np.cos(np.arange(N)))
    sigma = sigma_chan[None, :] * rs.uniform(0.5, 1.5, size=(npix, N))
    d = amp[:, None] * x[None, :] ** beta[:, None] + free[:, None] * x[None, :] ** FREEIND + sigma_chan[None, :] * rs.standard_normal((npix, N))
    w = rs.uniform(0.5, 1.5, size=(npix, N))
    w[rs.uniform(size=(npix, N)) < 0.18] = 0.
    w[:, list(FLAGGED_CHANNELS)] = 0.
    w_chan = 1. + 0.3 * np.sin(np.arange(N))
    w_chan[list(FLAGGED_CHANNELS)] = 0.
    w[ROW_EMPTY] = 0.
    w[ROW_NEGATIVE, 0] = 1.
    d[ROW_NEGATIVE, 0] = -d[ROW_NEGATIVE, 0]
    w[ROW_BOUND, :4] = 1.
    d[ROW_BOUND] = amp[ROW_BOUND] * x ** beta[ROW_BOUND]
    d[ROW_BOUND, 3] *= np.exp(0.3 * lever)
    d_nan = d.copy()
    d_nan[ROW_NAN, FLAGGED_CHANNELS[0]] = np.nan
    tpsmean = 3. * x ** -0.7
    out = dict(N=N, freqs=nu, d=d, d_nan=d_nan, w=w, w_chan=w_chan, sigma=sigma, sigma_chan=sigma_chan, tpsmean=tpsmean)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the polynomial fit ----------------------------------------------------------------------------------------------------------------
def legendre_design(freqs, order, space):
    """(N, order + 1): P_k(t) at t = 2 (u - u_min) / (u_max - u_min) - 1, u = ln nu ('loglog', 'semilog') or nu ('linear')"""
    u = np.asarray(freqs, dtype=np.float64) if space == "linear" else np.log(freqs)
    t = 2. * (u - u.min()) / (u.max() - u.min()) - 1.
    cols = [np.ones_like(t), t]
    for k in range(1, int(order)):                                       # Bonnet's recursion
        cols.append(((2 * k + 1) * t * cols[k] - k * cols[k - 1]) / (k + 1))
    return np.stack(cols[:int(order) + 1], axis=1)


def poly_status(T, w, order, space):
    good = w != 0.
    if good.sum() < order + 1:
        return TOO_FEW
    if not np.all(np.isfinite(T[good])):
        return NONFINITE
    if space == "loglog" and np.any(T[good] <= 0.):
        return NONPOSITIVE
    return OK


def poly_status_rows(T, w, order, space):
    """poly_status of every row at once"""
    good = w != 0.
    few = good.sum(axis=1) < order + 1
    nonfinite = (good & ~np.isfinite(T)).any(axis=1)
    with np.errstate(invalid="ignore"):
        nonpos = (good & (T <= 0.)).any(axis=1) if space == "loglog" else np.zeros(len(T), dtype=bool)
    return np.where(few, TOO_FEW, np.where(nonfinite, NONFINITE, np.where(nonpos, NONPOSITIVE, OK))).astype(np.int32)


def plaw_status_rows(d, w):
    """the status plaw_guess gives every row (d: the data after the mean spectrum is subtracted)"""
    good = w != 0.
    rank = np.cumsum(good, axis=1)
    few = rank[:, -1] < 4
    nonfinite = (good & ~np.isfinite(d)).any(axis=1)
    first, fourth = np.argmax(good & (rank == 1), axis=1), np.argmax(good & (rank == 4), axis=1)
    r = np.arange(len(d))
    with np.errstate(invalid="ignore", divide="ignore"):
        d0, d3 = d[r, first], d[r, fourth]
        nonpos = ~(d0 > 0.) | ~(d3 / d0 > 0.)
    return np.where(few, TOO_FEW, np.where(nonfinite, NONFINITE, np.where(nonpos, NONPOSITIVE, OK))).astype(np.int32)


def poly_statement(T, w, freqs, order, space, via="lstsq"):
    """T, w: (rows, N).  -> cleaned (T - model where w != 0, 0 elsewhere; NaN rows where the fit fails), coeffs (order + 1,
    rows), model (rows, N; at every channel), status, chi2"""
    from scipy.linalg import solve_triangular
    rows, N = T.shape
    V = legendre_design(freqs, order, space)
    cleaned, model = np.full((rows, N), np.nan), np.full((rows, N), np.nan)
    coeffs, chi2 = np.full((order + 1, rows), np.nan), np.full(rows, np.nan)
    status = np.zeros(rows, dtype=np.int32)
    for p in range(rows):
        status[p] = poly_status(T[p], w[p], order, space)
        if status[p]:
            continue
        good = w[p] != 0.
        y = np.log(T[p, good]) if space == "loglog" else T[p, good]
        A, b = w[p, good, None] * V[good], w[p, good] * y
        if via == "lstsq":
            a, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
            if rank < order + 1:
                status[p] = SINGULAR
                continue
        else:
            Q, R = np.linalg.qr(A)
            a = solve_triangular(R, Q.T @ b)
        fit = V @ a
        m = np.exp(fit) if space == "loglog" else fit
        coeffs[:, p], model[p] = a, m
        chi2[p] = np.sum((b - A @ a) ** 2)
        cleaned[p] = np.where(good, np.where(good, T[p], 0.) - m, 0.)
    return dict(cleaned=cleaned, coeffs=coeffs, model=model, status=status, chi2=chi2)


# ---- the power-law fit -----------------------------------------------------------------------------------------------------------------
def plaw_cost(amp, beta, d, x, q):
    """half the sum of squares of q (amp x^beta - d) over the channels with q != 0"""
    good = q != 0.
    r = q[good] * (amp * x[good] ** beta - d[good])
    return 0.5 * float(r @ r)


def plaw_guess(d, good, x):
    """(status, d0, b, lower, upper bound of betaS) of one row"""
    idx = np.flatnonzero(good)
    if idx.size < 4:
        return TOO_FEW, np.nan, np.nan, np.nan, np.nan
    if not np.all(np.isfinite(d[good])):
        return NONFINITE, np.nan, np.nan, np.nan, np.nan
    d0, d3 = d[idx[0]], d[idx[3]]
    if not d0 > 0. or not d3 / d0 > 0.:
        return NONPOSITIVE, np.nan, np.nan, np.nan, np.nan
    b = np.log(d3 / d0) / np.log(x[idx[3]] / x[idx[0]])
    return OK, d0, b, min(0.9 * b, 1.1 * b), max(0.9 * b, 1.1 * b)


def plaw_statement(maps, freqs, sigma, w, tpsmean=None, freeind=FREEIND, method="trf"):
    """maps, sigma, w: (rows, N) (sigma, w: arrays broadcast by the caller).  -> dict of bsval, ampS, syamp, ffamp, cost, status,
    guess (b), bounds (rows, 2), residual and model (rows, N)"""
    from scipy.optimize import least_squares
    rows, N = maps.shape
    x = freqs / freqs[0]
    lnx = np.log(x)
    out = dict(bsval=np.full(rows, np.nan), ampS=np.full(rows, np.nan), syamp=np.full(rows, np.nan), ffamp=np.full(rows, np.nan),
               cost=np.full(rows, np.nan), status=np.zeros(rows, dtype=np.int32), bounds=np.full((rows, 2), np.nan), guess=np.full(rows, np.nan),
               residual=np.full((rows, N), np.nan), model=np.full((rows, N), np.nan))
    for p in range(rows):
        good = w[p] != 0.
        d = np.where(good, maps[p] - (tpsmean if tpsmean is not None else 0.), 0.)
        st, d0, b, lo, hi = plaw_guess(d, good, x)
        out["status"][p], out["guess"][p] = st, b
        if st:
            continue
        q = np.where(good, w[p] / sigma[p], 0.)
        qg, dg, lg = q[good], d[good], lnx[good]

        def fun(par):
            return qg * (par[0] * np.exp(par[1] * lg) - dg)

        def jac(par):
            e = qg * np.exp(par[1] * lg)
            return np.stack([e, par[0] * e * lg], axis=1)

        res = least_squares(fun, [0.9 * d0, b], jac=jac, bounds=([0.5 * d0, lo], [1.5 * d0, hi]), method=method, ftol=1e-15,
                            xtol=1e-15, gtol=1e-15, max_nfev=2000)
        amp, beta = res.x
        out["ampS"][p], out["bsval"][p], out["cost"][p], out["bounds"][p] = amp, beta, plaw_cost(amp, beta, d, x, q), (lo, hi)
        S = np.stack([x ** beta, x ** freeind], axis=1)
        if method == "trf":
            amps = np.linalg.lstsq(S[good], dg, rcond=None)[0]
        else:
            amps = np.linalg.solve(S[good].T @ S[good], S[good].T @ dg)
        out["syamp"][p], out["ffamp"][p] = amps
        out["model"][p] = S @ amps
        out["residual"][p] = np.where(good, d - S @ amps, 0.)
    return out


# ---- Gaussian-process regression ---------------------------------------------------------------------------------------------------
def kernel_matrix(kind, variance, lengthscale, N, gradient=False):
    """K (and dK / d ln lengthscale) of a stationary kernel on nu = linspace(0, 1, N)"""
    nu = np.linspace(0., 1., N)
    s = np.abs(nu[:, None] - nu[None, :]) / lengthscale
    if kind == "rbf":
        K = variance * np.exp(-s ** 2 / 2.)
        dK = K * s ** 2
    elif kind == "exponential":
        K = variance * np.exp(-s)
        dK = K * s
    elif kind == "matern32":
        K = variance * (1. + np.sqrt(3.) * s) * np.exp(-np.sqrt(3.) * s)
        dK = variance * 3. * s ** 2 * np.exp(-np.sqrt(3.) * s)
    elif kind == "matern52":
        K = variance * (1. + np.sqrt(5.) * s + 5. * s ** 2 / 3.) * np.exp(-np.sqrt(5.) * s)
        dK = variance * (5. * s ** 2 / 3.) * (1. + np.sqrt(5.) * s) * np.exp(-np.sqrt(5.) * s)
    else:
        raise ValueError(kind)
    return (K, dK) if gradient else K


def gpr_parts(theta, kinds, N):
    """K and the list of dK / dtheta_i for theta = ln [v_1, l_1, ..., noise]"""
    par = np.exp(np.asarray(theta, dtype=np.float64))
    K = par[-1] * np.eye(N)
    grads = []
    for i, kind in enumerate(kinds):
        Ki, dKi = kernel_matrix(kind, par[2 * i], par[2 * i + 1], N, gradient=True)
        K = K + Ki
        grads += [Ki, dKi]
    grads.append(par[-1] * np.eye(N))
    return K, grads


def gpr_lml(theta, gram, npix, kinds, via="cholesky"):
    """(ln L, gradient) through the Gram matrix x^T x of the (npix, N) mean-subtracted data"""
    N = gram.shape[0]
    K, grads = gpr_parts(theta, kinds, N)
    if via == "cholesky":
        L = np.linalg.cholesky(K)
        Kinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(N)))
        logdet = 2. * np.sum(np.log(np.diag(L)))
    else:
        lam, V = np.linalg.eigh(K)
        Kinv = (V / lam) @ V.T
        logdet = np.sum(np.log(lam))
    lnL = -0.5 * (np.sum(Kinv * gram) + npix * logdet + npix * N * np.log(2. * np.pi))
    A = Kinv @ gram @ Kinv - npix * Kinv
    return lnL, np.array([0.5 * np.sum(A * g) for g in grads])


def gpr_matrices(theta, kinds, N, via="cholesky"):
    """M = K_fg K^-1 and cov_fg = K_fg - M K_fg, the first kernel being the foreground"""
    par = np.exp(np.asarray(theta, dtype=np.float64))
    K = gpr_parts(theta, kinds, N)[0]
    K_fg = kernel_matrix(kinds[0], par[0], par[1], N)
    if via == "cholesky":
        L = np.linalg.cholesky(K)
        M = np.linalg.solve(L.T, np.linalg.solve(L, K_fg)).T
    else:
        lam, V = np.linalg.eigh(K)
        M = K_fg @ ((V / lam) @ V.T)
    return M, K_fg - M @ K_fg


def gpr_draw(N, kinds, theta, seed=0, mean_level=5.):
    """(N^2, N) rows drawn from the model, plus a mean spectrum"""
    rs = np.random.RandomState(seed)
    K = gpr_parts(theta, kinds, N)[0]
    L = np.linalg.cholesky(K)
    x = rs.standard_normal((N * N, N)) @ L.T
    return x + mean_level * (1. + np.linspace(0., 1., N)) ** -2.


# ---- scikit-learn as the independent code --------------------------------------------------------------------------------------------
def sklearn_kernel(kinds, theta, bounds=None):
    """C * RBF / Matern(nu) + ... + WhiteKernel at theta = ln [v_1, l_1, ..., noise]; bounds: one (low, high) per parameter"""
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    par = np.exp(np.asarray(theta, dtype=np.float64))
    bnd = list(bounds) if bounds is not None else [(1e-12, 1e12)] * par.size      # (not "fixed": theta would be empty)
    total = None
    for i, kind in enumerate(kinds):
        c = ConstantKernel(par[2 * i], bnd[2 * i])
        if kind == "rbf":
            k = RBF(par[2 * i + 1], bnd[2 * i + 1])
        else:
            k = Matern(par[2 * i + 1], bnd[2 * i + 1], nu={"exponential": 0.5, "matern32": 1.5, "matern52": 2.5}[kind])
        total = c * k if total is None else total + c * k
    return total + WhiteKernel(par[-1], bnd[-1])


def sklearn_regressor(x, kinds, theta, bounds=None, n_restarts=0, seed=0):
    """GaussianProcessRegressor fitted to the mean-subtracted (npix, N) rows as N points with npix targets; without bounds the
    hyperparameters stay as given"""
    from sklearn.gaussian_process import GaussianProcessRegressor
    N = x.shape[1]
    gp = GaussianProcessRegressor(kernel=sklearn_kernel(kinds, theta, bounds), alpha=0., optimizer=None if bounds is None else "fmin_l_bfgs_b",
                                  n_restarts_optimizer=n_restarts, random_state=seed)
    return gp.fit(np.linspace(0., 1., N)[:, None], x.T)


SKLEARN_FTOL = 1e7 * np.finfo(np.float64).eps          # fmin_l_bfgs_b's default factr times eps


# the optimiser case: hyperparameters inside the default bounds of gpr_filter (var = np.var(x) is close to 1)
GPR_KINDS = ("rbf", "exponential")
GPR_TRUTH = np.log([1.0, 0.5, 1e-5, 5e-4, 1e-6])


def default_bounds(var):
    """the reference's bounds (filters.py:559-567) and the noise bounds of gpr_filter"""
    return [(1e-4 * var, 1e2 * var), (1e-3, 1e2), (1e-14 * var, 1e-4 * var), (1e-6, 1e-3), (1e-12 * var, var)]


@functools.lru_cache(maxsize=None)
def sklearn_optima(N, seed=0):
    """ln L at scikit-learn's optimum of the default model on gpr_draw(N, GPR_KINDS, GPR_TRUTH, seed) for two seeds of its
    restarts, from the geometric means of the bounds"""
    x = gpr_draw(N, GPR_KINDS, GPR_TRUTH, seed)
    x = x - x.mean(axis=0)
    bounds = default_bounds(float(np.var(x)))
    start = np.array([0.5 * (np.log(lo) + np.log(hi)) for lo, hi in bounds])
    return [float(sklearn_regressor(x, GPR_KINDS, start, bounds, n_restarts=2, seed=s).log_marginal_likelihood_value_) for s in (0, 1)]
