"""CPU: the statements of tests/losfit_numpy.py against independent code (numpy's legfit, scipy's two bounded least-squares
methods against each other, scikit-learn's Gaussian-process likelihood, gradient and prediction), and the host half of
fastbox_amd.losfit (kernels, likelihood through the Gram matrix, optimiser) against the same."""
import numpy as np
import pytest

from fastbox_amd import filters, losfit
from tests import losfit_numpy as ln

EPS = 2. ** -52


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- the polynomial fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["loglog", "semilog", "linear"])
@pytest.mark.parametrize("order", [0, 1, 3, 7])
def test_polynomial_statement_matches_legfit(order, space):
    """numpy.polynomial.legendre.legfit(t, y, order, w=w) solves the same weighted problem by its own scaled lstsq.  The design
    has condition <= 8 here (asserted), so two backward-stable solvers agree to a small multiple of cond 2^-52."""
    c = ln.build_case(16)
    nu = c["freqs"]
    u = nu if space == "linear" else np.log(nu)
    t = 2. * (u - u.min()) / (u.max() - u.min()) - 1.
    rows = np.arange(4, 68)
    a = ln.poly_statement(c["d"][rows], c["w"][rows], nu, order, space, via="lstsq")
    b = ln.poly_statement(c["d"][rows], c["w"][rows], nu, order, space, via="qr")
    fitted = 0
    for i, p in enumerate(rows):
        good = c["w"][p] != 0.
        if a["status"][i]:
            assert a["status"][i] == ln.TOO_FEW and good.sum() < order + 1
            continue
        fitted += 1
        V = ln.legendre_design(nu, order, space)
        cond = np.linalg.cond(c["w"][p, good, None] * V[good])
        y = np.log(c["d"][p, good]) if space == "loglog" else c["d"][p, good]
        want = np.polynomial.legendre.legfit(t[good], y, order, w=c["w"][p, good])
        scale = np.max(np.abs(want))
        for name, got in (("lstsq", a["coeffs"][:, i]), ("qr", b["coeffs"][:, i])):
            dev = np.max(np.abs(got - want)) / scale
            assert dev <= 100. * cond * EPS, "row %d, %s: deviation %.3e, cond %.1f" % (p, name, dev, cond)
    assert fitted >= 60
    assert np.array_equal(a["status"], b["status"])


def test_product_basis_is_the_statements_basis():
    for space in ("loglog", "linear"):
        nu = ln.frequencies(24)
        got = losfit.legendre_basis(nu if space == "linear" else np.log(nu), 7)
        want = ln.legendre_design(nu, 7, space).T
        assert _rel(got, want) <= 64. * EPS


# ---- the power-law fit -----------------------------------------------------------------------------------------------------------------
def test_power_law_statement_two_methods_agree_and_the_bound_row_sits_on_its_bound():
    """trf and dogbox from the same start under the tightest tolerances scipy accepts.  A minimum located from double-precision
    residuals is known to about sqrt(2^-52) = 1.5e-8 relative in its position; measured here 1e-9.  dogbox returns the bound
    exactly; trf keeps its iterates strictly inside the box and returns the next double (4.4e-16 away)."""
    N = 16
    c = ln.build_case(N)
    a = ln.plaw_statement(c["d_nan"], c["freqs"], c["sigma"], c["w"], method="trf")
    b = ln.plaw_statement(c["d_nan"], c["freqs"], c["sigma"], c["w"], method="dogbox")
    assert np.array_equal(a["status"], b["status"])
    failed = np.flatnonzero(a["status"])
    assert list(failed) == [ln.ROW_EMPTY, ln.ROW_NEGATIVE] and list(a["status"][failed]) == [ln.TOO_FEW, ln.NONPOSITIVE]
    ok = a["status"] == 0
    for k in ("ampS", "bsval"):
        spread = _rel(a[k][ok], b[k][ok])
        assert spread <= 1e-7, "%s: trf to dogbox %.3e" % (k, spread)
    for r in (a, b):
        dist = np.min(np.abs(r["bsval"][:, None] - r["bounds"]), axis=1) / np.abs(r["bsval"])
        on = np.flatnonzero(ok & (dist <= 4. * EPS))
        assert list(on) == [ln.ROW_BOUND], "rows on a bound: %s" % on
        assert abs(r["bsval"][ln.ROW_BOUND] - r["bounds"][ln.ROW_BOUND, 0]) <= 4. * EPS * abs(r["bsval"][ln.ROW_BOUND])
        assert np.all(np.isfinite(r["ampS"][ok])) and np.all(np.isfinite(r["cost"][ok]))
    assert np.array_equal(b["bsval"][ln.ROW_BOUND], b["bounds"][ln.ROW_BOUND, 0])
    # the two second stages (lstsq, normal equations) give the same residual
    big = np.max(np.abs(a["residual"][ok]))
    assert np.max(np.abs(a["residual"][ok] - b["residual"][ok])) / big <= 1e-6
    assert np.all(a["residual"][ok][c["w"][ok] == 0.] == 0.)


# ---- Gaussian-process regression ---------------------------------------------------------------------------------------------------
def _gpr_case(kinds, N=16, npix=64, seed=3):
    theta = np.log([4.0, 0.3, 0.05, 0.02, 1e-3][:2 * len(kinds)] + [1e-3])
    x = ln.gpr_draw(N, kinds, theta, seed)[:npix]
    x = x - x.mean(axis=0)
    return theta, x, x.T @ x


@pytest.mark.parametrize("kinds", [("rbf", "exponential"), ("rbf", "matern32"), ("matern52", "exponential")])
def test_gram_route_likelihood_and_gradient_match_scikit_learn(kinds):
    """ln L and its gradient from the N x N Gram matrix against scikit-learn's log_marginal_likelihood on the multi-target data
    (which works on the data themselves).  Bounds: 10 cond(K) 2^-52 times the magnitude of the terms that are summed -- for ln L
    |tr K^-1 G| + npix |ln det K| + npix N ln 2 pi, for each gradient component |tr K^-1 G K^-1 dK| / 2 + npix |tr K^-1 dK| / 2."""
    theta, x, gram = _gpr_case(kinds)
    npix, N = x.shape
    gp = ln.sklearn_regressor(x, kinds, theta)
    want, want_grad = gp.log_marginal_likelihood(theta, eval_gradient=True)
    K, grads = ln.gpr_parts(theta, kinds, N)
    cond = np.linalg.cond(K)
    Kinv = np.linalg.inv(K)
    scale = abs(np.sum(Kinv * gram)) + npix * abs(np.linalg.slogdet(K)[1]) + npix * N * np.log(2. * np.pi)
    gscale = np.array([0.5 * abs(np.sum((Kinv @ gram @ Kinv) * g)) + 0.5 * npix * abs(np.sum(Kinv * g)) for g in grads])
    kernels = [filters.GPRKernel(k) for k in kinds]
    cases = [("statement, cholesky", ln.gpr_lml(theta, gram, npix, kinds)), ("statement, eigh", ln.gpr_lml(theta, gram, npix, kinds, via="eigh")),
             ("product", losfit.gpr_log_likelihood(theta, gram, npix, kernels, eval_gradient=True))]
    for name, (got, got_grad) in cases:
        assert abs(got - want) <= 10. * cond * EPS * scale, "%s: ln L off by %.3e (relative %.3e), cond %.2e" % (
            name, abs(got - want), abs(got - want) / abs(want), cond)
        excess = np.abs(got_grad - want_grad) / (10. * cond * EPS * gscale)
        assert np.all(excess <= 1.), "%s: gradient off by %s, cond %.2e, largest error / bound %.3f" % (
            name, np.abs(got_grad - want_grad), cond, excess.max())
    assert losfit.gpr_log_likelihood(theta, gram, npix, kernels) == cases[2][1][0]


def test_prediction_matches_scikit_learn():
    """scikit-learn's predict at the training points is (K - noise I) K^-1 y: the sum of the foreground projections M with either
    kernel first.  Both evaluations of the statement and the product's gpr_projection."""
    kinds = ("rbf", "exponential")
    theta, x, gram = _gpr_case(kinds)
    npix, N = x.shape
    gp = ln.sklearn_regressor(x, kinds, theta)
    want = gp.predict(np.linspace(0., 1., N)[:, None]).T
    swapped = theta[[2, 3, 0, 1, 4]]
    cond = np.linalg.cond(ln.gpr_parts(theta, kinds, N)[0])
    par = np.exp(theta)
    for via in ("cholesky", "eigh", "product"):
        if via == "product":
            k1, k2 = filters.GPRKernel("rbf", par[0], par[1]), filters.GPRKernel("exponential", par[2], par[3])
            M1, c1, _ = losfit.gpr_projection([k1, k2], par[4], N)
            M2, c2, _ = losfit.gpr_projection([k2, k1], par[4], N)
        else:
            M1, c1 = ln.gpr_matrices(theta, kinds, N, via)
            M2, c2 = ln.gpr_matrices(swapped, kinds[::-1], N, via)
        got = x @ (M1 + M2).T
        dev = _rel(got, want)
        assert dev <= 10. * cond * EPS, "%s: prediction off by %.3e, cond %.2e" % (via, dev, cond)
        # cov_fg = K_fg - K_fg K^-1 K_fg is symmetric and positive semi-definite up to rounding
        assert _rel(c1, c1.T) <= 10. * cond * EPS and np.linalg.eigvalsh(0.5 * (c1 + c1.T)).min() >= -10. * cond * EPS * np.abs(c1).max()
    # the product's M and cov_fg against the statement's two evaluations; cov_fg is a difference of terms of size |K_fg|
    a, b = ln.gpr_matrices(theta, kinds, N), ln.gpr_matrices(theta, kinds, N, "eigh")
    kfg = float(np.max(np.abs(ln.kernel_matrix("rbf", par[0], par[1], N))))
    assert _rel(M1, a[0]) <= 10. * cond * EPS and _rel(b[0], a[0]) <= 10. * cond * EPS
    assert np.max(np.abs(c1 - a[1])) <= 10. * cond * EPS * kfg and np.max(np.abs(b[1] - a[1])) <= 10. * cond * EPS * kfg


def test_kernel_argument_errors():
    with pytest.raises(ValueError):
        filters.GPRKernel("cubic")
    with pytest.raises(ValueError):
        filters.GPRKernel("rbf", variance=-1.)
    with pytest.raises(ValueError):
        filters.GPRKernel("rbf", lengthscale_bounds=(1., 0.5))
    k = filters.GPRKernel("matern32", 2., 0.3)
    r = np.abs(np.linspace(0., 1., 8)[:, None] - np.linspace(0., 1., 8)[None, :])
    assert _rel(k.matrix(r), ln.kernel_matrix("matern32", 2., 0.3, 8)) <= 8. * EPS
    # d K / d ln l against a central difference
    h = 1e-5
    num = (k.matrix(r, lengthscale=0.3 * np.exp(h)) - k.matrix(r, lengthscale=0.3 * np.exp(-h))) / (2. * h)
    assert np.max(np.abs(k.matrix(r, gradient=True)[1] - num)) <= 1e-8


def test_host_optimiser_from_a_numpy_gram():
    """gpr_optimize on x^T x of a cube drawn from known hyperparameters inside the default bounds: ln L at its optimum is not
    below ln L at the generating hyperparameters, and not below scikit-learn's optimum of the same kernel and bounds by more
    than the spread of scikit-learn's own optima over two seeds of its restarts (floor: its L-BFGS-B ftol times |ln L|)."""
    N = 16
    x = ln.gpr_draw(N, ln.GPR_KINDS, ln.GPR_TRUTH, 0)
    x = x - x.mean(axis=0)
    npix = x.shape[0]
    gram = x.T @ x
    var = float(np.var(x))
    kernels = losfit.default_gpr_kernels(var)
    bounds = ln.default_bounds(var)
    assert [k.variance_bounds for k in kernels] == [bounds[0], bounds[2]] and [k.lengthscale_bounds for k in kernels] == [bounds[1], bounds[3]]
    theta, lnL, n_starts, log = losfit.gpr_optimize(gram, npix, kernels, 1.0, bounds[4], num_restarts=10, random_state=0)
    assert n_starts == 11 == len(log)
    lo, hi = np.log(bounds).T
    assert np.all(theta >= lo) and np.all(theta <= hi)
    assert abs(lnL - ln.gpr_lml(theta, gram, npix, ln.GPR_KINDS)[0]) <= 1e-9 * abs(lnL)
    truth = ln.gpr_lml(ln.GPR_TRUTH, gram, npix, ln.GPR_KINDS)[0]
    assert lnL >= truth, "ln L %.10e at the optimum, %.10e at the generating hyperparameters" % (lnL, truth)
    sk = ln.sklearn_optima(N)
    slack = max(abs(sk[0] - sk[1]), ln.SKLEARN_FTOL * abs(max(sk)))
    assert lnL >= max(sk) - slack, "ln L %.10e, scikit-learn's optima %.10e and %.10e (slack %.3e)" % (lnL, sk[0], sk[1], slack)
    # the same draw and the same starts: the same optimum, bit for bit
    again = losfit.gpr_optimize(gram, npix, kernels, 1.0, bounds[4], num_restarts=10, random_state=0)
    assert np.array_equal(again[0], theta) and again[1] == lnL
