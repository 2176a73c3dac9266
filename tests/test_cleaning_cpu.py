"""CPU: the numpy statements of NMF, FastICA and band-power PCA cleaning (tests/cleaning_numpy.py) against scikit-learn and
against a direct evaluation of the reference's band-power formula, at N = 16; argument checks that precede the device."""
import warnings

import numpy as np
import pytest

from tests import cleaning_numpy as cn

N = 16


@pytest.fixture(scope="module")
def X():
    return cn.as_matrix(cn.build_cube(N))


@pytest.mark.parametrize("k", [1, 3, 5])
def test_nmf_statement_matches_sklearn(X, k):
    decomposition = pytest.importorskip("sklearn.decomposition")
    rs = np.random.RandomState(5)
    W0, H0 = rs.uniform(0.1, 1., size=(X.shape[0], k)), rs.uniform(0.1, 1., size=(k, N))
    model = decomposition.NMF(n_components=k, init="custom", solver="cd", tol=1e-4, max_iter=200)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ws = model.fit_transform(X, W=W0.copy(), H=H0.copy())
    got = cn.nmf(X, k, W0, H0)
    assert got["n_iter"] == model.n_iter_
    dW = np.max(np.abs(got["W"] - Ws)) / np.max(np.abs(Ws))
    dH = np.max(np.abs(got["H"] - model.components_)) / np.max(np.abs(model.components_))
    assert dW < 1e-12 and dH < 1e-12, (dW, dH)
    assert abs(got["err"] - model.reconstruction_err_) < 1e-9 * model.reconstruction_err_


@pytest.mark.parametrize("k", [1, 3])
def test_nndsvda_statement_matches_sklearn_closely(X, k):
    """scikit-learn's NNDSVDA takes a randomised SVD (10 extra directions, power iterations): with k <= 3 its subspace is the
    whole of these 16 channels and the triplets are those of the exact decomposition up to rounding amplified by the ratio of the
    singular values (4e4 between the first and the third): 1e-8 is 'closely', not 'to rounding'."""
    nmf = pytest.importorskip("sklearn.decomposition._nmf")
    Ws, Hs = nmf._initialize_nmf(X, k, init="nndsvda", random_state=0)
    W, H = cn.nndsvda(X, k)
    dW, dH = np.max(np.abs(W - Ws)) / np.max(np.abs(Ws)), np.max(np.abs(H - Hs)) / np.max(np.abs(Hs))
    assert dW < 1e-8 and dH < 1e-8, (dW, dH)


def test_whitening_routes_agree(X):
    """The covariance route (the device's) against the SVD route (scikit-learn's): the error of the weakest direction is of
    order eps (d_1 / d_n)^2; the cleaned cube, which depends on the span only, is far less sensitive."""
    n = 3
    d = np.linalg.svd(X - X.mean(axis=0), compute_uv=False)
    bound = 100. * np.finfo(np.float64).eps * (d[0] / d[n - 1]) ** 2
    w_init = np.random.RandomState(2).normal(size=(n, n))
    a, b = cn.fastica(X, n, w_init=w_init, route="cov"), cn.fastica(X, n, w_init=w_init, route="svd")
    dev = np.max(np.abs(a["components_"] - b["components_"])) / np.max(np.abs(b["components_"]))
    assert a["n_iter_"] == b["n_iter_"] and dev < bound, (dev, bound)


@pytest.mark.parametrize("fun", ["logcosh", "exp", "cube"])
def test_fastica_statement_matches_sklearn(X, fun):
    decomposition = pytest.importorskip("sklearn.decomposition")
    n = 3
    w_init = np.random.RandomState(2).normal(size=(n, n))
    model = decomposition.FastICA(n_components=n, algorithm="parallel", whiten="unit-variance", fun=fun, w_init=w_init.copy(),
                                  tol=1e-4, max_iter=200)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        S = model.fit_transform(X)
    got = cn.fastica(X, n, fun=fun, w_init=w_init, route="svd")
    assert got["n_iter_"] == model.n_iter_
    d = np.max(np.abs(got["components_"] - model.components_)) / np.max(np.abs(model.components_))
    assert d < 1e-10, d
    assert np.max(np.abs(got["sources"].T - S)) < 1e-8 * np.max(np.abs(S))
    assert np.max(np.abs(got["whitening_"] - model.whitening_)) < 1e-10 * np.max(np.abs(model.whitening_))
    # the cleaned cube: scikit-learn's x - inverse_transform(transform(x)) is the PCA projection
    xc = X - X.mean(axis=0)
    sk_clean = xc - (model.inverse_transform(S) - model.mean_)
    pca_clean = cn.pca(X, n)
    scale = np.max(np.abs(X))
    assert np.max(np.abs(sk_clean - pca_clean)) < 1e-9 * scale
    assert np.max(np.abs(got["cleaned"] - pca_clean)) < 1e-9 * scale


def _reference_formula(cube, nbands, modes):
    """The reference's own steps, complex band-passed cube and unsymmetric eigen-solver included."""
    n = cube.shape[0]
    kx = np.fft.fftfreq(n, d=1.)
    kx, ky = np.meshgrid(kx, kx)
    k = np.sqrt(kx ** 2. + ky ** 2.)
    edges = np.linspace(np.min(k), np.max(k), nbands + 1)
    x = cube - np.mean(cube.reshape((-1, n)), axis=0)[None, None, :]
    total = 0
    for i in range(nbands):
        mask = np.logical_and(k >= edges[i], k < edges[i + 1])
        band = np.fft.ifftn(np.fft.fftn(x, axes=[0, 1]) * mask[:, :, None], axes=[0, 1])
        d = band.reshape((-1, n)).T
        d_mean = np.mean(d, axis=-1)[:, None]
        xx = d - d_mean
        vals, vecs = np.linalg.eig(np.cov(xx))
        U = vecs[:, np.argsort(vals)[::-1]][:, :modes[i]]
        fg = (np.dot(U, np.dot(U.T, xx)) + d_mean).T.reshape(cube.shape)
        total = total + (band - fg)
    return total


@pytest.mark.parametrize("nbands,modes", [(1, 2), (3, 2), (3, [3, 2, 1])])
def test_bandpower_statement_matches_the_reference_formula(nbands, modes):
    cube = cn.build_cube(N)
    want = _reference_formula(cube, nbands, [modes] * nbands if isinstance(modes, int) else modes)
    got = cn.bandpower_pca(cube, nbands, modes)
    scale = np.max(np.abs(cube))
    assert np.max(np.abs(want.imag)) < 1e-9 * scale
    assert np.max(np.abs(got - want.real)) < 1e-9 * scale
    with pytest.raises(AssertionError):
        cn.bandpower_pca(cube, 3, [1, 2])


def test_argument_checks_precede_the_device():
    from fastbox_amd import filters
    cube = np.ones((N, N, N))
    for bad in (0, 17):
        with pytest.raises(ValueError):
            filters.nmf_filter(cube, bad)
        with pytest.raises(ValueError):
            filters.ica_filter(cube, bad)
    with pytest.raises(ValueError):
        filters.nmf_filter(cube, 3, init="random")
    with pytest.raises(ValueError):
        filters.nmf_filter(cube, 3, solver="mu")
    with pytest.raises(ValueError):
        filters.ica_filter(cube, 3, fun="tanh")
    with pytest.raises(AssertionError):
        filters.bandpower_pca_filter(cube, 3, [1, 2])
