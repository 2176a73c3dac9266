"""Numpy statements of the three cleaning functions of fastbox_amd.filters that are not PCA -- nmf_filter, ica_filter and
bandpower_pca_filter -- written from their definitions, for the CPU and GPU tests to compare with.

    X is the cube as (Npix, Nfreq), a pixel's spectrum in a row.

nmf_cd         scikit-learn's coordinate-descent NMF solver (Frobenius loss, no regularisation, no shuffling)
nndsvda        its default initialisation, with an exact SVD in place of the randomised one
fastica        FastICA, algorithm 'parallel', whiten 'unit-variance', with scikit-learn's sign and unit-variance rules
bandpower_pca  the band-power PCA composition
build_cube     the test cubes: non-Gaussian positive maps times power laws, plus small positive noise
"""
import numpy as np


# ---- the test cubes -----------------------------------------------------------------------------------------------------------
SPECTRA = ((-2.7, 1e3), (-2.1, 30.), (-3.2, 3.))


def build_cube(N, seed=1, ncomp=3, noise=1e-2):
    """(N, N, N) positive cube, frequency last: component i is a non-Gaussian positive map (uniform, shifted Laplace, |sin| of a
    Gaussian, in turn) times a power law in nu = 1 .. 2; the first three are nu^-2.7 1e3, nu^-2.1 30 and nu^-3.2 3."""
    rng = np.random.RandomState(seed)
    nu = np.linspace(1., 2., N)
    out = noise * rng.uniform(0.05, 1., size=(N, N, N))
    for i in range(ncomp):
        kind = i % 3
        if kind == 0:
            m = rng.uniform(0.5, 1.5, size=(N, N))
        elif kind == 1:
            m = np.abs(rng.laplace(0., 0.3, size=(N, N)) + 1.) + 0.05
        else:
            m = np.abs(np.sin(3. * rng.normal(size=(N, N)))) + 0.05
        beta, amp = SPECTRA[i] if i < 3 else (-2.4 - 0.15 * i, 1.)
        out += m[:, :, None] * (amp * nu ** beta)[None, None, :]
    return out


def as_matrix(cube):
    return np.ascontiguousarray(np.asarray(cube).reshape((-1, cube.shape[-1])))


# ---- NMF ----------------------------------------------------------------------------------------------------------------------
def _cd_half(X, W, Ht):
    """One cyclic pass over the columns of W (every row independently), in place.  Returns the violation."""
    HHt = Ht.T @ Ht
    XHt = X @ Ht
    viol = 0.
    for t in range(W.shape[1]):
        grad = -XHt[:, t]
        for r in range(W.shape[1]):                    # in this order, as the definition is written
            grad = grad + HHt[t, r] * W[:, r]
        pg = np.where(W[:, t] == 0., np.minimum(0., grad), grad)
        viol += np.abs(pg).sum()
        if HHt[t, t] != 0.:
            W[:, t] = np.maximum(W[:, t] - grad / HHt[t, t], 0.)
    return viol


def nmf_cd(X, W0, H0, tol=1e-4, max_iter=200):
    """X ~ W H from (W0, H0).  Returns W, H, n_iter and the list of (violation of the W half, of the H half) per iteration."""
    W = np.array(W0, dtype=np.float64)
    Ht = np.array(np.asarray(H0, dtype=np.float64).T, order="C")
    viols = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        vw = _cd_half(X, W, Ht)
        vh = _cd_half(X.T, Ht, W)
        viols.append((vw, vh))
        v0 = viols[0][0] + viols[0][1]
        if v0 == 0. or (vw + vh) / v0 <= tol:
            break
    return W, np.ascontiguousarray(Ht.T), n_iter, viols


def nndsvda(X, k, eps=1e-6):
    """NNDSVD of the k leading singular triplets with zeros filled by the mean of X (Boutsidis & Gallopoulos 2008)."""
    U, S, Vt = np.linalg.svd(X, full_matrices=False)
    U, S, Vt = U[:, :k], S[:k], Vt[:k]
    W, H = np.zeros_like(U), np.zeros_like(Vt)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0] = np.sqrt(S[0]) * np.abs(Vt[0])
    for j in range(1, k):
        x, y = U[:, j], Vt[j]
        xp, yp, xn, yn = np.maximum(x, 0.), np.maximum(y, 0.), np.maximum(-x, 0.), np.maximum(-y, 0.)
        mp = np.sqrt(xp @ xp) * np.sqrt(yp @ yp)
        mn = np.sqrt(xn @ xn) * np.sqrt(yn @ yn)
        if mp > mn:
            u, v, sigma = xp / np.sqrt(xp @ xp), yp / np.sqrt(yp @ yp), mp
        else:
            u, v, sigma = xn / np.sqrt(xn @ xn), yn / np.sqrt(yn @ yn), mn
        W[:, j] = np.sqrt(S[j] * sigma) * u
        H[j] = np.sqrt(S[j] * sigma) * v
    avg = X.mean()
    W[W < eps] = avg
    H[H < eps] = avg
    return W, H


def nmf(X, k, W0=None, H0=None, tol=1e-4, max_iter=200):
    """The whole filter: returns a dict with the cleaned matrix X - W H, W, H, n_iter, the violations and the error norm."""
    if W0 is None:
        W0, H0 = nndsvda(X, k)
    W, H, n_iter, viols = nmf_cd(X, W0, H0, tol, max_iter)
    res = X - W @ H
    return dict(cleaned=res, W=W, H=H, n_iter=n_iter, viols=viols, err=np.sqrt((res * res).sum()))


# ---- FastICA ------------------------------------------------------------------------------------------------------------------
def sym_decorrelation(W):
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return (u * (1. / np.sqrt(s))) @ u.T @ W


def contrast(fun, y, alpha=1.):
    """g(y) and the mean over pixels of g'(y), row by row."""
    if fun == "logcosh":
        g = np.tanh(alpha * y)
        return g, (alpha * (1. - g * g)).mean(axis=-1)
    if fun == "exp":
        e = np.exp(-(y * y) / 2.)
        return y * e, ((1. - y * y) * e).mean(axis=-1)
    if fun == "cube":
        return y ** 3, (3. * y * y).mean(axis=-1)
    raise ValueError(fun)


def whiten(X, n, route="cov"):
    """mean (Nfreq), K (n, Nfreq), X1 (n, Npix) = K (X - mean)^T sqrt(Npix): the n leading principal directions u_i scaled to
    unit variance, each with its first entry positive.  route 'cov': u_i and d_i = sqrt(lambda_i (Npix - 1)) from the
    eigenpairs of the channel covariance, as fastbox_amd.filters forms them; route 'svd': from the singular value decomposition
    of the centred data, as scikit-learn does.  The same numbers in exact arithmetic; in fp64 the covariance squares the
    condition number, so the weakest of the n directions carries a relative error of order eps (d_1 / d_n)^2 on route 'cov'."""
    npix = X.shape[0]
    mean = X.mean(axis=0)
    xc = X - mean
    if route == "svd":
        u, d = np.linalg.svd(xc.T, full_matrices=False)[:2]
        u, d = u[:, :n], d[:n]
    else:
        lam, u = np.linalg.eigh(xc.T @ xc / (npix - 1.))
        lam, u = lam[::-1][:n], u[:, ::-1][:, :n]
        d = np.sqrt(lam * (npix - 1.))
    u = u * np.sign(u[0])
    K = (u / d).T
    return mean, K, (K @ xc.T) * np.sqrt(npix)


def fastica(X, n, fun="logcosh", alpha=1., w_init=None, random_state=None, tol=1e-4, max_iter=200, route="cov"):
    """Returns a dict: components_ (n, Nfreq), mixing_, mean_, whitening_, n_iter_, sources (n, Npix), unmixing (W K before the
    unit-variance rule), lims (max | |diag(W1 W^T)| - 1 | per iteration) and cleaned (X minus its projection on the sources)."""
    npix = X.shape[0]
    mean, K, X1 = whiten(X, n, route)
    if w_init is None:
        w_init = np.random.RandomState(random_state).normal(size=(n, n))
    W = sym_decorrelation(np.asarray(w_init, dtype=np.float64))
    lims = []
    for _ in range(max_iter):
        g, gp = contrast(fun, W @ X1, alpha)
        W1 = sym_decorrelation(g @ X1.T / float(npix) - gp[:, None] * W)
        lims.append(np.max(np.abs(np.abs(np.einsum("ij,ij->i", W1, W)) - 1.)))
        W = W1
        if lims[-1] < tol:
            break
    WK = W @ K
    xc = X - mean
    S = WK @ xc.T
    std = S.std(axis=1)
    comps = WK / std[:, None]
    mixing = np.linalg.pinv(comps)
    cleaned = xc - (mixing @ (comps @ xc.T)).T
    return dict(components_=comps, mixing_=mixing, mean_=mean, whitening_=K, n_iter_=len(lims), sources=S / std[:, None],
                unmixing=WK, lims=lims, cleaned=cleaned)


# ---- PCA and the band-power composition ---------------------------------------------------------------------------------------
def pca(X, m):
    """X minus the channel means minus the projection on the m leading eigenvectors of the channel covariance."""
    xc = X - X.mean(axis=0)
    if m == 0:
        return xc
    lam, u = np.linalg.eigh(xc.T @ xc / (X.shape[0] - 1.))
    u = u[:, ::-1][:, :m]
    return xc - (xc @ u) @ u.T


def band_edges(N, nbands):
    k = np.fft.fftfreq(N)
    k = np.sqrt(k[None, :] ** 2. + k[:, None] ** 2.)
    return k, np.linspace(k.min(), k.max(), nbands + 1)


def bandpower_pca(cube, nbands, modes, dtype=np.float64):
    """Sum over nbands equal-width bands in |k_perp| of PCA-cleaned band-passed cubes; of every band-passed cube the real part is
    taken (its imaginary part is rounding error: the mask is symmetric under k -> -k).  dtype: the precision in which the
    mean-subtracted cube is held and transformed (np.float32: what an f32 plan does); the PCA and the sum stay in fp64."""
    cube = np.asarray(cube, dtype=np.float64)
    N = cube.shape[0]
    if isinstance(modes, (int, np.integer)):
        modes = [int(modes)] * nbands
    assert nbands == len(modes), "len(modes) must equal nbands"
    k, edges = band_edges(N, nbands)
    x = (cube - cube.mean(axis=(0, 1))).astype(dtype)
    fx = np.fft.fftn(x, axes=[0, 1])
    out = np.zeros_like(cube)
    for i in range(nbands):
        mask = np.logical_and(k >= edges[i], k < edges[i + 1])
        band = np.fft.ifftn(fx * mask[:, :, None], axes=[0, 1]).real.astype(np.float64)
        out += pca(as_matrix(band), int(modes[i])).reshape(cube.shape)
    return out
