"""
Foreground cleaning of a data cube on the device: the step between "add foregrounds and noise" and
"estimate the power spectrum" in the reference's end-to-end flow (examples/example_endtoend.py:105-111).
Same function names, arguments and return values as fastbox/filters.py (:35-56, :93-183).

The cube never leaves HBM: channel means, the frequency-frequency covariance (N^2 pixels x N x N
channels, on the fp64 matrix cores) and the projection run in libfastbox_hip.  The leading eigenvectors
of the N x N covariance come from LAPACK on the host by default (the faster of the two for one small matrix)
or, with `eigensolver="device"`, from fb_leading_eigenvectors (cyclic Jacobi in fp64 on the GPU: the route
of a C-ABI consumer without LAPACK).  The cleaned cube depends only on the span of the modes, so it equals the reference's
(which uses the unsymmetric solver numpy.linalg.eig); individual eigenvectors and mode amplitudes may
differ from the reference's by a sign.

nmf_filter, ica_filter and bandpower_pca_filter (filters.py:187-243, :373-491) follow further down: scikit-learn's
coordinate-descent NMF and parallel FastICA with their per-pixel work in libfastbox_hip (fb_clean.hip) and their k x k
algebra here, and the band-power composition of the band-pass and PCA steps.  Definitions: DESIGN.md section 4.
"""
import ctypes

import numpy as np

from . import _lib
from .device import FULL, REAL, DeviceArray


def _few_blas_threads():
    """An N x N eigenproblem does not feed 64 BLAS threads: on a many-core GPU host the default pool makes it
    10-40x slower (5 ms with two threads, 60-200 ms with 64, measured on the MI355X boxes)."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=2)
    except Exception:
        import contextlib
        return contextlib.nullcontext()


def _as_cube(field, box=None):
    if isinstance(field, DeviceArray):
        if field.kind != REAL:
            raise TypeError("expected a real-space cube")
        return field
    if box is None:
        raise TypeError("a host array needs `box=` (the CosmoBox whose engine holds the cube)")
    return box._as_real(field)


def _channel_means(eng, cube):
    mean = eng._alloc_bytes(eng.N * 8)
    _lib.call("fb_channel_means", eng._plan, cube.ptr, mean.ptr, eng.stream)
    return mean


def mean_spectrum_filter(field, box=None):
    """Subtract the mean of every frequency channel (filters.py:35-56)."""
    cube = _as_cube(field, box)
    eng = cube.engine
    mean = _channel_means(eng, cube)
    out = eng.empty(REAL)
    _lib.call("fb_pca_clean", eng._plan, cube.ptr, mean.ptr, None, 0, out.ptr, None, eng.stream)
    return out


def pca_filter(field, nmodes, fit_powerlaw=False, return_filter=False, box=None, eigensolver="host"):
    """Remove the `nmodes` leading eigenmodes of the empirical frequency-frequency covariance
    (filters.py:93-183).  Returns the cleaned cube (DeviceArray) and, if `return_filter`, the mode matrix
    U_fg (Nfreq, nmodes) and the amplitudes fg_amps (nmodes, Npix) as host arrays.
    eigensolver: "host" (default: LAPACK dsyevr on the downloaded N x N covariance -- 6.5 ms at N = 512) or "device"
    (fb_leading_eigenvectors: cyclic Jacobi in fp64 on the GPU, nothing leaves it and no LAPACK is needed -- 30 ms at
    N = 512, profiles/r04_eigen_bench.txt).  The sign of a mode is not defined in either, as in the reference."""
    if eigensolver not in ("device", "host"):
        raise ValueError("eigensolver: 'device' or 'host'")
    cube = _as_cube(field, box)
    eng = cube.engine
    N = eng.N
    mean_true = _channel_means(eng, cube)
    mean = mean_true
    if fit_powerlaw:
        # filters.py:146-154: x = d - (power-law fit of the mean spectrum) is what the modes are projected out of and
        # what is added back; np.cov(x) (:157-158) still centres every channel on its own mean, so the covariance
        # is taken about the TRUE channel means -- the fit only enters the projection step (N numbers: host)
        from scipy.optimize import curve_fit
        h = eng.download_raw(mean_true, N)
        freqs = np.linspace(1., 10., N)

        def fn(nu, amp, beta):
            return amp * (nu / nu[0]) ** beta
        pfit, _ = curve_fit(fn, freqs, h, p0=[h[0], -2.7])
        mean = eng.upload_raw(np.ascontiguousarray(fn(freqs, pfit[0], pfit[1])))
    cov_dev = eng._alloc_bytes(N * N * 8)
    _lib.call("fb_channel_covariance", eng._plan, cube.ptr, mean_true.ptr, cov_dev.ptr, eng.stream)
    nmodes = int(nmodes)
    if not 0 <= nmodes <= N:
        raise ValueError("nmodes must lie in 0 .. %d" % N)
    # filters.py:161-169: eigenvectors by decreasing eigenvalue, keep nmodes
    U_fg = None
    if eigensolver == "device":
        U_dev = eng._alloc_bytes(max(1, nmodes) * N * 8)
        _lib.call("fb_leading_eigenvectors", eng._plan, cov_dev.ptr, nmodes, U_dev.ptr, None, None, eng.stream)
    else:
        cov = eng.download_raw(cov_dev, (N, N))
        with _few_blas_threads():
            if 0 < nmodes < N:
                from scipy.linalg import eigh      # only the nmodes largest eigenpairs (LAPACK dsyevr)
                w, v = eigh(cov, subset_by_index=[N - nmodes, N - 1])
            else:
                w, v = np.linalg.eigh(cov)
        U_fg = np.ascontiguousarray(v[:, ::-1][:, :nmodes])
        U_dev = eng.upload_raw(U_fg)
    out = eng.empty(REAL)
    amps_dev = eng._alloc_bytes(max(1, nmodes) * N * N * 8) if return_filter else None
    _lib.call("fb_pca_clean", eng._plan, cube.ptr, mean.ptr, U_dev.ptr, int(nmodes), out.ptr,
              amps_dev.ptr if amps_dev is not None else None, eng.stream)
    if not return_filter:
        return out
    fg_amps = eng.download_raw(amps_dev, (nmodes, N * N))
    if U_fg is None:
        U_fg = eng.download_raw(U_dev, (N, nmodes))
    return out, U_fg, fg_amps


def angular_bandpass_filter(field, kmin, kmax, d=1., box=None):
    """Top-hat band-pass in |k_perp| applied to every frequency channel (filters.py:58-90).  Returns the complex
    cube ifftn(fftn(field, axes=[0, 1]) * mask, axes=[0, 1]) as a device array, like the reference's result."""
    if isinstance(field, DeviceArray) and field.kind == FULL:
        eng = field.engine
        cube = eng.clone(field)
    else:
        real = _as_cube(field, box)
        eng = real.engine
        cube = eng.empty(FULL)
        _lib.call("fb_real_to_complex", eng._plan, real.ptr, cube.ptr, eng.stream)
    N = eng.N
    kx = np.fft.fftfreq(N, d=d)                               # :83-86, N^2 numbers on the host
    kx, ky = np.meshgrid(kx, kx)
    k = np.sqrt(kx ** 2. + ky ** 2.)
    mask = np.logical_and(k >= kmin, k < kmax).astype(eng.rdtype)
    mask_dev = eng.upload_raw(np.ascontiguousarray(mask))
    _lib.call("fb_fft_transverse", eng._plan, cube.ptr, -1, eng.stream)
    _lib.call("fb_mask_transverse", eng._plan, cube.ptr, mask_dev.ptr, eng.stream)
    _lib.call("fb_fft_transverse", eng._plan, cube.ptr, +1, eng.stream)
    cube.invalidate()
    return cube


def _check_nmodes(nmodes):
    nmodes = int(nmodes)
    if not 1 <= nmodes <= 16:
        raise ValueError("nmodes must lie in 1 .. 16")
    return nmodes


def _as_state(eng, a, shape, what):
    """A host array or a raw device buffer of `shape` fp64 values -> a device buffer of the filter's own (the caller's
    initial values are not modified)."""
    nbytes = int(np.prod(shape)) * 8
    if isinstance(a, DeviceArray):
        raise TypeError("%s: a host array or a raw device buffer of fp64 values" % what)
    if hasattr(a, "ptr") and hasattr(a, "nbytes"):
        if a.nbytes != nbytes:
            raise ValueError("%s: expected %d bytes on the device" % (what, nbytes))
        out = eng._alloc_bytes(nbytes)
        _lib.call("fb_memcpy_d2d", out.ptr, a.ptr, nbytes, eng.stream)
        return out
    h = np.ascontiguousarray(a, dtype=np.float64)
    if h.shape != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (what, tuple(shape), h.shape))
    return eng.upload_raw(h)


class NMFResult(object):
    """What nmf_filter found: components_ (k, Nfreq) on the host, W (k x Npix fp64 on the device, the layout of pca_filter's
    amplitudes; `W_host()` downloads it as (Npix, k)), n_iter_, reconstruction_err_ = ||X - W H||_F and violations (the
    projected-gradient violation of the W half and of the H half, per iteration)."""

    def __init__(self, engine, components, W, n_iter, err, violations):
        self.engine, self.components_, self.W, self.n_iter_ = engine, components, W, n_iter
        self.reconstruction_err_, self.violations = err, violations
        self.n_components_ = components.shape[0]

    def W_host(self):
        k = self.n_components_
        return np.ascontiguousarray(self.engine.download_raw(self.W, (k, self.engine.N ** 2)).T)


def _nndsvda(eng, cube, k, eps=1e-6):
    """scikit-learn's default initialisation (NNDSVD with zeros filled by the mean of X) from an exact decomposition.  A
    first V from the Nfreq x Nfreq Gram matrix X^T X = (Npix - 1) cov + Npix mean mean^T (eigh on the host); that squares the
    condition number, so the weak directions are then corrected as a one-sided Jacobi method would: B = X V has nearly
    orthogonal columns, B^T B = D C D with D its column norms and C close to the identity (fb_rotated_covariance, B in
    fp64), and the singular values and right vectors of C^(1/2) D, which are those of B, give S and V <- V V_r with the
    accuracy of a decomposition of X itself.  U S = X V from fb_pca_clean with a zero mean; the positive / negative part
    rule is applied on the device for W and here for H."""
    N = eng.N
    npix = N * N
    mean_dev = _channel_means(eng, cube)
    cov_dev = eng._alloc_bytes(N * N * 8)
    _lib.call("fb_channel_covariance", eng._plan, cube.ptr, mean_dev.ptr, cov_dev.ptr, eng.stream)
    mean, cov = eng.download_raw(mean_dev, (N,)), eng.download_raw(cov_dev, (N, N))
    gram = (npix - 1.) * cov + npix * np.outer(mean, mean)
    with _few_blas_threads():
        v = np.linalg.eigh(gram)[1][:, ::-1]
    work = eng._alloc_bytes((N * N * N + N) * 8)
    _lib.call("fb_rotated_covariance", eng._plan, cube.ptr, eng.upload_raw(np.ascontiguousarray(v.T)).ptr, work.ptr, cov_dev.ptr,
              eng.stream)
    gram = eng.download_raw(cov_dev, (N, N)) * (npix - 1.)                # B^T B
    del work
    d = np.sqrt(np.diag(gram))
    d[d == 0.] = 1.
    with _few_blas_threads():
        lam, q = np.linalg.eigh(gram / np.outer(d, d))
        S, vr = np.linalg.svd(((q * np.sqrt(np.maximum(lam, 0.))) @ q.T) * d)[1:]
    S = S[:k]
    V = np.ascontiguousarray(v @ vr[:k].T)                            # (Nfreq, k)
    W = eng._alloc_bytes(k * npix * 8)
    scratch = eng.empty(REAL)
    zero = eng.upload_raw(np.zeros(N))
    _lib.call("fb_pca_clean", eng._plan, cube.ptr, zero.ptr, eng.upload_raw(V).ptr, k, scratch.ptr, W.ptr, eng.stream)   # W = (U S)^T
    norms = np.empty(2 * k)
    _lib.call("fb_nndsvd_norms", eng._plan, W.ptr, k, norms.ctypes.data_as(_lib.P_double), eng.stream)
    avg = float(mean.mean())
    H = np.zeros((k, N))
    coef = np.zeros(k)
    coef[0] = 1. / np.sqrt(S[0])                                       # sqrt(S) |U| = |U S| / sqrt(S)
    H[0] = np.sqrt(S[0]) * np.abs(V[:, 0])
    for j in range(1, k):
        y = V[:, j]
        yp, yn = np.maximum(y, 0.), np.maximum(-y, 0.)
        xp_nrm, xn_nrm = np.sqrt(norms[2 * j]) / S[j], np.sqrt(norms[2 * j + 1]) / S[j]          # of the parts of U_j
        yp_nrm, yn_nrm = np.sqrt(yp @ yp), np.sqrt(yn @ yn)
        mp, mn = xp_nrm * yp_nrm, xn_nrm * yn_nrm
        if mp > mn:
            lbd = np.sqrt(S[j] * mp)
            coef[j], H[j] = lbd / (xp_nrm * S[j]), lbd * yp / yp_nrm
        else:
            lbd = np.sqrt(S[j] * mn)
            coef[j], H[j] = -lbd / (xn_nrm * S[j]), lbd * yn / yn_nrm
    H[H < eps] = avg
    _lib.call("fb_nndsvd_fill", eng._plan, W.ptr, k, coef.ctypes.data_as(_lib.P_double), 1, float(eps), avg, eng.stream)
    return W, eng.upload_raw(H)


def nmf_filter(field, nmodes, return_filter=False, box=None, **kwargs_nmf):
    """Subtract a non-negative matrix factorisation X ~ W H with `nmodes` components from the cube (filters.py:373-432), X =
    the cube as (Npix, Nfreq) without mean subtraction.  The solver is that of sklearn.decomposition.NMF's defaults --
    coordinate descent on the Frobenius loss, no regularisation, no shuffling -- one pass over the cube per iteration
    (fb_nmf_sweep); every other option of scikit-learn's is refused.  kwargs_nmf: tol (1e-4), max_iter (200), init (None or
    'nndsvda': the default initialisation, from an exact decomposition where scikit-learn uses a randomised one, so results
    agree closely with scikit-learn's but not to rounding; or 'custom' with W= (Npix, nmodes) and H= (nmodes, Nfreq) as host
    arrays, or as raw fp64 device buffers of (nmodes, Npix) and (nmodes, Nfreq)).  1 <= nmodes <= 16; a negative or non-finite
    cube raises ValueError.  Returns the cleaned cube X - W H (DeviceArray) and, with return_filter, an NMFResult."""
    nmodes = _check_nmodes(nmodes)
    kw = dict(kwargs_nmf)
    tol, max_iter, init = float(kw.pop("tol", 1e-4)), int(kw.pop("max_iter", 200)), kw.pop("init", None)
    W0, H0 = kw.pop("W", None), kw.pop("H", None)
    if kw:
        raise ValueError("nmf_filter: unsupported options %s" % sorted(kw))
    if init not in (None, "nndsvda", "custom"):
        raise ValueError("nmf_filter: init must be None, 'nndsvda' or 'custom'")
    if (init == "custom") != (W0 is not None and H0 is not None) or (init != "custom" and (W0 is not None or H0 is not None)):
        raise ValueError("nmf_filter: init='custom' goes with both W= and H=")
    if max_iter < 1:
        raise ValueError("nmf_filter: max_iter must be positive")
    cube = _as_cube(field, box)
    eng = cube.engine
    N = eng.N
    npix = N * N
    xmin, bad = ctypes.c_double(), ctypes.c_int64()
    _lib.call("fb_real_min", eng._plan, cube.ptr, ctypes.byref(xmin), ctypes.byref(bad), eng.stream)
    if bad.value:
        raise ValueError("Input contains NaN or infinity.")
    if xmin.value < 0:
        raise ValueError("Negative values in data passed to NMF (input X)")
    if init == "custom":
        if isinstance(W0, np.ndarray) or not hasattr(W0, "ptr"):
            W0 = np.ascontiguousarray(np.asarray(W0, dtype=np.float64).T)
        W, H = _as_state(eng, W0, (nmodes, npix), "W"), _as_state(eng, H0, (nmodes, N), "H")
    else:
        W, H = _nndsvda(eng, cube, nmodes)
    viols = []
    v = np.empty(2)
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        _lib.call("fb_nmf_sweep", eng._plan, cube.ptr, W.ptr, H.ptr, nmodes, v.ctypes.data_as(_lib.P_double), eng.stream)
        viols.append((float(v[0]), float(v[1])))
        v0 = viols[0][0] + viols[0][1]
        if v0 == 0. or (v[0] + v[1]) / v0 <= tol:
            break
    out = eng.empty(REAL)
    ss = ctypes.c_double()
    _lib.call("fb_nmf_residual", eng._plan, cube.ptr, W.ptr, H.ptr, nmodes, out.ptr, ctypes.byref(ss) if return_filter else None,
              eng.stream)
    if not return_filter:
        return out
    return out, NMFResult(eng, eng.download_raw(H, (nmodes, N)), W, n_iter, float(np.sqrt(ss.value)), viols)


class ICAResult(object):
    """What ica_filter found, named as sklearn.decomposition.FastICA names it: components_ (n, Nfreq), mixing_ (Nfreq, n),
    mean_ (Nfreq), whitening_ (n, Nfreq), n_iter_; and sources: n x Npix fp64 on the device (`sources_host()` downloads them
    as (Npix, n), the shape of FastICA.transform's result).  unmixing_ = W K, the components before the unit-variance rule;
    lims = max | |diag(W1 W^T)| - 1 | per iteration."""

    def __init__(self, engine, components, mixing, mean, whitening, n_iter, sources, lims, unmixing):
        self.engine, self.components_, self.mixing_, self.mean_ = engine, components, mixing, mean
        self.whitening_, self.n_iter_, self.sources, self.lims, self.unmixing_ = whitening, n_iter, sources, lims, unmixing

    def sources_host(self):
        n = self.components_.shape[0]
        return np.ascontiguousarray(self.engine.download_raw(self.sources, (n, self.engine.N ** 2)).T)


_ICA_FUN = {"logcosh": 0, "exp": 1, "cube": 2}           # FB_ICA_LOGCOSH, FB_ICA_EXP, FB_ICA_CUBE


def _sym_decorrelation(W):
    """W <- (W W^T)^(-1/2) W"""
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return (u * (1. / np.sqrt(s))) @ u.T @ W


def ica_filter(field, nmodes, return_filter=False, box=None, eigensolver="host", **kwargs_ica):
    """Subtract the `nmodes` independent components FastICA finds in the mean-subtracted cube (filters.py:187-243).

    The cleaned cube is x - pinv(W K) (W K) x, the projection of x off the row space of the whitening matrix K: the span of the
    nmodes leading principal directions, whatever the (invertible) unmixing matrix W.  It therefore EQUALS pca_filter(field,
    nmodes) and is formed by the same kernel from the same modes; without return_filter no ICA iteration is run at all.

    With return_filter an ICAResult follows: FastICA with algorithm='parallel', whiten='unit-variance' on the device
    (fb_ica_step: g(W X1) X1^T / Npix and the means of g' in one pass over the whitened data X1, n x Npix fp64; the n x n
    symmetric decorrelation on the host).  kwargs_ica: fun ('logcosh', 'exp' or 'cube'), fun_args ({'alpha': 1.0} for
    logcosh), tol (1e-4), max_iter (200), w_init ((n, n) array), random_state (seeds the normal draw of w_init when that is
    missing, as scikit-learn does); every other option of scikit-learn's is refused.  1 <= nmodes <= 16.  eigensolver: 'host'
    or 'device', handed to pca_filter, which finds the principal directions."""
    nmodes = _check_nmodes(nmodes)
    kw = dict(kwargs_ica)
    fun, fun_args = kw.pop("fun", "logcosh"), dict(kw.pop("fun_args", None) or {})
    tol, max_iter = float(kw.pop("tol", 1e-4)), int(kw.pop("max_iter", 200))
    w_init, random_state = kw.pop("w_init", None), kw.pop("random_state", None)
    if kw.pop("algorithm", "parallel") != "parallel" or kw.pop("whiten", "unit-variance") != "unit-variance" or kw:
        raise ValueError("ica_filter: only algorithm='parallel', whiten='unit-variance'; unsupported options %s" % sorted(kw))
    if fun not in _ICA_FUN:
        raise ValueError("ica_filter: fun must be 'logcosh', 'exp' or 'cube'")
    alpha = float(fun_args.pop("alpha", 1.0))
    if fun_args or not 1. <= alpha <= 2.:
        raise ValueError("ica_filter: fun_args takes alpha in [1, 2] only")
    if max_iter < 1:
        raise ValueError("ica_filter: max_iter must be positive")
    cube = _as_cube(field, box)
    eng = cube.engine
    N = eng.N
    npix = N * N
    n = nmodes
    if n > N:
        raise ValueError("nmodes must not exceed the number of channels")
    if not return_filter:
        return pca_filter(cube, nmodes, eigensolver=eigensolver)
    out, U, _ = pca_filter(cube, n, return_filter=True, eigensolver=eigensolver)
    # whitening: the singular values of the centred data are d_i = sqrt(lambda_i (Npix - 1)), lambda_i = u_i^T cov u_i
    mean_dev = _channel_means(eng, cube)
    cov_dev = eng._alloc_bytes(N * N * 8)
    _lib.call("fb_channel_covariance", eng._plan, cube.ptr, mean_dev.ptr, cov_dev.ptr, eng.stream)
    mean, cov = eng.download_raw(mean_dev, (N,)), eng.download_raw(cov_dev, (N, N))
    lam = np.einsum("ci,cd,di->i", U, cov, U)
    d = np.sqrt(lam * (npix - 1.))
    u = U * np.sign(U[0])
    K = np.ascontiguousarray((u / d).T)
    X1 = eng._alloc_bytes(n * npix * 8)
    scratch = eng.empty(REAL)
    _lib.call("fb_pca_clean", eng._plan, cube.ptr, mean_dev.ptr, eng.upload_raw(np.ascontiguousarray(K.T * np.sqrt(npix))).ptr,
              n, scratch.ptr, X1.ptr, eng.stream)
    del scratch
    if w_init is None:
        w_init = np.random.RandomState(random_state).normal(size=(n, n))
    w_init = np.asarray(w_init, dtype=np.float64)
    if w_init.shape != (n, n):
        raise ValueError("w_init has invalid shape -- should be %s" % ((n, n),))
    W = np.ascontiguousarray(_sym_decorrelation(w_init))
    G, gp = np.empty((n, n)), np.empty(n)
    lims = []
    for _ in range(max_iter):
        _lib.call("fb_ica_step", eng._plan, W.ctypes.data_as(_lib.P_double), X1.ptr, n, _ICA_FUN[fun], alpha,
                  G.ctypes.data_as(_lib.P_double), gp.ctypes.data_as(_lib.P_double), eng.stream)
        W1 = np.ascontiguousarray(_sym_decorrelation(G - gp[:, None] * W))
        lims.append(float(np.max(np.abs(np.abs(np.einsum("ij,ij->i", W1, W)) - 1.))))
        W = W1
        if lims[-1] < tol:
            break
    # sources S = W K x = W X1 / sqrt(Npix), then scikit-learn's unit-variance rule (std over pixels, ddof = 0)
    sources = eng._alloc_bytes(n * npix * 8)
    scale = np.full(n, 1. / np.sqrt(npix))
    mom = np.empty(2 * n)
    _lib.call("fb_ica_sources", eng._plan, W.ctypes.data_as(_lib.P_double), scale.ctypes.data_as(_lib.P_double), X1.ptr, n,
              sources.ptr, mom.ctypes.data_as(_lib.P_double), eng.stream)
    std = np.sqrt(mom[n:] - mom[:n] ** 2)
    scale = scale / std
    _lib.call("fb_ica_sources", eng._plan, W.ctypes.data_as(_lib.P_double), scale.ctypes.data_as(_lib.P_double), X1.ptr, n,
              sources.ptr, None, eng.stream)
    WK = W @ K
    comps = WK / std[:, None]
    return out, ICAResult(eng, comps, np.linalg.pinv(comps), mean, K, len(lims), sources, lims, WK)


def bandpower_pca_filter(field, nbands, modes, box=None):
    """Split the mean-subtracted cube into `nbands` contiguous top-hat bands of equal width in |k_perp|, PCA-clean every band
    with its own number of modes and add the results (filters.py:435-491).  modes: an int, or one value per band.  The band
    edges are linspace(min |k|, max |k|, nbands + 1) over the fftfreq grid; like the reference's, the last band's `< kmax`
    leaves out the single largest |k|.  The reference hands the complex band-passed cube to pca_filter; its imaginary part is
    rounding error (the mask is symmetric under k -> -k), and here the real part is taken on the device first.  The sum runs
    on the device (fb_real_axpby)."""
    nbands = int(nbands)
    if isinstance(modes, (int, np.integer)):
        modes = int(modes) * np.ones(nbands, dtype=int)
    assert nbands == len(modes), "len(modes) must equal nbands"
    cube = _as_cube(field, box)
    eng = cube.engine
    kx = np.fft.fftfreq(eng.N, d=1.)
    kx, ky = np.meshgrid(kx, kx)
    k = np.sqrt(kx ** 2. + ky ** 2.)
    band_edges = np.linspace(np.min(k), np.max(k), nbands + 1)
    x = mean_spectrum_filter(cube)
    total = None
    for i in range(nbands):
        band = angular_bandpass_filter(x, kmin=band_edges[i], kmax=band_edges[i + 1])
        real = eng.empty(REAL)
        _lib.call("fb_complex_to_real", eng._plan, band.ptr, real.ptr, eng.stream)
        del band
        cleaned = pca_filter(real, int(modes[i]))
        total = cleaned if total is None else eng.axpby(total, cleaned, 1.0, 1.0, 0.0)
    return total


# polynomial_filter, LSQfitting and gpr_filter (filters.py:494-664): fits along the line of sight, in fastbox_amd/losfit.py
from .losfit import (GPRKernel, GPRResult, LOSFit, LSQResult, LSQfitting, gpr_filter, polynomial_filter)    # noqa: E402,F401
