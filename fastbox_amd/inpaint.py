"""
In-painting of flagged frequency channels by Gaussian constrained realisations, on the device: fastbox/inpaint.py:8-155
for a whole cube at once.  Same function names and arguments as the reference; the cube is (N, N, N) with frequency along
the last axis, a line of sight (ix, iy) being one row of the reference's (Npix, Nfreq) view.

For every line of sight p with flags w (1 good, 0 flagged), diagonal noise variance sigma^2 and signal prior S:

    q_p = w_p^2 / sigma_p^2                          (exactly 0 where w = 0, whatever sigma and d hold there)
    A_p = I + S^(1/2) diag(q_p) S^(1/2)
    b_p = S^(1/2) (q_p d_p + sqrt(q_p) omega2) + omega1,     omega1, omega2 unit normals
    A_p x_p = b_p,    s_p = S^(1/2) x_p

solved for all N^2 lines of sight together by preconditioned conjugate gradients in fp64 (fb_gcr_solve: the products along the
frequency axis run on the fp64 matrix cores).  S^(1/2) and the preconditioner P = (I + S^(1/2) diag(qbar) S^(1/2))^-1 -- one
N x N matrix for every pixel, qbar the channel's weight without flags -- come from LAPACK on the host.  With per-channel noise
A_p differs from P^-1 by a matrix whose rank is the number of flagged channels k_p of the pixel, so a row needs at most k_p + 1
iterations in exact arithmetic.  Definitions, differences from the reference and measurements: DESIGN.md section 4.
"""
import ctypes

import numpy as np

from . import _lib
from .device import REAL, DeviceArray
from .filters import _few_blas_threads

NMAX = 1024                      # about nine fp64 cubes of working memory: 9 GiB at 512^3, 72 GiB at 1024^3
_PER_CHANNEL, _PER_VOXEL = 0, 1  # FB_GCR_PER_CHANNEL, FB_GCR_PER_VOXEL
_NONE, _GIVEN, _DEVICE = 0, 1, 2  # FB_GCR_DRAWS_*
_X_PLAN, _X_FP64 = 0, 1          # FB_LOS_X_*


def simple_signal_cov(freqs, amplitude, width, ridge_var=1e-10):
    """Gaussian correlation function of the given width (in frequency units) times `amplitude`, plus ridge_var on the
    diagonal (inpaint.py:8-32).  Host array (Nfreq, Nfreq)."""
    freqs = np.asarray(freqs, dtype=np.float64)
    nu, nup = np.meshgrid(freqs, freqs)
    return amplitude * np.exp(-0.5 * (nu - nup) ** 2. / width ** 2.) + ridge_var * np.eye(freqs.size)


class GCRInfo(object):
    """What the solver did: n_iter (int32 (N, N) on the device; `n_iter_host()` downloads it), max_iter_ (the largest
    iteration count of a line of sight), converged (lines of sight that met the tolerance; N^2 when all did), residual
    (max_p |b - A x| / |b| from one more application of A).  With several realisations these describe the last one and
    `per_realisation` lists (max_iter_, converged, residual) of each."""

    def __init__(self, engine, n_iter, max_iter, converged, residual, per_realisation):
        self.engine, self.n_iter, self.max_iter_, self.converged, self.residual = engine, n_iter, max_iter, converged, residual
        self.per_realisation = per_realisation

    def n_iter_host(self):
        N = self.engine.N
        h = np.empty((N, N), dtype=np.int32)
        _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), self.n_iter.ptr, h.nbytes, self.engine.stream)
        return h


def _engine_of(d, w, box):
    for a in (d, w):
        if isinstance(a, DeviceArray):
            return a.engine
    if box is None:
        raise TypeError("host arrays need `box=` (the CosmoBox whose engine holds the cube)")
    return box.engine


def _as_cube(eng, a, what):
    """REAL DeviceArray of this engine, or a host array (N, N, N) / (N^2, N) -> DeviceArray"""
    N = eng.N
    if isinstance(a, DeviceArray):
        if a.kind != REAL or a.engine is not eng:
            raise TypeError("%s: expected a real-space cube of the same box" % what)
        return a
    h = np.asarray(a)
    if np.iscomplexobj(h):
        h = h.real
    if h.shape == (N * N, N):
        h = h.reshape(N, N, N)
    if h.shape != (N, N, N):
        raise ValueError("%s: expected shape %s or %s, got %s" % (what, (N, N, N), (N * N, N), h.shape))
    return eng.upload(h, REAL)


def _flags(eng, w):
    """-> (device object, kind, host (N,) copy for per-channel flags or None)"""
    if not isinstance(w, DeviceArray):
        h = np.asarray(w)
        if h.shape == (eng.N,):
            h = np.ascontiguousarray(h, dtype=np.float64)
            return eng.upload_raw(h), _PER_CHANNEL, h
    return _as_cube(eng, w, "w"), _PER_VOXEL, None


def _noise(eng, Nv):
    """-> (device object, kind, host (N,) variances or None).  A matrix must be diagonal (exactly)."""
    N = eng.N
    if isinstance(Nv, DeviceArray):
        return _as_cube(eng, Nv, "N"), _PER_VOXEL, None
    h = np.asarray(Nv, dtype=np.float64)
    if h.shape == (N, N) and N != 1:
        diag = np.diag(h)
        if np.max(np.abs(h - np.diag(diag))) != 0.:
            raise NotImplementedError("gaussian_cr_1d: a noise covariance with off-diagonal terms is not supported")
        h = diag
    if h.shape == (N,):
        h = np.ascontiguousarray(h)
        if not np.all(h > 0.):
            raise ValueError("N: noise variances must be positive")
        return eng.upload_raw(h), _PER_CHANNEL, h
    return _as_cube(eng, h, "N"), _PER_VOXEL, None


def _sqrt_psd(S):
    with _few_blas_threads():
        lam, V = np.linalg.eigh(S)
    return np.ascontiguousarray((V * np.sqrt(np.maximum(lam, 0.))) @ V.T)


def _preconditioner(eng, sqrtS, var_dev, var_kind, var_host, w_dev, w_kind, w_host):
    """P = (I + S^(1/2) diag(qbar) S^(1/2))^-1: qbar = 1 / sigma^2 for per-channel noise, else the channel mean of q."""
    N = eng.N
    if var_kind == _PER_CHANNEL:
        qbar = 1. / var_host
    else:
        # q does not depend on the data (any cube of the plan's precision stands in for it); its channel means come from the same call
        q = eng._alloc_bytes(N ** 3 * 8)
        u = eng._alloc_bytes(N ** 3 * 8)
        mean = eng._alloc_bytes(N * 8)
        _lib.call("fb_gcr_rhs", eng._plan, w_dev.ptr if w_kind == _PER_VOXEL else var_dev.ptr, w_dev.ptr, w_kind, var_dev.ptr,
                  var_kind, None, _NONE, 0, 0, q.ptr, u.ptr, None, mean.ptr, eng.stream)
        qbar = np.empty(N)
        _lib.call("fb_memcpy_d2h", qbar.ctypes.data_as(ctypes.c_void_p), mean.ptr, qbar.nbytes, eng.stream)
        qbar = np.maximum(qbar, 0.)
    # through eigh: A >= I, so every eigenvalue of P is taken from (0, 1] and P is positive definite whatever cond A
    with _few_blas_threads():
        A = np.eye(N) + (sqrtS * qbar) @ sqrtS
        lam, V = np.linalg.eigh(0.5 * (A + A.T))
    return np.ascontiguousarray((V / np.maximum(lam, 1.)) @ V.T)


def _solve(d, w, S, N, realisations, add_noise, precondition, cg_maxiter, verbose, box, tol, draws, inpaint):
    eng = _engine_of(d, w, box)
    n = eng.N
    if n > NMAX:
        raise ValueError("in-painting holds about nine fp64 cubes: N <= %d" % NMAX)
    tol, cg_maxiter, realisations = float(tol), int(cg_maxiter), int(realisations)
    if not tol > 0.:
        raise ValueError("tol must be positive")
    if cg_maxiter < 1:
        raise ValueError("cg_maxiter must be at least 1")
    if realisations < 1:
        raise ValueError("realisations must be at least 1")
    S = np.asarray(S, dtype=np.float64)
    if S.shape != (n, n):
        raise ValueError("S must have shape (Nfreq, Nfreq) = %s, got %s" % ((n, n), S.shape))
    if not np.all(np.isfinite(S)) or np.max(np.abs(S - S.T)) > 1e-12 * np.max(np.abs(S)):
        raise ValueError("S must be a finite symmetric matrix")
    d_dev = _as_cube(eng, d, "d")
    w_dev, w_kind, w_host = _flags(eng, w)
    var_dev, var_kind, var_host = _noise(eng, N)
    sqrtS = _sqrt_psd(0.5 * (S + S.T))
    sqrtS_dev = eng.upload_raw(sqrtS)
    P_dev = None
    if precondition:
        P_dev = eng.upload_raw(_preconditioner(eng, sqrtS, var_dev, var_kind, var_host, w_dev, w_kind, w_host))
    numpy_rng = box is not None and box.rng == "numpy"
    seed = 0
    om1 = om2 = om3 = None
    if draws:
        if box is None:
            raise TypeError("random draws follow the box (`box=`): rng='numpy' or rng='device'")
        if numpy_rng:
            # the reference's order (inpaint.py:120-141): per pixel, per realisation, omega1 then omega2
            om = np.random.randn(n * n, realisations, 2, n)
            if add_noise:
                om3 = np.random.randn(realisations, n * n, n)
        else:
            from .sky import _Maps
            seed = _Maps(box).next_seed()
    nbytes = n ** 3 * 8
    q, u, b, x = [eng._alloc_bytes(nbytes) for _ in range(4)]
    work = eng._alloc_bytes((5 if precondition else 4) * nbytes)
    n_iter = eng._alloc_bytes(n * n * 4)
    info = np.zeros(4)
    outs, stats = [], []
    for i in range(realisations):
        mode = _NONE if not draws else (_GIVEN if numpy_rng else _DEVICE)
        om1_dev = om2_dev = om3_dev = None
        if mode == _GIVEN:
            om1_dev = eng.upload_raw(np.ascontiguousarray(om[:, i, 0, :]))
            om2_dev = eng.upload_raw(np.ascontiguousarray(om[:, i, 1, :]))
        _lib.call("fb_gcr_rhs", eng._plan, d_dev.ptr, w_dev.ptr, w_kind, var_dev.ptr, var_kind,
                  om2_dev.ptr if om2_dev is not None else None, mode, seed, i, q.ptr, u.ptr, b.ptr if mode == _DEVICE else None,
                  None, eng.stream)
        add = om1_dev.ptr if mode == _GIVEN else (b.ptr if mode == _DEVICE else None)
        _lib.call("fb_los_matmul", eng._plan, sqrtS_dev.ptr, u.ptr, _X_FP64, None, None, add, b.ptr, eng.stream)
        _lib.call("fb_gcr_solve", eng._plan, sqrtS_dev.ptr, P_dev.ptr if P_dev is not None else None, q.ptr, b.ptr, x.ptr, work.ptr,
                  tol, cg_maxiter, n_iter.ptr, info.ctypes.data_as(_lib.P_double), eng.stream)
        stats.append((int(info[2]), int(info[1]), float(info[0])))
        noise = _NONE
        if draws and add_noise:
            noise = mode
            if mode == _GIVEN:
                om3_dev = eng.upload_raw(np.ascontiguousarray(om3[i]))
        out = eng.empty(REAL)
        _lib.call("fb_gcr_finish", eng._plan, sqrtS_dev.ptr, x.ptr, u.ptr, var_dev.ptr, var_kind,
                  om3_dev.ptr if om3_dev is not None else None, noise, seed, i, d_dev.ptr, w_dev.ptr, w_kind, 1 if inpaint else 0,
                  out.ptr, eng.stream)
        eng.sync()                     # the uploaded draws of this realisation are dropped next
        outs.append(out)
    if verbose:
        print("    constrained realisations: %d x %d lines of sight, %d channels; at most %d CG iterations, residual %.2e, "
              "%d converged" % (realisations, n * n, n, max(s[0] for s in stats), max(s[2] for s in stats),
                                min(s[1] for s in stats)))
    return outs, GCRInfo(eng, n_iter, stats[-1][0], stats[-1][1], stats[-1][2], stats)


def gaussian_cr_1d(d, w, S, N, realisations=1, add_noise=True, precondition=True, cg_maxiter=10000, verbose=True, box=None,
                   tol=1e-10, return_info=False):
    """Gaussian constrained realisations of the signal of a flagged cube (inpaint.py:35-155).

    d, w: REAL DeviceArrays, or host arrays (N, N, N) / (N^2, N) with box=; w may be (N,), one flag per channel.  d may hold NaN
    where w = 0.  S: (N, N) signal prior covariance.  N: the noise, an (N, N) diagonal matrix, (N,) variances or a cube-shaped
    variance (a matrix with off-diagonal terms raises NotImplementedError).  The draws follow the box: rng='numpy' takes
    np.random.randn in the reference's order, rng='device' the counter generator (streams 7-9, fastbox_amd.rng.gcr_normals).
    add_noise adds sigma times an independent third draw.  precondition=False runs plain CG.  Returns a list of `realisations`
    REAL DeviceArrays and, with return_info, a GCRInfo.  Prints one line per call when verbose."""
    outs, info = _solve(d, w, S, N, realisations, add_noise, precondition, cg_maxiter, verbose, box, tol, True, False)
    return (outs, info) if return_info else outs


def wiener_filter_1d(d, w, S, N, precondition=True, cg_maxiter=10000, verbose=False, box=None, tol=1e-10, return_info=False):
    """The Wiener-filter mean S (S + N_w)^-1 d of every line of sight: the same solve with zero draws."""
    outs, info = _solve(d, w, S, N, 1, False, precondition, cg_maxiter, verbose, box, tol, False, False)
    return (outs[0], info) if return_info else outs[0]


def inpaint_cube(d, w, S, N, precondition=True, cg_maxiter=10000, verbose=False, box=None, tol=1e-10, return_info=False):
    """d where it is not flagged (bit for bit) and one constrained realisation of the signal (without added noise) where it
    is: a cube without holes for the FFT-based estimators."""
    outs, info = _solve(d, w, S, N, 1, False, precondition, cg_maxiter, verbose, box, tol, True, True)
    return (outs[0], info) if return_info else outs[0]
