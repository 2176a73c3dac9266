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

The second half of the reference's module (inpaint.py:158-399), least-squares spectral analysis of flagged spectra, is served
for the whole cube by one fused kernel (fb_lssa): lssa_fit_modes, lssa_pspec and lssa_delay_spectrum below; trim_flagged_channels
and lssa_decorr_matrix are the reference's host functions.  Definitions and the reference's quirks: DESIGN.md section 4 (LSSA).
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
        return self.engine.download_raw(self.n_iter, (N, N), np.int32)


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
        qbar = np.maximum(eng.download_raw(mean, N), 0.)
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


# ---- least-squares spectral analysis (inpaint.py:158-399) ----------------------------------------------------------------------
NTAU_MAX = 1024


def trim_flagged_channels(w, x):
    """Remove the flagged channels (w != 1) from a 1-D array or from the rows and columns of a square one (inpaint.py:158-183).
    Host arrays.  The device functions below take the untrimmed cube and its flags instead."""
    w, x = np.asarray(w), np.asarray(x)
    if x.shape != (w.size,) and x.shape != (w.size, w.size):
        raise ValueError("x must have shape (w.size,) or (w.size, w.size), got %s" % (x.shape,))
    keep = w.reshape(-1) == 1.
    return x[keep] if x.ndim == 1 else x[:, keep][keep, :]


def lssa_tau(freqs):
    """The default delays in ns of frequencies in MHz: the reference's np.fft.fftfreq(n, d=freqs[1] - freqs[0]) * 1e3
    (inpaint.py:257), sign included (negative for the descending frequencies of freq_array)."""
    freqs = np.asarray(freqs, dtype=np.float64)
    return np.fft.fftfreq(n=freqs.size, d=freqs[1] - freqs[0]) * 1e3


def lssa_phase(tau, freqs):
    """phi[n, j] = 2 pi tau[n] freqs[j] / 1e3 (tau in ns, freqs in MHz), the expression of inpaint.py:343; (Ntau, N) fp64.  Every
    trigonometric table of the device is np.cos / np.sin of this."""
    tau, freqs = np.asarray(tau, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    return 2. * np.pi * tau[:, None] * freqs[None, :] / 1e3


def lssa_decorr_matrix(w, tau, freqs):
    """The rotation that decorrelates the cosine and sine amplitudes of the mode of delay `tau` (a scalar, ns) under the flags
    w, and the eigenvalues of their overlap matrix (inpaint.py:309-361).  Host, one spectrum.  Returns (rot (2, 2), eigvals (2,));
    np.dot(rot, [A_re, A_im]) are the decorrelated amplitudes."""
    w, freqs = np.asarray(w, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    cos = w * np.cos(2. * np.pi * tau * freqs / 1e3)
    sin = w * np.sin(2. * np.pi * tau * freqs / 1e3)
    cov = np.zeros((2, 2))
    cov[0, 0] = np.sum(cos * cos)
    cov[0, 1] = cov[1, 0] = np.sum(cos * sin)
    cov[1, 1] = np.sum(sin * sin)
    theta = 0.5 * np.arctan2(2. * np.sum(cos * sin), np.sum(cos * cos) - np.sum(sin * sin))
    rot = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
    rinv = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    return rot, np.diag(np.dot(rot, np.dot(cov, rinv)))


def _pspec_host(A_re, A_im, w, tau, freqs, decorrelate_amps):
    A_re, A_im = np.asarray(A_re, dtype=np.float64), np.asarray(A_im, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    if A_re.shape != tau.shape or A_im.shape != tau.shape:
        raise ValueError("A_re, A_im and tau must be 1-D arrays of one length")
    if np.shape(w) != np.shape(freqs) or np.ndim(w) != 1:
        raise ValueError("w and freqs must be 1-D arrays of one length")
    if not decorrelate_amps:
        return A_re ** 2. + A_im ** 2.
    ps = np.zeros(tau.size)
    with np.errstate(invalid="ignore"):
        for i, t in enumerate(tau):
            rot, eigvals = lssa_decorr_matrix(w=w, tau=t, freqs=freqs)
            A1, A2 = np.matmul(rot, np.array([A_re[i], A_im[i]]))
            ps[i] = ((A1 * eigvals[1]) ** 2. + (A2 * eigvals[0]) ** 2.) / (eigvals[0] ** 2. + eigvals[1] ** 2.)
    return ps


def _rows_host(eng, buf, ntau):
    return eng.download_raw(buf, (eng.N ** 2, ntau))


class LSSAModes(object):
    """What lssa_fit_modes fitted: A_re, A_im (fp64 (N^2, Ntau) on the device, the amplitude A e^{+i phi} of every line of sight
    and mode), tau (ns), freqs (MHz), n_los (lines of sight with a non-zero total weight; the others have A = 0).  `host()`
    downloads (A_re, A_im) or, for a fit with fit_amp_phase, (|A|, arg A mod 2 pi): the same optimum in the other form."""

    def __init__(self, engine, A_re, A_im, tau, freqs, n_los, fit_amp_phase, inputs):
        self.engine, self.A_re, self.A_im, self.tau, self.freqs, self.n_los = engine, A_re, A_im, tau, freqs, n_los
        self.fit_amp_phase, self._inputs = fit_amp_phase, inputs

    def A_re_host(self):
        return _rows_host(self.engine, self.A_re, self.tau.size)

    def A_im_host(self):
        return _rows_host(self.engine, self.A_im, self.tau.size)

    def host(self):
        re, im = self.A_re_host(), self.A_im_host()
        if not self.fit_amp_phase:
            return re, im
        return np.hypot(re, im), np.mod(np.arctan2(im, re), 2. * np.pi)


class LSSASpectrum(object):
    """An LSSA delay spectrum: tau (ns), ps_mean and ps_stderr (host (Ntau,): over the n_los lines of sight with a non-zero
    total weight, the mean of the per-row power and its population standard deviation / sqrt(n_los), the convention of
    binned_power_spectrum), n_los; ps (fp64 (N^2, Ntau) on the device, NaN in a fully flagged row; `ps_host()`) and modes (the
    LSSAModes) where they were kept, else None."""

    def __init__(self, engine, tau, ps_mean, ps_stderr, n_los, ps=None, modes=None):
        self.engine, self.tau, self.ps_mean, self.ps_stderr, self.n_los, self.ps, self.modes = engine, tau, ps_mean, ps_stderr, n_los, ps, modes

    def ps_host(self):
        if self.ps is None:
            raise ValueError("the per-row power was not kept (keep=True)")
        return _rows_host(self.engine, self.ps, self.tau.size)


def _host_cube_shape(n, a, what):
    """shape check of a host cube before anything reaches the device"""
    if not isinstance(a, DeviceArray) and np.shape(a) not in ((n, n, n), (n * n, n)):
        raise ValueError("%s: expected shape %s or %s, got %s" % (what, (n, n, n), (n * n, n), np.shape(a)))


class _LSSAInputs(object):
    """The validated arguments of one LSSA call on the device: cubes, per-channel vectors and the phase tables."""

    def __init__(self, d, w, freqs, noise, tau, taper, box, need_d=True):
        from .losfit import _frequencies
        eng = _engine_of(d, w, box)
        n = eng.N
        if n > NMAX:
            raise ValueError("LSSA: N <= %d" % NMAX)
        self.freqs = _frequencies(freqs, box, n)
        self.tau = np.ascontiguousarray(lssa_tau(self.freqs) if tau is None else tau, dtype=np.float64)
        if self.tau.ndim != 1 or not 1 <= self.tau.size <= NTAU_MAX or not np.all(np.isfinite(self.tau)):
            raise ValueError("tau: 1 .. %d finite delays, got shape %s" % (NTAU_MAX, self.tau.shape))
        if taper is not None:
            taper = np.ascontiguousarray(taper, dtype=np.float64)
            if taper.shape != (n,) or not np.all(np.isfinite(taper)):
                raise ValueError("taper: expected %d finite values, got shape %s" % (n, taper.shape))
        if need_d:
            if not isinstance(d, DeviceArray) and np.iscomplexobj(d):
                d = np.asarray(d)
                if np.any(d.imag != 0.):
                    raise NotImplementedError("LSSA of complex data is not supported: box cubes are real")
                d = d.real
            _host_cube_shape(n, d, "d")
        w_is_chan = not isinstance(w, DeviceArray) and np.shape(w) == (n,)
        if not w_is_chan:
            _host_cube_shape(n, w, "w")
        if noise is not None and not isinstance(noise, DeviceArray) and np.shape(noise) not in ((n,), (n, n), (n, n, n), (n * n, n)):
            raise ValueError("N: expected (N,) variances, a diagonal (N, N) matrix or a cube, got shape %s" % (np.shape(noise),))
        # ---- the device from here on ----
        self.engine = eng
        self.d = _as_cube(eng, d, "d") if need_d else None
        self.w, self.w_kind, self.w_host = _flags(eng, w)
        self.var, self.var_kind = None, _PER_CHANNEL
        if noise is not None:
            self.var, self.var_kind, _ = _noise(eng, noise)
        self.taper = eng.upload_raw(taper) if taper is not None else None
        phi = lssa_phase(self.tau, self.freqs)
        cos, sin = np.cos(phi), np.sin(phi)
        self.cos, self.sin = eng.upload_raw(cos), eng.upload_raw(sin)
        self.S = None
        if self.w_kind == _PER_CHANNEL:
            c, s = self.w_host * cos, self.w_host * sin
            self.S = eng.upload_raw(np.stack([np.sum(c * c, axis=1), np.sum(c * s, axis=1), np.sum(s * s, axis=1)]))

    def run(self, decorrelate, A_re, A_im, ps, amps_given=False):
        """one fb_lssa call -> (ps_mean, ps_stderr, n_los)"""
        eng, ntau = self.engine, self.tau.size
        mean, err, n_los = np.empty(ntau), np.empty(ntau), _lib.c_i64(0)
        p = lambda b: b.ptr if b is not None else None                       # noqa: E731
        _lib.call("fb_lssa", eng._plan, p(self.d), self.w.ptr, self.w_kind, p(self.var), self.var_kind, p(self.taper), self.cos.ptr,
                  self.sin.ptr, p(self.S), ntau, 1 if decorrelate else 0, 1 if amps_given else 0,
                  p(A_re), p(A_im), p(ps), mean.ctypes.data_as(_lib.P_double), err.ctypes.data_as(_lib.P_double),
                  ctypes.byref(n_los), eng.stream)
        return mean, err, int(n_los.value)

    def rows(self):
        return self.engine._alloc_bytes(self.engine.N ** 2 * self.tau.size * 8)


def lssa_fit_modes(d, w, freqs=None, N=None, tau=None, taper=None, fit_amp_phase=False, box=None):
    """Weighted LSSA fit of every line of sight of a flagged cube (inpaint.py:192-306 with a diagonal inverse covariance): each
    mode n is fitted on its own with the model A e^{+i phi}, phi[n, j] = 2 pi tau_n nu_j / 1e3, minimising sum_j g_j |d_j - A
    e^{i phi}|^2 with g = taper^2 w^2 / sigma^2.  That objective is quadratic in A, so the optimum is closed-form,
    A = sum_j g d e^{-i phi} / sum_j g, where the reference runs one SciPy minimisation per mode.

    Unlike the reference, which takes one spectrum with its flagged channels trimmed away, this takes the untrimmed cube and
    its flags: d, w are REAL DeviceArrays, or host arrays (N, N, N) / (N^2, N) with box=; w may be (N,), one flag per channel.
    d may hold NaN where w = 0.  freqs: (N,) MHz, positive and strictly monotonic, default box.freq_array() (without box=, as
    polynomial_filter, np.linspace(1, 10, N)).  N: the noise
    variance, None (1), (N,), a diagonal (N, N) matrix or a cube.  tau: (Ntau,) ns, 1 <= Ntau <= 1024, default
    lssa_tau(freqs).  taper: (N,) or None.  One phase convention serves the fit and the decorrelation (the reference's fit
    lacks the / 1e3 of its lssa_decorr_matrix and agrees when handed tau / 1e3).  Returns an LSSAModes; fit_amp_phase only
    selects what its host() returns, (A_re, A_im) or (|A|, arg A mod 2 pi)."""
    inp = _LSSAInputs(d, w, freqs, N, tau, taper, box)
    A_re, A_im = inp.rows(), inp.rows()
    _, _, n_los = inp.run(False, A_re, A_im, None)
    return LSSAModes(inp.engine, A_re, A_im, inp.tau, inp.freqs, n_los, bool(fit_amp_phase), inp)


def lssa_pspec(modes_or_A_re, A_im=None, w=None, tau=None, freqs=None, decorrelate_amps=True, box=None):
    """The LSSA power with the decorrelation of the cosine and sine amplitudes (inpaint.py:364-399).

    With 1-D host arrays A_re, A_im, w, tau, freqs: the reference's function, one spectrum on the host; returns ps (Ntau,).
    With an LSSAModes: the per-row power of the whole cube on the device, under the flags the modes were fitted with (or w: a
    cube or (N,) flags of the same box); returns an LSSASpectrum that holds the per-row ps buffer and the modes.
    decorrelate_amps=False returns A_re^2 + A_im^2 (the reference ignores the argument)."""
    if not isinstance(modes_or_A_re, LSSAModes):
        if A_im is None or w is None or tau is None or freqs is None:
            raise TypeError("lssa_pspec of host amplitudes needs A_im, w, tau and freqs")
        return _pspec_host(modes_or_A_re, A_im, w, tau, freqs, decorrelate_amps)
    modes = modes_or_A_re
    if A_im is not None or tau is not None or freqs is not None:
        raise TypeError("lssa_pspec of an LSSAModes takes its amplitudes, delays and frequencies from it")
    inp = modes._inputs
    if w is not None:
        inp = _LSSAInputs(None, w, modes.freqs, None, modes.tau, None, box, need_d=False)
        if inp.engine is not modes.engine:
            raise TypeError("w: expected flags of the same box")
    ps = inp.rows()
    mean, err, n_los = inp.run(decorrelate_amps, modes.A_re, modes.A_im, ps, amps_given=True)
    return LSSASpectrum(modes.engine, modes.tau, mean, err, n_los, ps, modes)


def lssa_delay_spectrum(d, w, freqs=None, N=None, tau=None, taper=None, decorrelate_amps=True, keep=False, box=None):
    """The LSSA delay spectrum of a flagged cube in one fused call: the fit of lssa_fit_modes, the power of lssa_pspec and its
    average over the lines of sight, without storing either per-row array unless keep=True.  Arguments as lssa_fit_modes.
    Returns an LSSASpectrum: tau, ps_mean, ps_stderr (host (Ntau,)), n_los; with keep also ps and modes.  A fully flagged line
    of sight has A = 0 and ps = NaN and is left out of the averages."""
    inp = _LSSAInputs(d, w, freqs, N, tau, taper, box)
    A_re = A_im = ps = modes = None
    if keep:
        A_re, A_im, ps = inp.rows(), inp.rows(), inp.rows()
    mean, err, n_los = inp.run(decorrelate_amps, A_re, A_im, ps)
    if keep:
        modes = LSSAModes(inp.engine, A_re, A_im, inp.tau, inp.freqs, n_los, False, inp)
    return LSSASpectrum(inp.engine, inp.tau, mean, err, n_los, ps, modes)
