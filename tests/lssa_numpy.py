"""The statement of the LSSA definitions and the cases the LSSA tests share.  numpy only.

For a line of sight with data d, flags w, variances var, taper t, delays tau (ns) and frequencies freqs (MHz):
    phi[n, j] = 2 pi tau[n] freqs[j] / 1e3
    g = t^2 w^2 / var where w != 0, else 0;  G = sum_j g;  d is selected away (not multiplied) where g = 0
    A_re = sum_j g d cos phi / G,  A_im = -sum_j g d sin phi / G
    S_cc = sum_j (w cos phi)^2,  S_cs = sum_j (w cos phi)(w sin phi),  S_ss = sum_j (w sin phi)^2
    theta = atan2(2 S_cs, S_cc - S_ss) / 2;  A_1 = cos theta A_re + sin theta A_im,  A_2 = -sin theta A_re + cos theta A_im
    l_0 = cos^2 theta S_cc + 2 sin theta cos theta S_cs + sin^2 theta S_ss,  l_1 = sin^2 theta S_cc - 2 sin theta cos theta S_cs + cos^2 theta S_ss
    ps = ((A_1 l_1)^2 + (A_2 l_0)^2) / (l_0^2 + l_1^2);  without the decorrelation ps = A_re^2 + A_im^2
    a row with G = 0: A = 0, ps = NaN, left out of the averages.
`statement` evaluates the sums directly with np.sum in channel order; via="alt" in reversed channel order with S_cc, S_cs, S_ss
from the double-angle identities 1/2 sum w^2 (1 +- cos 2 phi), 1/2 sum w^2 sin 2 phi: the two differ by rounding only, and that
deviation, relative to max|A| or max|ps| of the case, is the statement's own error (delta_ref).  via="matmul" takes the sums
as matrix products: the whole cube at once, for the averages."""
import functools

import numpy as np


def phase(tau, freqs):
    tau, freqs = np.asarray(tau, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    return 2. * np.pi * tau[:, None] * freqs[None, :] / 1e3


def weights(w, var, taper, shape):
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), shape)
    var = np.broadcast_to(1. if var is None else np.asarray(var, dtype=np.float64), shape)
    t = np.broadcast_to(1. if taper is None else np.asarray(taper, dtype=np.float64), shape)
    with np.errstate(all="ignore"):
        return np.where(w != 0., t * t * w * w / var, 0.), w


def power(A_re, A_im, Scc, Scs, Sss, decorrelate=True):
    if not decorrelate:
        return A_re ** 2 + A_im ** 2
    th = 0.5 * np.arctan2(2. * Scs, Scc - Sss)
    c, s = np.cos(th), np.sin(th)
    A1, A2 = c * A_re + s * A_im, -s * A_re + c * A_im
    l0 = c * c * Scc + 2. * s * c * Scs + s * s * Sss
    l1 = s * s * Scc - 2. * s * c * Scs + c * c * Sss
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((A1 * l1) ** 2 + (A2 * l0) ** 2) / (l0 ** 2 + l1 ** 2)


def statement(d, w, var, taper, tau, freqs, decorrelate=True, via="direct"):
    """(A_re, A_im, ps, G): (rows, Ntau) each and G (rows,).  d: (rows, N); w, var: (rows, N) or (N,); var, taper may be None"""
    d = np.asarray(d, dtype=np.float64)
    g, w = weights(w, var, taper, d.shape)
    u = np.where(g != 0., g * np.where(g != 0., d, 0.), 0.)
    phi = phase(tau, freqs)
    cos, sin = np.cos(phi), np.sin(phi)
    w2 = w * w
    if via == "direct":
        G = np.sum(g, axis=1)
        uc = np.sum(u[:, None, :] * cos[None], axis=2)
        us = np.sum(u[:, None, :] * sin[None], axis=2)
        wc, ws = w[:, None, :] * cos[None], w[:, None, :] * sin[None]
        Scc, Scs, Sss = np.sum(wc * wc, axis=2), np.sum(wc * ws, axis=2), np.sum(ws * ws, axis=2)
    elif via == "alt":
        r = slice(None, None, -1)
        G = np.sum(g[:, r], axis=1)
        uc = np.sum(u[:, None, r] * cos[None, :, r], axis=2)
        us = np.sum(u[:, None, r] * sin[None, :, r], axis=2)
        c2, s2 = np.cos(2. * phi), np.sin(2. * phi)
        Scc = 0.5 * np.sum(w2[:, None, r] * (1. + c2[None, :, r]), axis=2)
        Sss = 0.5 * np.sum(w2[:, None, r] * (1. - c2[None, :, r]), axis=2)
        Scs = 0.5 * np.sum(w2[:, None, r] * s2[None, :, r], axis=2)
    else:
        G = np.sum(g, axis=1)
        uc, us = u @ cos.T, u @ sin.T
        Scc, Scs = w2 @ (cos * cos).T, w2 @ (cos * sin).T
        Sss = np.sum(w2, axis=1)[:, None] - Scc
    on = G > 0.
    with np.errstate(invalid="ignore", divide="ignore"):
        A_re = np.where(on[:, None], uc / G[:, None], 0.)
        A_im = np.where(on[:, None], -us / G[:, None], 0.)
    ps = np.where(on[:, None], power(A_re, A_im, Scc, Scs, Sss, decorrelate), np.nan)
    return A_re, A_im, ps, G


def averages(ps, G):
    """(mean, population standard deviation / sqrt(n_los), n_los) over the rows with G > 0"""
    on = G > 0.
    n = int(on.sum())
    if n == 0:
        return np.full(ps.shape[1], np.nan), np.full(ps.shape[1], np.nan), 0
    return ps[on].mean(axis=0), ps[on].std(axis=0) / np.sqrt(n), n


def delta_ref(a, b):
    """the deviation of two evaluations relative to the largest magnitude; NaN must sit in the same places"""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    big = float(np.max(np.abs(a[ok]))) if ok.any() else 0.
    return (float(np.max(np.abs(a[ok] - b[ok]))) / big if big > 0. else 0.), big


def case_freqs(N):
    """descending, as CosmoBox.freq_array gives; 0.5 MHz channels"""
    return 1000. + 0.5 * np.arange(N, dtype=np.float64)[::-1]


def case_tau(N, ntau):
    """the first ntau delays of the FFT grid of case_freqs(N) (the reference's default expression); past N the grid goes on
    at half steps, off the FFT grid"""
    f = case_freqs(N)
    grid = np.fft.fftfreq(n=N, d=f[1] - f[0]) * 1e3
    if ntau <= N:
        return np.ascontiguousarray(grid[:ntau])
    return np.concatenate([grid, grid[1] * (0.5 + np.arange(ntau - N))])


@functools.lru_cache(maxsize=None)
def build_case(N, per_voxel, noise=None, taper=False, seed=11):
    """d (N^2, N): unit normals plus a sinusoid on the delay grid.  per_voxel flags w (N^2, N): row 0 without a flag, row 1
    with a run of flags, row 2 with a single good channel, row 3 fully flagged, every other row with channel N // 3 flagged and
    3 % of the voxels at random; else w (N,) with channel N // 3 and two more flagged.  noise: None, 'chan' ((N,) variances) or
    'cube' ((N^2, N)).  taper: a Hann window or None.  d_nan holds NaN under the flags of rows 1, 2, 3 and every seventh flagged
    voxel (under every flagged channel for per-channel flags).  Read-only arrays."""
    rs = np.random.RandomState(seed + N)
    npix = N * N
    freqs = case_freqs(N)
    d = rs.standard_normal((npix, N)) + 0.7 * np.cos(phase(case_tau(N, min(3, N))[-1:], freqs)[0] + 0.3)
    if per_voxel:
        w = np.ones((npix, N))
        w[rs.uniform(size=(npix, N)) < 0.03] = 0.
        w[:, N // 3] = 0.
        w[0] = 1.
        w[1] = 1.
        w[1, N // 2:N // 2 + max(2, N // 8)] = 0.
        w[2] = 0.
        w[2, N // 4] = 1.
        w[3] = 0.
        d_nan = d.copy()
        for r in (1, 2, 3):
            d_nan[r, w[r] == 0.] = np.nan
        sel = np.argwhere(w == 0.)[::7]
        d_nan[sel[:, 0], sel[:, 1]] = np.nan
    else:
        w = np.ones(N)
        w[[N // 3, 1, N - 2]] = 0.
        d_nan = d.copy()
        d_nan[:, w == 0.] = np.nan
    var = None
    if noise == "chan":
        var = rs.uniform(0.5, 2.0, size=N)
    elif noise == "cube":
        var = rs.uniform(0.5, 2.0, size=(npix, N))
    case = dict(N=N, d=d, d_nan=d_nan, w=w, var=var, taper=np.hanning(N) if taper else None, freqs=freqs)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case
