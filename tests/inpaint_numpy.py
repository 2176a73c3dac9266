"""The dense per-pixel statement of the constrained-realisation definition and the cases the in-painting
tests share.  numpy only.

For a line of sight with flags w, variances var, data d and unit normals om1, om2:
    q = w^2 / var where w != 0, else 0;  A = I + S^(1/2) diag(q) S^(1/2);  b = S^(1/2) (q d + sqrt(q) om2) + om1  (d is selected,
    not multiplied, where w = 0);  s = S^(1/2) A^-1 b.
`statement` solves with np.linalg.solve, `statement(..., via="eigh")` through the eigen-decomposition of A: the two differ by
rounding only, and that deviation is the reference's own error (delta_ref)."""
import functools

import numpy as np


def simple_signal_cov(freqs, amplitude, width, ridge_var=1e-10):
    nu, nup = np.meshgrid(freqs, freqs)
    return amplitude * np.exp(-0.5 * (nu - nup) ** 2. / width ** 2.) + ridge_var * np.eye(freqs.size)


def sqrt_psd(S):
    lam, V = np.linalg.eigh(S)
    return (V * np.sqrt(np.maximum(lam, 0.))) @ V.T


def weights(w, var):
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(w != 0., w * w / var, 0.)


def rhs(d, w, S, var, om1=None, om2=None):
    """b (Npix, Nfreq) and q"""
    q = weights(w, np.broadcast_to(var, np.shape(d)))
    u = np.where(q != 0., q * np.where(q != 0., d, 0.), 0.)
    if om2 is not None:
        u = u + np.sqrt(q) * om2
    b = u @ sqrt_psd(S).T
    if om1 is not None:
        b = b + om1
    return b, q


def statement(d, w, S, var, om1=None, om2=None, via="solve"):
    """s (Npix, Nfreq): one dense solve per line of sight"""
    d = np.asarray(d, dtype=np.float64)
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), d.shape)
    b, q = rhs(d, w, S, var, om1, om2)
    rS = sqrt_psd(S)
    n = d.shape[1]
    out = np.empty_like(b)
    for p in range(d.shape[0]):
        A = np.eye(n) + (rS * q[p]) @ rS
        if via == "solve":
            x = np.linalg.solve(A, b[p])
        else:
            lam, V = np.linalg.eigh(0.5 * (A + A.T))
            x = V @ ((V.T @ b[p]) / lam)
        out[p] = rS @ x
    return out


@functools.lru_cache(maxsize=None)
def build_case(N, per_voxel_noise=False, max_flags=None, seed=3):
    """S = simple_signal_cov(amplitude 1, width N / 12 channels), var = 1e-2, d = a draw from S plus noise, (N^2, N).  The flags
    always include: pixel 0 without a flag, pixel 1 with one flagged channel, pixel 2 with a run, pixel 3 fully flagged; unless
    max_flags is given also a channel flagged in every pixel and 3 % of the voxels at random (with max_flags: up to that many
    random channels per pixel and no common channel, the well-conditioned case of the iteration-count test).  NaN is written
    into d under the flags of pixels 1, 2 and 3 and every seventh flagged voxel.  Read-only arrays."""
    rs = np.random.RandomState(seed + N)
    npix = N * N
    S = simple_signal_cov(np.arange(N, dtype=np.float64), 1.0, N / 12.)
    var = np.full(N, 1e-2)
    if per_voxel_noise:
        var = 1e-2 * rs.uniform(0.5, 2.0, size=(npix, N))
    d = rs.standard_normal((npix, N)) @ sqrt_psd(S).T + np.sqrt(var) * rs.standard_normal((npix, N))
    w = np.ones((npix, N))
    if max_flags is None:
        w[rs.uniform(size=(npix, N)) < 0.03] = 0.
        w[:, N // 3] = 0.
        w[0] = 1.
        w[0, N // 3] = 0.
    else:
        for p in range(npix):
            k = rs.randint(0, max_flags + 1)
            w[p, rs.choice(N, size=k, replace=False)] = 0.
        w[0] = 1.
    w[1] = 1.
    w[1, 2] = 0.
    w[2] = 1.
    w[2, N // 2:N // 2 + max(2, N // 8)] = 0.
    w[3] = 0.
    if max_flags is None:
        w[1, N // 3] = w[2, N // 3] = 0.
    d_nan = d.copy()
    flagged = np.argwhere(w == 0.)
    for r in (1, 2, 3):
        d_nan[r, w[r] == 0.] = np.nan
    sel = flagged[::7]
    d_nan[sel[:, 0], sel[:, 1]] = np.nan
    case = dict(N=N, S=S, var=var, d=d, d_nan=d_nan, w=w, nflag=(w == 0.).sum(axis=1))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def nan_channel_mean(cube):
    """the reference's replace_nan_with_channel_mean (analysis.py:5-28) on an (Npix, Nfreq) view; also returns the means"""
    out = np.array(cube, dtype=np.float64, copy=True)
    means = np.full(out.shape[1], np.nan)
    for j in range(out.shape[1]):
        bad = np.isnan(out[:, j])
        if not bad.all():
            means[j] = np.mean(out[~bad, j])
        out[bad, j] = means[j]
    return out, means
