"""numpy statements of the halo tracers (fastbox_amd/halos.py): expected counts, the catalogue order, periodic NGP / CIC /
TSC painting with np.add.at and compensation with np.fft.  Test helpers, not product code."""
import numpy as np


def expected_counts(delta, nbar, bias, L, lognormal=False):
    """lam of halos.py:92-114 (nbar, bias: scalar, z-profile or (N,N,N)); NaN -> 0."""
    N = delta.shape[-1]
    nbar = np.atleast_1d(np.asarray(nbar, dtype=np.float64))
    bias = np.atleast_1d(np.asarray(bias, dtype=np.float64))
    if nbar.ndim == 1:
        nbar = nbar[np.newaxis, np.newaxis, :]
    if bias.ndim == 1:
        bias = bias[np.newaxis, np.newaxis, :]
    voxel_vol = L[0] * L[1] * L[2] / N ** 3.
    dh = bias * delta
    if lognormal:
        dh = np.exp(dh)
        dh /= np.mean(dh)
        dh -= 1.
    lam = voxel_vol * nbar * (1. + dh)
    if not lognormal:
        lam[np.where(lam < 0.)] = 0.
    return np.nan_to_num(lam)


def catalogue(counts, L, u=None):
    """Positions in the reference's order: ascending count, voxels in C order, each repeated `count` times;
    (index + u) * (L_a / N).  u: (Nh, 3) offsets or None."""
    counts = np.asarray(counts).astype(np.int64)
    N = counts.shape[0]
    flat = counts.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] > 0]
    vox = np.repeat(order, flat[order])
    idx = np.stack(np.unravel_index(vox, counts.shape), axis=-1).astype(np.float64)
    if u is not None:
        idx = idx + u
    return idx * (np.asarray(L, dtype=np.float64) / N)


def _axis(u, window, N):
    if window == "ngp":
        return [(np.floor(u + 0.5), np.ones_like(u))]
    if window == "cic":
        f0 = np.floor(u)
        f = u - f0
        return [(f0, 1. - f), (f0 + 1., f)]
    c = np.floor(u + 0.5)
    d = u - c
    return [(c - 1., 0.5 * (0.5 - d) ** 2), (c, 0.75 - d * d), (c + 1., 0.5 * (0.5 + d) ** 2)]


def paint(pos, N, L, window="cic", weights=None, compensated=False):
    """Particles with a position that is not finite are skipped, as fb_paint skips them."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    w = np.ones(pos.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    ok = np.all(np.isfinite(pos), axis=1)
    pos, w = pos[ok], w[ok]
    mesh = np.zeros((N, N, N))
    ax = [_axis(pos[:, a] * (N / L[a]), window, N) for a in range(3)]
    for m0, w0 in ax[0]:
        for m1, w1 in ax[1]:
            for m2, w2 in ax[2]:
                i = [np.mod(m, N).astype(np.int64) for m in (m0, m1, m2)]
                np.add.at(mesh, tuple(i), w * w0 * w1 * w2)
    if compensated:
        p = {"ngp": 1, "cic": 2, "tsc": 3}[window]
        m = np.fft.fftfreq(N) * N
        s = np.sinc(m / N) ** p                    # np.sinc(x) = sin(pi x) / (pi x)
        W = s[:, None, None] * s[None, :, None] * s[None, None, :]
        mesh = np.fft.ifftn(np.fft.fftn(mesh) / W).real
    return mesh
