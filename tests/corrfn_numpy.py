"""numpy restatement of CosmoBox.correlation_function (the definition its kernels implement), in two independent forms:

    (a) xi_fft:   D_a = rfftn(d_a - mean(d_a)),  xi(s) = irfftn(conj(D_1) D_2, s=(N, N, N)) / N^3
    (b) xi_brute: xi(s) = (1/N^3) sum_x (d_1(x) - mean)(d_2(x + s) - mean), a sum over all cell pairs (N <= 16)

and the binning both share: s_a = m_a (L_a / N), m_a the signed FFT index (Nyquist negative); |s| = sqrt((s_x s_x + s_y s_y)
+ s_z s_z); mu = s_z / |s| (0 at s = 0); bin = np.digitize(|s|, edges) - 1; npairs, mean |s|, (2l+1) sum xi L_l / npairs."""
import math

import numpy as np


def signed_index(N):
    i = np.arange(N)
    return np.where(i < N // 2, i, i - N)


def xi_fft(d1, d2=None):
    N = d1.shape[0]
    D1 = np.fft.rfftn(d1 - d1.mean())
    D2 = D1 if d2 is None else np.fft.rfftn(d2 - d2.mean())
    return np.fft.irfftn(np.conj(D1) * D2, s=d1.shape, axes=(0, 1, 2)) / float(N) ** 3


def xi_brute(d1, d2=None):
    N = d1.shape[0]
    assert N <= 16, "brute force: up to 16^3 (4096^2 pairs)"
    a = d1 - d1.mean()
    b = a if d2 is None else d2 - d2.mean()
    out = np.empty_like(a)
    for i in range(N):
        for j in range(N):
            for l in range(N):
                # d_2(x + s): the field rolled back by s
                out[i, j, l] = np.sum(a * np.roll(b, (-i, -j, -l), axis=(0, 1, 2))) / float(N) ** 3
    return out


def legendre(l, mu):
    m2 = mu * mu
    if l == 0:
        return np.ones_like(mu)
    if l == 2:
        return 1.5 * m2 - 0.5
    if l == 4:
        return ((35. * m2 - 30.) * m2 + 3.) * 0.125
    raise ValueError(l)


def separation_axes(N, L, edges=None):
    """Per axis: the indices to visit and their s_a.  With edges, only |m_a| <= floor(e_last N / L_a) + 1 (cells beyond
    cannot reach a bin) -- the same cells are dropped either way, this only saves time."""
    m = signed_index(N)
    out = []
    for La in L:
        idx = np.arange(N)
        if edges is not None and np.isfinite(edges[-1]):
            M = np.floor(edges[-1] * N / La) + 1
            idx = idx[np.abs(m) <= M]
        out.append((idx, m[idx] * (La / N)))
    return out


def bin_xi(xi, L, edges, poles=(0,)):
    """(r, xi_l [len(poles), nbins], npairs) of a real field xi on the separation grid."""
    N = xi.shape[0]
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    (ix, sx), (iy, sy), (iz, sz) = separation_axes(N, L, edges)
    x = xi[np.ix_(ix, iy, iz)]
    sx, sy, sz = sx[:, None, None], sy[None, :, None], sz[None, None, :]
    S = np.sqrt((sx * sx + sy * sy) + sz * sz)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(S > 0, sz / S, 0.)
    b = np.digitize(S, edges) - 1
    ok = (b >= 0) & (b < nb)
    bv = b[ok]
    npairs = np.bincount(bv, minlength=nb).astype(np.float64)
    # sum |s| per bin correctly rounded (math.fsum): bins of 10^5 cells would otherwise carry 1e-13 of summation error
    order = np.argsort(bv, kind="stable")
    sv, cut = S[ok][order], np.searchsorted(bv[order], np.arange(nb + 1))
    sum_r = np.array([math.fsum(sv[cut[q]:cut[q + 1]]) for q in range(nb)])
    sums = [np.bincount(bv, weights=(x * legendre(l, mu))[ok], minlength=nb) for l in poles]
    with np.errstate(invalid="ignore", divide="ignore"):
        empty = npairs == 0
        r = np.where(empty, np.nan, sum_r / npairs)
        xil = np.array([np.where(empty, np.nan, (2 * l + 1) * s / npairs) for l, s in zip(poles, sums)])
    return r, xil, npairs


def correlation_function(d1, d2, L, edges, poles=(0,), brute=False):
    """(r, xi_l, npairs) of the auto- (d2 None) or cross-correlation; brute: form (b) instead of (a)."""
    xi = (xi_brute if brute else xi_fft)(np.asarray(d1, dtype=np.float64), None if d2 is None else np.asarray(d2, dtype=np.float64))
    return bin_xi(xi, L, edges, poles)
