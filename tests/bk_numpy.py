"""Numpy statement of CosmoBox.bispectrum (the definition in include/fastbox_hip.h at fb_bispectrum): the FFT triangle-bin
estimator in fp64, and the explicit sum over mode pairs it must equal.

    D = fftn(d);  k_a = m_a (2 pi / L_a), m_a the signed FFT index (Nyquist negative);
    |k| = sqrt((k_x k_x + k_y k_y) + k_z k_z);  shell S_b = {m != 0 : np.digitize(|k|, edges) - 1 == b};
    I_b(x) = sum_{m in S_b} D(m) exp(+2 pi i m.x / N),  U_b the same with D = 1;
    ntri_t = sum_x U_b1 U_b2 U_b3 / N^3 (an integer: the closed triangles modulo N),
    B_t = (V^2 / N^12) sum_x I_b1 I_b2 I_b3 / ntri_t  for t = (b1 <= b2 <= b3).
"""
import itertools

import numpy as np


def triples(nb):
    return np.array(list(itertools.combinations_with_replacement(range(nb), 3)), dtype=np.intp).reshape(-1, 3)


def shell_map(N, L, edges):
    """(b, |k|): the shell index of every mode of the full grid (-1: none, k = 0 included) and its |k|."""
    idx = np.arange(N)
    m = np.where(idx < N // 2, idx, idx - N).astype(np.float64)
    kx = (m * (2. * np.pi / L[0]))[:, None, None]
    ky = (m * (2. * np.pi / L[1]))[None, :, None]
    kz = (m * (2. * np.pi / L[2]))[None, None, :]
    kk = np.sqrt((kx * kx + ky * ky) + kz * kz)
    edges = np.asarray(edges, dtype=np.float64)
    b = np.digitize(kk, edges) - 1
    b[b >= edges.size - 1] = -1
    b[0, 0, 0] = -1
    return b, kk


def _as_L(L):
    return (float(L),) * 3 if np.ndim(L) == 0 else tuple(float(x) for x in L)


def shell_cubes(d, L, edges, single=False, counts=True):
    """(I[nb][N^3], U[nb][N^3], D, b, |k|).  ``single``: the transforms of the data in single precision and the I_b
    rounded to it (what an f32 plan holds); the U_b are always fp64 (None unless ``counts``)."""
    d = np.asarray(d, dtype=np.float64)
    N = d.shape[0]
    L = _as_L(L)
    b, kk = shell_map(N, L, edges)
    nb = len(edges) - 1
    D = np.fft.fftn(d.astype(np.float32)) if single else np.fft.fftn(d)
    n3 = float(N) ** 3
    I = np.empty((nb, N, N, N))
    U = np.empty((nb, N, N, N)) if counts else None
    for q in range(nb):
        sel = b == q
        x = np.fft.ifftn(np.where(sel, D, 0).astype(D.dtype))
        if single:
            I[q] = (x.real.astype(np.float32) * np.float32(n3)).astype(np.float64)
        else:
            I[q] = x.real * n3
        if counts:
            U[q] = np.fft.ifftn(sel.astype(np.complex128)).real * n3
    return I, U, D, b, kk


def bispectrum(d, L, edges, single=False, ntri=None):
    """dict(k (T, 3), B (T,), Q (T,), ntri (T,), A (T,), sums (T,), nmodes (nb,), P (nb,), triples (T, 3)); A_t =
    (V^2 / N^12) sum_x |I_b1 I_b2 I_b3| / ntri_t is the scale of the rounding error of B_t.  ``single``: see shell_cubes.
    ``ntri``: the triangle counts of this grid and edge set from an earlier call (they are not formed again)."""
    L = _as_L(L)
    edges = np.asarray(edges, dtype=np.float64)
    I, U, D, b, kk = shell_cubes(d, L, edges, single=single, counts=ntri is None)
    nb = edges.size - 1
    N = I.shape[1]
    n3 = float(N) ** 3
    V = L[0] * L[1] * L[2]
    tri = triples(nb)
    T = tri.shape[0]
    sums, asums, usums = np.zeros(T), np.zeros(T), np.zeros(T)
    I2, U2 = I.reshape(nb, -1), (U.reshape(nb, -1) if ntri is None else None)
    Ia = np.abs(I2)
    for b3 in range(nb):                      # for a fixed third shell the sums are a matrix product over the voxels
        sel = np.nonzero(tri[:, 2] == b3)[0]
        r, c = tri[sel, 0], tri[sel, 1]
        sums[sel] = ((I2[:b3 + 1] * I2[b3]) @ I2[:b3 + 1].T)[r, c]
        asums[sel] = ((Ia[:b3 + 1] * Ia[b3]) @ Ia[:b3 + 1].T)[r, c]
        if ntri is None:
            usums[sel] = ((U2[:b3 + 1] * U2[b3]) @ U2[:b3 + 1].T)[r, c]
    if ntri is None:
        ntri = np.rint(usums / n3)
    else:
        ntri = np.array(ntri, dtype=np.float64)
        usums = ntri * n3
    nmodes = np.array([np.count_nonzero(b == q) for q in range(nb)], dtype=np.float64)
    D64 = D.astype(np.complex128)
    p2 = D64.real * D64.real + D64.imag * D64.imag
    with np.errstate(all="ignore"):
        kbar = np.array([np.sum(kk[b == q]) / nmodes[q] if nmodes[q] else np.nan for q in range(nb)])
        P = np.array([(V / (n3 * n3)) * np.sum(p2[b == q]) / nmodes[q] if nmodes[q] else np.nan for q in range(nb)])
        fac = (V * V) / (n3 ** 4)
        empty = ntri == 0
        B = np.where(empty, np.nan, fac * sums / ntri)
        A = np.where(empty, np.nan, fac * asums / ntri)
        k = kbar[tri]
        k[empty] = np.nan
        p1, p2_, p3 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
        Q = B / (p1 * p2_ + p2_ * p3 + p3 * p1)
    return dict(k=k, B=B, Q=Q, ntri=ntri, A=A, sums=sums, usums=usums, nmodes=nmodes, P=P, kbar=kbar, triples=tri)


def bispectrum_brute(d, L, edges):
    """(sums (T,), ntri (T,)): N^3 sum D(m1) D(m2) D(m3) and the count over the pairs (m1, m2) in S_b1 x S_b2 with
    m3 = -(m1 + m2) mod N in S_b3 -- what sum_x I_b1 I_b2 I_b3 and ntri are, without a transform of a shell."""
    d = np.asarray(d, dtype=np.float64)
    N = d.shape[0]
    L = _as_L(L)
    edges = np.asarray(edges, dtype=np.float64)
    b, _ = shell_map(N, L, edges)
    nb = edges.size - 1
    D = np.fft.fftn(d)
    tri = triples(nb)
    index = {tuple(t): q for q, t in enumerate(tri)}
    sums, cnt = np.zeros(tri.shape[0]), np.zeros(tri.shape[0])
    members = [np.argwhere(b == q) for q in range(nb)]
    for b1 in range(nb):
        m1 = members[b1]
        if not len(m1):
            continue
        d1 = D[m1[:, 0], m1[:, 1], m1[:, 2]]
        for b2 in range(b1, nb):
            m2 = members[b2]
            if not len(m2):
                continue
            d2 = D[m2[:, 0], m2[:, 1], m2[:, 2]]
            m3 = (-(m1[:, None, :] + m2[None, :, :])) % N
            b3 = b[m3[..., 0], m3[..., 1], m3[..., 2]]
            prod = (d1[:, None] * d2[None, :]) * D[m3[..., 0], m3[..., 1], m3[..., 2]]
            for q in range(b2, nb):
                sel = b3 == q
                t = index[(b1, b2, q)]
                cnt[t] = np.count_nonzero(sel)
                sums[t] = np.sum(prod[sel]).real * float(N) ** 3
    return sums, cnt
