"""Host statements of the three-point multipole moments, used only by tests.  Two statements written
apart: ``alm_statement`` follows the device's definition op for op -- the geometry of tests/fof_numpy.py, the harmonic
recurrence of include/fastbox_hip.h with its constants formed the same way, every sum over particles by ``math.fsum`` -- and
``legendre_statement`` is brute force over triplets with ``numpy.polynomial.legendre``, with no harmonics anywhere."""
import math

import numpy as np
from numpy.polynomial import legendre

from tests.fof_numpy import min_image, wrap


def constants(lmax):
    """A_m, sqrt(2 m + 3), alpha_lm, beta_lm, 4 pi / (2 l + 1) and sqrt(2), each formed in fp64 as fb_triplets.hip forms it."""
    A = np.zeros(lmax + 1)
    A[0] = np.sqrt(1.0 / (4.0 * np.pi))
    for m in range(1, lmax + 1):
        A[m] = A[m - 1] * np.sqrt((2.0 * m + 1.0) / (2.0 * m))
    G = np.array([np.sqrt(2.0 * m + 3.0) for m in range(lmax + 1)])
    al, be = np.zeros((lmax + 1, lmax + 1)), np.zeros((lmax + 1, lmax + 1))
    for l in range(2, lmax + 1):
        for m in range(0, l - 1):
            dl, dm, d1 = float(l), float(m), float(l) - 1.0
            al[l, m] = np.sqrt((4.0 * dl * dl - 1.0) / (dl * dl - dm * dm))
            be[l, m] = np.sqrt((d1 * d1 - dm * dm) / (4.0 * d1 * d1 - 1.0))
    fl = np.array([(4.0 * np.pi) / (2.0 * l + 1.0) for l in range(lmax + 1)])
    return A, G, al, be, fl, np.sqrt(2.0)


def neighbours(w, i, L, e2):
    """(indices, bins, dx, dy, dz, d2) of the particles j != i (by index) with e2[0] <= d^2 < e2[-1] around particle i of the
    wrapped positions w."""
    dx, dy, dz = [min_image(w[:, a] - w[i, a], L[a]) for a in range(3)]
    d2 = (dx * dx + dy * dy) + dz * dz
    ok = (d2 >= e2[0]) & (d2 < e2[-1])
    ok[i] = False
    j = np.nonzero(ok)[0]
    b = np.searchsorted(e2, d2[j], side='right') - 1
    return j, b, dx[j], dy[j], dz[j], d2[j]


def harmonics(x, y, z, lmax):
    """Y[l^2 + l + m] of unit vectors (arrays): the recurrence, every operation rounded on its own."""
    A, G, al, be, _, sq2 = constants(lmax)
    k = x.size
    c, s = [np.ones(k)], [np.zeros(k)]
    for m in range(1, lmax + 1):
        c.append(x * c[m - 1] - y * s[m - 1])
        s.append(x * s[m - 1] + y * c[m - 1])
    Y = np.zeros(((lmax + 1) ** 2, k))
    for m in range(lmax + 1):
        Q = {m: np.full(k, A[m])}
        if m + 1 <= lmax:
            Q[m + 1] = (G[m] * z) * Q[m]
        for l in range(m + 2, lmax + 1):
            Q[l] = al[l, m] * (z * Q[l - 1] - be[l, m] * Q[l - 2])
        for l in range(m, lmax + 1):
            if m == 0:
                Y[l * l + l] = Q[l]
            else:
                sq = sq2 * Q[l]
                Y[l * l + l + m] = sq * c[m]
                Y[l * l + l - m] = sq * s[m]
    return Y


def _prepare(pos, weights, L, edges):
    L = np.asarray(L, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    w = wrap(pos, L) if n else np.zeros((0, 3))
    wt = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    return L, w, wt, e * e, n, e.size - 1


def alm_statement(pos, weights, L, edges, lmax):
    """dict(alm (n, (lmax + 1)^2, nr), N int64 (n, nr), S (n, nr), A (n, nr) = sum_j |w_j|, M (lmax + 1, nr, nr),
    T (nr, nr) = sum_i |w_i| A_i(b1) A_i(b2), npairs int64 (nr,))."""
    L, w, wt, e2, n, nr = _prepare(pos, weights, L, edges)
    nlm = (lmax + 1) ** 2
    fl = constants(lmax)[4]
    alm, N, S, A = np.zeros((n, nlm, nr)), np.zeros((n, nr), dtype=np.int64), np.zeros((n, nr)), np.zeros((n, nr))
    terms = np.zeros((n, lmax + 1, nr, nr))
    for i in range(n):
        j, b, dx, dy, dz, d2 = neighbours(w, i, L, e2)
        if not j.size:
            continue
        r = np.sqrt(d2)
        Yw = wt[j][None, :] * harmonics(dx / r, dy / r, dz / r, lmax)
        for q in range(nr):
            sel = b == q
            if not sel.any():
                continue
            N[i, q] = sel.sum()
            S[i, q] = math.fsum((wt[j][sel] * wt[j][sel]).tolist())
            A[i, q] = math.fsum(np.abs(wt[j][sel]).tolist())
            alm[i, :, q] = [math.fsum(row) for row in Yw[:, sel].tolist()]
        a = alm[i]
        for l in range(lmax + 1):
            acc = np.zeros((nr, nr))
            for lm in range(l * l, l * l + 2 * l + 1):            # m ascending
                acc = acc + a[lm][:, None] * a[lm][None, :]
            terms[i, l] = wt[i] * (fl[l] * acc - np.diag(S[i]))
    M = np.array([math.fsum(col) for col in terms.reshape(n, -1).T.tolist()]).reshape(lmax + 1, nr, nr) if n else \
        np.zeros((lmax + 1, nr, nr))
    T = np.einsum('i,ib,ic->bc', np.abs(wt), A, A)
    return dict(alm=alm, N=N, S=S, A=A, M=M, T=T, npairs=N.sum(axis=0))


def legendre_statement(pos, weights, L, edges, lmax):
    """M (lmax + 1, nr, nr): the sum over ordered triplets (i; j != k) of w_i w_j w_k P_l(u_ij . u_ik), j in bin b1 and k in
    bin b2 of primary i."""
    L, w, wt, e2, n, nr = _prepare(pos, weights, L, edges)
    M = np.zeros((lmax + 1, nr, nr))
    for i in range(n):
        j, b, dx, dy, dz, d2 = neighbours(w, i, L, e2)
        if j.size < 2:
            continue
        u = np.stack([dx, dy, dz], axis=1) / np.sqrt(d2)[:, None]
        cosine = np.clip(u @ u.T, -1., 1.)
        P = legendre.legvander(cosine, lmax)                      # (k, k, lmax + 1)
        P[np.arange(j.size), np.arange(j.size), :] = 0.           # j != k
        B = (b[:, None] == np.arange(nr)[None, :]) * wt[j][:, None]
        M += wt[i] * np.einsum('jkl,jb,kc->lbc', P, B, B, optimize=True)
    return M


def gap(stmt, M_legendre):
    """The largest |M_alm - M_legendre| / T over the entries with T > 0; the other entries must agree exactly at 0."""
    T = stmt["T"]
    d = np.abs(stmt["M"] - M_legendre)
    assert np.all(d[:, T == 0.] == 0.)
    return float((d[:, T > 0.] / T[T > 0.]).max()) if np.any(T > 0.) else 0.
